"""What every op family shares: pointer / stream plumbing, the operand checks at the ops boundary, and the three autograd
switches with their state (input-gradient-only mode, "no gradient towards this leaf", parameter gradients written straight into the
flat arena of ``optim.ParamArena``).

Drives no kernel file of its own except the row-workspace size query of csrc/norm.hip.  ``gan_lab_amd.ops`` re-exports every name
here.  A test rebinds ``ops.direct_param_grads``: it is defined here, and the learners reach the context manager
as ``ops.direct_param_grads``.  How many outputs went into an arena slot is counted here (``arena_takes``), whichever module the
launcher that calls ``_take`` lives in."""
import ctypes
import os

import torch

from .. import _lib


# ---------------------------------------------------------------------------------------------- #
# plumbing
# ---------------------------------------------------------------------------------------------- #
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# torch.cuda.current_stream() builds a Python Stream object through several layers of device-index resolution (~10 us;
# a quarter of the host time of a launch-bound step): ask the C binding for the raw handle of this process's device.
_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_GET_DEVICE = getattr(torch._C, '_cuda_getDevice', None)


def _st():
    if _RAW_STREAM is None or _GET_DEVICE is None:
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return ctypes.c_void_p(_RAW_STREAM(_GET_DEVICE()))      # two C calls (~0.3 us): follows torch.cuda.set_device


def _c(t, what='tensor'):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f'gan_lab_amd.ops: {what} must be a float32 tensor on the GPU (got '
                        f'{type(t).__name__}, {getattr(t, "device", None)}, {getattr(t, "dtype", None)}); '
                        f'the HIP path has no CPU fallback')
    return t if t.is_contiguous() else t.contiguous()


def _inplace(t, what):
    """``_c`` for an operand that a kernel updates in place through its raw pointer: a non-contiguous view is an error
    (``.contiguous()`` would update a copy)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f'gan_lab_amd.ops: {what} must be a float32 tensor on the GPU (got '
                        f'{type(t).__name__}, {getattr(t, "device", None)}, {getattr(t, "dtype", None)}); '
                        f'the HIP path has no CPU fallback')
    if not t.is_contiguous():
        raise ValueError(f'gan_lab_amd.ops: {what} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()}): '
                         f'the kernel updates it in place')
    return t


def _same_numel(op, named):
    """The raw-pointer ops walk every operand with the first one's element count."""
    n, dev = named[0][1].numel(), named[0][1].device
    for what, t in named[1:]:
        if t.numel() != n or t.device != dev:
            raise ValueError(f'gan_lab_amd.ops: {op}: {what} must have the {n} elements of {named[0][0]} on {dev} (got '
                             f'{t.numel()} on {t.device})')


def _gpu_device(device, what):
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: {what} draws on the GPU (got device {device!r}); the HIP path has no CPU fallback')


def _new(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _ct(t, dtype, what):
    """``_c`` for the non-fp32 operands of the SWD kernels (int32 centres, fp64 partials and statistics)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        raise TypeError(f'gan_lab_amd.ops: {what} must be a {dtype} tensor on the GPU (got {type(t).__name__}, '
                        f'{getattr(t, "device", None)}, {getattr(t, "dtype", None)}); the HIP path has no CPU fallback')
    return t if t.is_contiguous() else t.contiguous()


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _nchw(x):
    if x.dim() == 2:
        return x.shape[0], x.shape[1], 1
    n, c = x.shape[0], x.shape[1]
    hw = 1
    for s in x.shape[2:]:
        hw *= s
    return n, c, hw


def _row_workspace(rows, length, device):
    nbytes = _lib.lib().ganlab_ln_rowsums_workspace(rows, length)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


# ---- "input gradient only" mode ---------------------------------------------------------------------
# torch.autograd.grad(D(x), x, create_graph=True) (the gradient-penalty pass) only needs d/dx, but a
# Python autograd.Function cannot see which of its outputs the engine will keep: without this flag
# every conv would also run its weight-gradient kernel there and throw the result away.  The flag is
# a module global (the autograd engine runs backward on its own device thread).
_INPUT_GRAD_ONLY = [False]


class input_grad_only(object):
    def __enter__(self):
        self._prev = _INPUT_GRAD_ONLY[0]
        _INPUT_GRAD_ONLY[0] = True

    def __exit__(self, *exc):
        _INPUT_GRAD_ONLY[0] = self._prev
        return False


def _want_param_grads():
    return not _INPUT_GRAD_ONLY[0]


# ---- "no gradient towards this leaf" ----------------------------------------------------------------
# The mirror case: ``loss_d.backward()`` of the D step.  The real batch is a leaf with requires_grad (R1 needs
# d D/d x with create_graph=True), so the sweep would also produce d loss/d x - one input-gradient kernel of the
# first layer over the widest tensor of the network - which nobody reads.  ``with ops.no_grad_towards(x):`` makes the
# first layer's backward skip it (a Python autograd.Function cannot see that the engine will discard an output).
_NO_GRAD_TOWARDS = [None]


class no_grad_towards(object):
    def __init__(self, leaf):
        self.ptr = leaf.data_ptr() if leaf is not None else None

    def __enter__(self):
        self._prev = _NO_GRAD_TOWARDS[0]
        _NO_GRAD_TOWARDS[0] = self.ptr

    def __exit__(self, *exc):
        _NO_GRAD_TOWARDS[0] = self._prev
        return False


def _wants_input_grad(ctx, x):
    return ctx.needs_input_grad[0] and not (_NO_GRAD_TOWARDS[0] is not None and x.grad_fn is None and
                                            x.data_ptr() == _NO_GRAD_TOWARDS[0])


# ---- parameter gradients written straight into the flat arena ---------------------------------------
# ``loss.backward()`` hands every parameter gradient to an AccumulateGrad node: one ``grad += g`` launch per parameter and
# use (~250 per StyleGAN step - a fifth of the launches of the launch-bound configurations).  Inside
# ``with direct_param_grads():`` (the learners' backward sweeps) the gradient kernels of a parameter
# that lives in a ``ParamArena`` write their result INTO its (zeroed) arena slot when it is the first contribution of this
# step, and the Function returns None for it; later contributions of the same step (the critic is applied to two batches)
# take the ordinary accumulating path.  Never active while a differentiable backward is being recorded.
_DIRECT = [False]
_SINK, _TAKEN = {}, {}
_TAKE_HITS = [0]        # outputs that went into an arena slot, ever: the tests read the difference over a step


def direct_grads_enabled():
    """A/B knob GANLAB_DIRECT_GRADS=0.  The mechanism is the same with and without data parallelism: the reducer's
    post-accumulate hooks fire when a parameter's AccumulateGrad node runs - after EVERY contributing Function, direct or not -
    and a parameter whose Functions never ran (RgbHandoff) simply leaves its bucket to ``GradReducer.start``; the data-parallel
    code path on one rank (GANLAB_DIST_WORLD1=1) ends bit-identical to the plain one (tools/dist1_probe.py)."""
    import os
    return os.environ.get('GANLAB_DIRECT_GRADS') != '0'


class direct_param_grads(object):
    def __init__(self, enabled=True):
        self.enabled = bool(enabled)

    def __enter__(self):
        self._prev = _DIRECT[0]
        _DIRECT[0] = self.enabled
        _SINK.clear()
        _TAKEN.clear()

    def __exit__(self, *exc):
        _DIRECT[0] = self._prev
        _SINK.clear()
        _TAKEN.clear()
        return False


def _sink(name, p):
    """Offer parameter ``p``'s arena slot to the next launcher that allocates the output called ``name``."""
    if not _DIRECT[0] or p is None or torch.is_grad_enabled():
        return
    base = p._base if p._base is not None else p
    arena = getattr(base, '_ganlab_arena', None)
    if arena is None or not base.is_leaf or base.grad is None or base.numel() != p.numel() or \
            getattr(base, '_ganlab_written', -1) == arena.serial:
        return
    _SINK[name] = base


def _take(name, shape, like):
    """Output buffer ``name`` of a launcher: the offered arena slot (marked written for this step) or a fresh tensor."""
    if _SINK:
        base = _SINK.pop(name, None)
        if base is not None:
            n = 1
            for v in shape:
                n *= int(v)
            if base.grad.numel() == n and base.grad.device == like.device:
                base._ganlab_written = base._ganlab_arena.serial
                _TAKEN[name] = True
                _TAKE_HITS[0] += 1
                return base.grad.view(shape)
    return _new(shape, like)


def arena_takes():
    """How many ``_take`` calls have returned an arena slot so far (monotonic)."""
    return _TAKE_HITS[0]


def _sunk(name):
    """After the launcher: did it write the parameter's arena slot (-> the Function returns None for that gradient)?"""
    if _SINK:
        _SINK.pop(name, None)
    return _TAKEN.pop(name, False) if _TAKEN else False
