"""Consistency regularisation: the bCR image transform and the two mean squared differences.

Drives csrc/cr.hip; composed in gan_lab_amd/consistency.py.  Re-exported by ``gan_lab_amd.ops``."""
import ctypes

import torch
from torch.autograd import Function

from .. import _lib
from .._lib import check
from .core import _c, _gpu_device, _new, _p, _st


# ---------------------------------------------------------------------------------------------- #
# consistency regularisation (csrc/cr.hip; consistency.py): the bCR image transform, the two mean squared differences
# ---------------------------------------------------------------------------------------------- #
def _cr_table(params, n, what):
    """A transform table at the ops boundary: a contiguous (n, 4) int32 device tensor."""
    if not isinstance(params, torch.Tensor) or not params.is_cuda or params.dtype != torch.int32:
        raise TypeError(f'gan_lab_amd.ops: {what} params must be an int32 tensor on the GPU (got {type(params).__name__}, '
                        f'{getattr(params, "device", None)}, {getattr(params, "dtype", None)}); the HIP path has no CPU fallback')
    if tuple(params.shape) != (n, 4):
        raise ValueError(f'{what}: params must have shape ({n}, 4), one (flip, dx, dy, 0) row per image (got '
                         f'{tuple(params.shape)})')
    return params if params.is_contiguous() else params.contiguous()


def cr_params(n, shift, flip, seed, offset, device, base=None):
    """(n, 4) int32 rows (flip, dx, dy, 0) of ``cr_transform`` from the Philox stream at ``offset`` (+ ``*base``: the step-scalar
    block of graphs.GraphedStep), one counter per row: flip in {0, 1} (0 when ``flip`` is False), dx, dy uniform in
    [-shift, shift]."""
    _gpu_device(device, 'cr_params')
    n, shift = int(n), int(shift)
    if n < 1 or shift < 0:
        raise ValueError(f'cr_params: needs n >= 1 and shift >= 0 (got {n}, {shift})')
    out = torch.empty((n, 4), dtype=torch.int32, device=device)
    check(_lib.lib().ganlab_cr_params_i32(ctypes.c_void_p(out.data_ptr()), n, shift, int(bool(flip)), int(seed) & (2 ** 64 - 1),
                                          int(offset) & (2 ** 64 - 1), _p(base), _st()), 'cr_params')
    return out


def cr_transform(x, params):
    """The bCR image transform: ``y[n,c,i,j] = x[n,c,i-dy, f(j-dx)]`` per row (flip, dx, dy, 0) of the (N, 4) int32 ``params``, f
    the horizontal mirror when flip is set, zero where the source leaves the image.  Bit-exact; no gradient (every transformed
    input of the critic step is detached)."""
    x = _c(x, 'cr_transform input')
    if x.dim() != 4:
        raise ValueError(f'cr_transform: needs an (N, C, H, W) batch (got {tuple(x.shape)})')
    if x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError('cr_transform has no adjoint: detach its input (consistency regularisation transforms detached '
                           'batches only)')
    n, c, h, w = x.shape
    params = _cr_table(params, n, 'cr_transform')
    y = torch.empty_like(x)
    check(_lib.lib().ganlab_cr_transform_f32(_p(x), ctypes.c_void_p(params.data_ptr()), _p(y), n, c, h, w, _st()),
          'cr_transform')
    return y


class _FirstOrderOnly(Function):
    """The gradients a first-order-only backward computed, tied to the op's inputs so that differentiating them - a second
    differentiation of the op - raises by the op's name instead of returning a silently wrong (or missing) second derivative."""

    @staticmethod
    def forward(ctx, name, n_inputs, *tensors):
        ctx.name = name
        return tuple(t.view_as(t) for t in tensors[n_inputs:])

    @staticmethod
    def backward(ctx, *gg):
        raise RuntimeError(f'gan_lab_amd.ops.{ctx.name} is first order only: its backward was asked to differentiate twice (no '
                           f'double backward is provided; keep it out of create_graph=True penalties)')


def _first_order(name, inputs, grads):
    """``grads`` as they are, or - while autograd is recording the backward (create_graph=True) - guarded by ``_FirstOrderOnly``."""
    if not torch.is_grad_enabled():
        return grads
    return _FirstOrderOnly.apply(name, len(inputs), *inputs, *grads)


class _CrMsd(Function):
    """mean_n (a_n - b_n)^2 of two score vectors -> 0-dim tensor; first order only."""

    @staticmethod
    def forward(ctx, a, b):
        out = _new((), a)
        check(_lib.lib().ganlab_cr_msd_fwd_f32(_p(a), _p(b), _p(out), a.numel(), _st()), 'cr_msd_fwd')
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        g1 = _c(gout.detach()).reshape(1)
        check(_lib.lib().ganlab_cr_msd_bwd_f32(_p(a), _p(b), _p(g1), _p(ga), _p(gb), a.numel(), _st()), 'cr_msd_bwd')
        return _first_order('cr_msd', (a, b, gout), (ga, gb))


def _cr_imsd_fwd(a, b, n):
    L = _lib.lib()
    ws = torch.empty((L.ganlab_cr_imsd_workspace(n) + 7) // 8, dtype=torch.float64, device=a.device)
    out = _new((), a)
    check(L.ganlab_cr_imsd_fwd_f32(_p(a), _p(b), _p(out), n, _p(ws), ws.numel() * 8, _st()), 'cr_imsd_fwd')
    return out


class _CrImsd(Function):
    """Mean over every element of (a - b)^2 for two image batches -> 0-dim tensor; first order only."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _cr_imsd_fwd(a, b, a.numel())

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        g1 = _c(gout.detach()).reshape(1)
        check(_lib.lib().ganlab_cr_imsd_bwd_f32(_p(a), _p(b), _p(g1), _p(ga), _p(gb), a.numel(), _st()), 'cr_imsd_bwd')
        return _first_order('cr_imsd', (a, b, gout), (ga, gb))


class _CrImsdHalves(Function):
    """``_CrImsd`` of the two halves of one contiguous (2N, ...) tensor: the backward writes both gradients into the halves of ONE
    gradient tensor, so the producer's backward starts from a single (2N, ...) cotangent."""

    @staticmethod
    def forward(ctx, both):
        ctx.save_for_backward(both)
        half = both.numel() // 2
        flat = both.view(-1)
        return _cr_imsd_fwd(flat[:half], flat[half:], half)

    @staticmethod
    def backward(ctx, gout):
        both, = ctx.saved_tensors
        half = both.numel() // 2
        flat, g = both.detach().view(-1), torch.empty_like(both)
        gflat = g.view(-1)
        g1 = _c(gout.detach()).reshape(1)
        check(_lib.lib().ganlab_cr_imsd_bwd_f32(_p(flat[:half]), _p(flat[half:]), _p(g1), _p(gflat[:half]), _p(gflat[half:]), half,
                                                _st()), 'cr_imsd_bwd')
        return _first_order('cr_imsd', (both, gout), (g,))[0]


def cr_msd(a, b):
    """Mean over the batch of the squared difference of two critic score vectors, (N,) or (N, 1): fp32 differences squared in
    fp32, summed in fp64 in a fixed order (bitwise reproducible).  Differentiable ONCE in both; a second differentiation raises."""
    a, b = _c(a, 'cr_msd a'), _c(b, 'cr_msd b')
    for t in (a, b):
        if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)) or t.numel() < 1:
            raise ValueError(f'cr_msd: scores must be (N,) or (N, 1) with N >= 1 (got {tuple(a.shape)} and {tuple(b.shape)})')
    if a.numel() != b.numel() or a.device != b.device:
        raise ValueError(f'cr_msd: the two score vectors differ ({tuple(a.shape)} on {a.device}, {tuple(b.shape)} on {b.device})')
    return _CrMsd.apply(a, b)


def cr_imsd(a, b=None):
    """Mean over all N*C*H*W elements of the squared difference of two equal-shaped image batches (fp64 partials per workgroup,
    summed in a fixed order: bitwise reproducible).  ``b=None``: ``a`` is one contiguous (2N, ...) tensor and its two halves are
    compared - the gradient then is ONE (2N, ...) tensor written in a single launch.  Differentiable ONCE; a second
    differentiation raises."""
    if b is None:
        a = _c(a, 'cr_imsd input')
        if a.dim() < 1 or a.shape[0] < 2 or a.shape[0] % 2:
            raise ValueError(f'cr_imsd: one tensor must hold two halves along its first axis (got {tuple(a.shape)})')
        return _CrImsdHalves.apply(a)
    a, b = _c(a, 'cr_imsd a'), _c(b, 'cr_imsd b')
    if a.shape != b.shape or a.device != b.device or a.numel() < 1:
        raise ValueError(f'cr_imsd: the two batches differ ({tuple(a.shape)} on {a.device}, {tuple(b.shape)} on {b.device})')
    return _CrImsd.apply(a, b)
