"""BigGAN's generator conditioning - the batched modulation of hierarchical latents with a shared class embedding, the modulated
BatchNorm - and the projection critic's class term.

Drives csrc/hier.hip and csrc/cond.hip (``class_projection``); composed in gan_lab_amd/hier_latent.py and conditional.py.
Re-exported by ``gan_lab_amd.ops``."""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import ACT_LRELU, ACT_NONE, check
from .core import _c, _DIRECT, _nchw, _new, _p, _st, _want_param_grads
from .cond import _bn_batch_stats, _labels


# ---------------------------------------------------------------------------------------------- #
# hierarchical latents + shared class embedding (csrc/hier.hip; hier_latent.py): the batched modulation, the modulated BatchNorm
# ---------------------------------------------------------------------------------------------- #
def _slot_open(p):
    """May this step's first gradient of parameter ``p`` be written straight into its arena slot (``_sink``'s rule)?"""
    arena = getattr(p, '_ganlab_arena', None)
    return _DIRECT[0] and not torch.is_grad_enabled() and arena is not None and p.is_leaf and p.grad is not None and \
        getattr(p, '_ganlab_written', -1) != arena.serial


class HierTable(object):
    """Device-resident job table of ``ganlab_hier_fwd_f32`` / ``ganlab_hier_bwd_f32``.  ``jobs``: one dict per modulation linear,
    in column order, with ``w`` (the (C, D) float32 GPU parameter, contiguous), ``z_off`` / ``z_len`` (its chunk of the latent;
    D = z_len + embed), ``scale`` and ``one`` (1 for a gain, 0 for a shift).  ``shared``: the (num_classes, embed) embedding
    parameter or None.  Job j owns columns [cols[j], cols[j] + C_j) of the (N, T) buffer.  A weight that lives in an arena
    (``optim.ParamArena``) gets its gradient written into its arena slot inside ``direct_param_grads``; otherwise, and for every
    later use in the same step, the gradients come back as ordinary tensors from the table's own buffer.  Built and uploaded
    once (outside any capture); keeps the tensors it points at alive."""

    def __init__(self, jobs, len_latent, shared=None):
        if not jobs:
            raise ValueError('HierTable: no jobs')
        self.weights = [d['w'] for d in jobs]
        self.shared = shared
        dev = self.weights[0].device
        self.len_latent = int(len_latent)
        self.embed = int(shared.shape[1]) if shared is not None else 0
        self.num_classes = int(shared.shape[0]) if shared is not None else 0
        if shared is not None:
            _c(shared, 'HierTable shared')
            if shared.dim() != 2 or not shared.is_contiguous() or shared.device != dev:
                raise ValueError(f'HierTable: shared must be a contiguous (num_classes, E) tensor on {dev}')
        self.cols, self.widths, self.own_offsets = [], [], []
        col = own = bf = bw = 0
        arr = (_lib.HierJob * len(jobs))()
        for j, d in zip(arr, jobs):
            w, z_off, z_len = d['w'], int(d['z_off']), int(d['z_len'])
            _c(w, 'HierTable w')
            D = z_len + self.embed
            if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] != D or D < 1 or not w.is_contiguous() or w.device != dev:
                raise ValueError(f'HierTable: w must be a contiguous (C, {D}) tensor on {dev} (got {tuple(w.shape)})')
            if z_len < 0 or z_off < 0 or z_off + z_len > self.len_latent:
                raise ValueError(f'HierTable: chunk [{z_off}, {z_off + z_len}) leaves the latent [0, {self.len_latent})')
            C = int(w.shape[0])
            self.cols.append(col)
            self.widths.append(C)
            self.own_offsets.append(own)
            j.C, j.z_off, j.z_len, j.col, j.scale, j.one = C, z_off, z_len, col, float(d['scale']), float(d['one'])
            j.blk_f0, j.blk_w0 = bf, bw
            col += C
            own += (C * D + 3) // 4 * 4
            bf += (C + 63) // 64
            bw += (C * D + 255) // 256
        self.T, self.blocks = col, (bf, bw)
        self.gw_own = torch.zeros(own, dtype=torch.float32, device=dev)
        self.in_arena = all(getattr(w, '_ganlab_arena', None) is not None and w.grad is not None and
                            w.grad.is_contiguous() for w in self.weights)
        for j, w, o in zip(arr, self.weights, self.own_offsets):
            j.w = w.data_ptr()
            j.gw = w.grad.data_ptr() if self.in_arena else None
            j.gw_own = self.gw_own.data_ptr() + 4 * o
        self.n = len(jobs)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.pointers = self._pointers()
        self._grad = {}

    def _pointers(self):
        ts = self.weights + ([self.shared] if self.shared is not None else [])
        return tuple(t.data_ptr() for t in ts) + tuple(t.grad.data_ptr() if t.grad is not None else 0 for t in self.weights)

    def is_current(self):
        """Do the parameters still lie where the uploaded table points?"""
        return self.pointers == self._pointers()

    def grad_buffer(self, n):
        """The (n, T) gradient buffer that ``mod_batch_norm`` writes d gain / d shift into and ``hier_modulate``'s backward reads."""
        g = self._grad.get(n)
        if g is None:
            g = self._grad[n] = torch.zeros(n, self.T, dtype=torch.float32, device=self.table.device)
        return g


class _HierModulate(Function):
    """out (N, T) = every gain (1 + s <W, cond>) and shift (s <W, cond>) of ``table`` in one launch.  Backward (first order, at
    most 3 launches): the incoming gradient, or - when every consumer wrote its columns into ``table.grad_buffer(N)`` and handed
    back None - that buffer."""

    @staticmethod
    def forward(ctx, table, z, shared, labels, *weights):
        n = z.shape[0]
        out = _new((n, table.T), z)
        bf, _ = table.blocks
        check(_lib.lib().ganlab_hier_fwd_f32(table.table.data_ptr(), table.n, bf, _p(z), _p(shared), _p(labels), _p(out), n,
                                             table.T, table.len_latent, table.embed, max(table.num_classes, 1), _st()),
              'hier_fwd')
        ctx.table = table
        ctx.save_for_backward(z, shared, labels)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        table = ctx.table
        z, shared, labels = ctx.saved_tensors
        n = z.shape[0]
        g = table.grad_buffer(n) if g is None else _c(g)
        want_w = _want_param_grads() and any(ctx.needs_input_grad[4:])
        direct = want_w and table.in_arena and all(_slot_open(w) for w in table.weights)
        dz = _new(z.shape, z) if ctx.needs_input_grad[1] else None
        dshared = de = None
        shared_direct = False
        if shared is not None and ctx.needs_input_grad[2] and _want_param_grads():
            de = _new((n, table.embed), z)
            shared_direct = _slot_open(shared) and shared.grad.is_contiguous()
            dshared = shared.grad if shared_direct else _new(shared.shape, z)
        _, bw = table.blocks
        check(_lib.lib().ganlab_hier_bwd_f32(table.table.data_ptr(), table.n, bw, _p(g), _p(z), _p(shared), _p(labels), _p(dz),
                                             _p(de), _p(dshared), n, table.T, table.len_latent, table.embed,
                                             max(table.num_classes, 1), 0 if direct else 1, _st()), 'hier_bwd')
        if direct:
            for w in table.weights:
                w._ganlab_written = w._ganlab_arena.serial
            gws = [None] * table.n
        elif want_w:
            own = table.gw_own.clone()
            gws = [own[o:o + w.numel()].view(w.shape) if need else None
                   for o, w, need in zip(table.own_offsets, table.weights, ctx.needs_input_grad[4:])]
        else:
            gws = [None] * table.n
        if shared_direct:
            shared._ganlab_written = shared._ganlab_arena.serial
            dshared = None
        return (None, dz, dshared, None) + tuple(gws)


def hier_modulate(table, z, labels=None):
    """The flat (N, T) modulation buffer of ``table`` (a ``HierTable``) for the latents ``z`` (N, len_latent) and, with a shared
    embedding, the int32 device ``labels`` (N,): column ``table.cols[j] + c`` holds ``one_j + s_j <W_j[c], cond_j[n]>``.
    Differentiable once towards ``z``, the embedding and every weight."""
    z = _c(z, 'hier_modulate z')
    if z.dim() != 2 or z.shape[1] != table.len_latent or z.shape[0] < 1:
        raise ValueError(f'hier_modulate: z must be (N, {table.len_latent}) (got {tuple(z.shape)})')
    if not table.is_current():
        raise RuntimeError('hier_modulate: the parameters moved since the job table was uploaded; rebuild the table')
    if table.shared is not None:
        if labels is None:
            raise TypeError('hier_modulate: the table has a shared class embedding: labels are required')
        labels = _labels(labels, z.shape[0], 'hier_modulate')
    else:
        labels = None
    return _HierModulate.apply(table, z, table.shared, labels, *table.weights)


class _ModBatchNorm(Function):
    """Normalise with the given per-channel ``mean`` / ``rstd`` and apply each sample's own gain / shift row (+ the LeakyReLU
    behind it) in one pass.  The rows are columns [gcol, gcol + C) / [scol, scol + C) of ``gsrc`` / ``ssrc``.  With ``sink`` (the
    (N, T) gradient buffer of a ``HierTable``) the backward writes d gain / d shift into the same columns of it and returns None
    towards ``token`` (the modulation buffer these rows were cut from, which keeps its backward behind this one); without, it
    returns them as tensors.  First order only, like ``_CondBatchNorm``."""

    @staticmethod
    def forward(ctx, x, gsrc, ssrc, token, gcol, scol, mean, rstd, act_slope, batch_stats, sink):
        n, c, hw = _nchw(x)
        y = torch.empty_like(x)
        gs, ss = gsrc.stride(0), ssrc.stride(0)
        check(_lib.lib().ganlab_mbn_apply_f32(_p(x), _p(mean), _p(rstd), ctypes.c_void_p(gsrc.data_ptr() + 4 * gcol), gs,
                                              ctypes.c_void_p(ssrc.data_ptr() + 4 * scol), ss, _p(y), n, c, hw,
                                              ACT_LRELU if act_slope is not None else ACT_NONE,
                                              float(act_slope) if act_slope is not None else 1.0, _st()), 'mbn_apply')
        ctx.save_for_backward(x, gsrc, mean, rstd, y if act_slope is not None else None)
        ctx.act_slope, ctx.batch_stats, ctx.sink, ctx.cols = act_slope, bool(batch_stats), sink, (gcol, scol)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, gsrc, mean, rstd, yact = ctx.saved_tensors
        if gy is None:
            return (None,) * 11
        gy = _c(gy)
        n, c, hw = _nchw(x)
        gcol, scol = ctx.cols
        L = _lib.lib()
        ws = torch.empty((L.ganlab_mbn_bwd_workspace(n, c) + 7) // 8, dtype=torch.float64, device=x.device)
        gz = torch.empty_like(gy) if yact is not None else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        sums = _new((c, 2), x)
        sink = ctx.sink
        dg = ds = None
        if sink is not None:
            pg, ps, stride = sink.data_ptr() + 4 * gcol, sink.data_ptr() + 4 * scol, sink.stride(0)
        elif ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dg, ds = _new((n, c), x), _new((n, c), x)
            pg, ps, stride = dg.data_ptr(), ds.data_ptr(), c
        else:
            pg = ps = None
            stride = c
        check(L.ganlab_mbn_bwd_f32(_p(gy), _p(x), _p(mean), _p(rstd), ctypes.c_void_p(gsrc.data_ptr() + 4 * gcol), gsrc.stride(0),
                                   _p(yact), _p(gz), _p(gx), ctypes.c_void_p(pg) if pg else None,
                                   ctypes.c_void_p(ps) if ps else None, stride, _p(sums), n, c, hw, int(ctx.batch_stats),
                                   float(ctx.act_slope) if yact is not None else 1.0, ctypes.c_void_p(ws.data_ptr()),
                                   ws.numel() * 8, _st()), 'mbn_bwd')
        return (gx, dg if ctx.needs_input_grad[1] else None, ds if ctx.needs_input_grad[2] else None) + (None,) * 8


def _mod_rows(t, n, c, what):
    _c(t, what)
    if t.dim() != 2 or tuple(t.shape) != (n, c) or (c > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < c):
        raise ValueError(f'mod_batch_norm: {what} must be ({n}, {c}) with unit column stride - a contiguous tensor or a column '
                         f'slice of an (N, T) buffer (got {tuple(t.shape)}, strides {tuple(t.stride())})')
    return t


def _mod_stats(x, running_mean, running_var, training, momentum, eps, batches):
    if not training:
        return _c(running_mean), torch.rsqrt(running_var + eps)
    fin = _bn_batch_stats(x, running_mean, running_var, momentum, eps, batches)
    return fin[0], fin[2]


def mod_batch_norm(x, gain, shift, running_mean, running_var, training, momentum=0.1, eps=1e-5, batches=None,
                   act_slope=None):
    """Modulated BatchNorm: ``batch_norm`` whose affine is sample n's own row of the (N, C) tensors ``gain`` / ``shift`` -
    contiguous, or column slices of one flat (N, T) buffer (row stride T), read where they lie.  Statistics, bookkeeping and
    eval mode as ``cond_batch_norm``; equal rows reproduce ``batch_norm`` bit for bit.  First order."""
    x = _c(x, 'mod_batch_norm input')
    n, c, hw = _nchw(x)
    gain, shift = _mod_rows(gain, n, c, 'gain'), _mod_rows(shift, n, c, 'shift')
    slope = None if act_slope is None else float(act_slope)
    mean, rstd = _mod_stats(x, running_mean, running_var, training, momentum, eps, batches)
    # a 1-row view may report any row stride: the kernels never step over a row then
    return _ModBatchNorm.apply(x, gain if n > 1 or gain.stride(0) >= c else gain.contiguous(),
                               shift if n > 1 or shift.stride(0) >= c else shift.contiguous(), None, 0, 0, mean, rstd, slope,
                               bool(training), None)


def mod_batch_norm_cols(x, mod, flat, sink, gcol, scol, running_mean, running_var, training, momentum=0.1, eps=1e-5,
                        batches=None, act_slope=None):
    """``mod_batch_norm`` for the layers of a network: gain / shift are columns [gcol, gcol + C) / [scol, scol + C) of ``flat`` =
    ``mod.detach()``, ``mod`` the output of ``hier_modulate``; d gain / d shift go straight into the same columns of ``sink`` =
    ``table.grad_buffer(N)`` (None when ``mod`` carries no gradient) - no per-layer slice, zero-fill or add - and ``mod``'s backward
    picks them up there."""
    x = _c(x, 'mod_batch_norm input')
    n, c, hw = _nchw(x)
    if flat.dim() != 2 or flat.shape[0] != n or not flat.is_contiguous() or max(gcol, scol) + c > flat.shape[1] or \
            min(gcol, scol) < 0 or (sink is not None and (sink.shape != flat.shape or not sink.is_contiguous())):
        raise ValueError(f'mod_batch_norm_cols: columns [{gcol}, +{c}) / [{scol}, +{c}) do not fit the ({n}, T) buffers '
                         f'(got {tuple(flat.shape)})')
    slope = None if act_slope is None else float(act_slope)
    mean, rstd = _mod_stats(x, running_mean, running_var, training, momentum, eps, batches)
    return _ModBatchNorm.apply(x, flat, flat, mod, int(gcol), int(scol), mean, rstd, slope, bool(training),
                               sink if mod.requires_grad else None)


def _proj_dims(f, weight, what):
    if f.dim() != 2 or weight.dim() != 2 or f.shape[1] != weight.shape[1]:
        raise ValueError(f'{what}: features (N, F) and weight (K, F) do not fit (got {tuple(f.shape)}, {tuple(weight.shape)})')
    return f.shape[0], f.shape[1], weight.shape[0]


class _ClassProj(Function):
    """P(f, W, l, base)[n] = base[n] + <W[l_n], f[n]>.  d/df = G(g, W, l), d/dW = S(g, f, l), d/dbase = g."""

    @staticmethod
    def forward(ctx, f, weight, labels, base):
        f, weight = _c(f, 'class_projection features'), _c(weight, 'class_projection weight')
        n, nf, k = _proj_dims(f, weight, 'class_projection')
        base = _c(base, 'class_projection base').reshape(n) if base is not None else None
        out = _new((n,), f)
        check(_lib.lib().ganlab_proj_fwd_f32(_p(f), _p(weight), _p(labels), _p(base), _p(out), n, nf, k, _st()), 'proj_fwd')
        ctx.save_for_backward(f, weight, labels)
        ctx.has_base = base is not None
        return out

    @staticmethod
    def backward(ctx, g):
        f, weight, labels = ctx.saved_tensors
        gf = _ClassProjDfeat.apply(g, weight, labels) if ctx.needs_input_grad[0] else None
        gw = _ClassProjDweight.apply(g, f, labels, weight.shape[0]) if (ctx.needs_input_grad[1] and _want_param_grads()) \
            else None
        return gf, gw, None, g if (ctx.has_base and ctx.needs_input_grad[3]) else None


class _ClassProjDfeat(Function):
    """G(g, W, l)[n,j] = g[n] W[l_n,j].  d/dg = P(cot, W, l, 0), d/dW = S(g, cot, l)."""

    @staticmethod
    def forward(ctx, g, weight, labels):
        g, weight = _c(g), _c(weight)
        k, nf = weight.shape
        n = g.numel()
        out = _new((n, nf), g)
        check(_lib.lib().ganlab_proj_dfeat_f32(_p(g), _p(weight), _p(labels), _p(out), n, nf, k, _st()), 'proj_dfeat')
        ctx.save_for_backward(g, weight, labels)
        return out

    @staticmethod
    def backward(ctx, cot):
        g, weight, labels = ctx.saved_tensors
        gg = _ClassProj.apply(cot, weight, labels, None).view(g.shape) if ctx.needs_input_grad[0] else None
        gw = _ClassProjDweight.apply(g, cot, labels, weight.shape[0]) if (ctx.needs_input_grad[1] and _want_param_grads()) \
            else None
        return gg, gw, None


class _ClassProjDweight(Function):
    """S(g, f, l)[k,j] = sum_{n: l_n = k} g[n] f[n,j].  d/dg = P(f, cot, l, 0), d/df = G(g, cot, l)."""

    @staticmethod
    def forward(ctx, g, f, labels, k):
        g, f = _c(g), _c(f)
        n, nf = f.shape
        out = _new((k, nf), f)
        check(_lib.lib().ganlab_proj_dweight_f32(_p(g), _p(f), _p(labels), _p(out), n, nf, k, _st()), 'proj_dweight')
        ctx.save_for_backward(g, f, labels)
        return out

    @staticmethod
    def backward(ctx, cot):
        g, f, labels = ctx.saved_tensors
        gg = _ClassProj.apply(f, cot, labels, None).view(g.shape) if ctx.needs_input_grad[0] else None
        gf = _ClassProjDfeat.apply(g, cot, labels) if ctx.needs_input_grad[1] else None
        return gg, gf, None, None


def class_projection(f, weight, labels, base=None):
    """The projection critic's output (Miyato & Koyama 2018): ``base[n] + <weight[labels[n]], f[n]>`` for features (N, F), a
    (K, F) class embedding and the unconditional score ``base`` (N,) (None: 0).  Any order of differentiation."""
    if not isinstance(f, torch.Tensor) or f.dim() != 2:
        raise ValueError('class_projection: features must be an (N, F) tensor')
    return _ClassProj.apply(f, weight, _labels(labels, f.shape[0], 'class_projection'), base)
