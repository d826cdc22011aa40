"""Class labels at the ops boundary, label draws and conditional BatchNorm.

Drives csrc/cond.hip and the batch-statistics kernels of csrc/norm.hip; composed in gan_lab_amd/conditional.py.  Re-exported by
``gan_lab_amd.ops``."""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import ACT_LRELU, ACT_NONE, check
from .core import _c, _nchw, _new, _p, _row_workspace, _st, _want_param_grads


# ---------------------------------------------------------------------------------------------- #
# class conditioning (csrc/cond.hip; conditional.py): conditional BatchNorm, the projection critic's class term
# ---------------------------------------------------------------------------------------------- #
def _labels(labels, n, what):
    """Class labels at the ops boundary: a device tensor of shape (n,), int32 (int64 is converted)."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'gan_lab_amd.ops: {what} labels must be an int32 / int64 tensor on the GPU (got '
                        f'{type(labels).__name__}, {getattr(labels, "device", None)}, {getattr(labels, "dtype", None)}); '
                        f'the HIP path has no CPU fallback')
    if tuple(labels.shape) != (n,):
        raise ValueError(f'{what}: labels must have shape ({n},), one per sample (got {tuple(labels.shape)})')
    if labels.dtype != torch.int32:
        labels = labels.to(torch.int32)
    return labels if labels.is_contiguous() else labels.contiguous()


def randint(n, high, seed, offset, device):
    """``n`` int32 labels uniform in [0, high) from the Philox stream at (seed, offset); (n + 3) // 4 counters."""
    out = torch.empty(int(n), dtype=torch.int32, device=device)
    check(_lib.lib().ganlab_randint_i32(ctypes.c_void_p(out.data_ptr()), int(n), int(high),
                                        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _st()), 'randint')
    return out


def _bn_batch_stats(x, running_mean, running_var, momentum, eps, batches):
    """The batch statistics of ``x`` and BatchNorm's running-estimate / counter bookkeeping on ``batch_norm``'s own kernels
    (3 launches), without an affine.  -> fin (4, C): mean, biased variance, rstd, rstd again (no weight to fold in here)."""
    n, c, hw = _nchw(x)
    m = n * hw
    L = _lib.lib()
    with torch.no_grad():
        ws = _row_workspace(c, m, x.device)
        mom = _new((c, 3), x)
        check(L.ganlab_bn_stats_f32(_p(x), _p(mom), n, c, hw, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _st()),
              'bn_stats')
        fin = _new((4, c), x)
        for buf in (running_mean, running_var, batches):
            assert buf is None or (buf.is_contiguous() and buf.device == x.device)
        assert batches is None or batches.dtype == torch.int64
        check(L.ganlab_bn_finalize_f32(_p(mom), None, _p(running_mean) if running_mean is not None else None,
                                       _p(running_var) if running_var is not None else None,
                                       ctypes.c_void_p(batches.data_ptr()) if batches is not None else None, _p(fin), c,
                                       float(eps), float(momentum), m / max(m - 1, 1), _st()), 'bn_finalize')
    return fin


class _CondBatchNorm(Function):
    """Normalise with the given per-channel ``mean`` / ``rstd`` and apply the affine row of each sample's class (+ the
    LeakyReLU behind it) in one pass.  ``batch_stats``: mean / rstd are the statistics of ``x`` itself (training mode) and the
    backward carries their derivative; otherwise (eval mode) they are constants.  First order only, like ``_BatchNormTrain``:
    the generator is never inside a gradient penalty.  Backward: 3 launches, the table gradients as ordinary tensors."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, mean, rstd, act_slope, batch_stats):
        n, c, hw = _nchw(x)
        k = weight.shape[0]
        y = torch.empty_like(x)
        check(_lib.lib().ganlab_cbn_apply_f32(_p(x), _p(mean), _p(rstd), _p(weight), _p(bias), _p(labels), _p(y), n, c, hw, k,
                                              ACT_LRELU if act_slope is not None else ACT_NONE,
                                              float(act_slope) if act_slope is not None else 1.0, _st()), 'cbn_apply')
        ctx.save_for_backward(x, weight, labels, mean, rstd, y if act_slope is not None else None)
        ctx.act_slope, ctx.batch_stats = act_slope, bool(batch_stats)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, labels, mean, rstd, yact = ctx.saved_tensors
        gy = _c(gy)
        n, c, hw = _nchw(x)
        k = weight.shape[0]
        L = _lib.lib()
        ws = torch.empty((L.ganlab_cbn_bwd_workspace(n, c) + 7) // 8, dtype=torch.float64, device=x.device)
        gz = torch.empty_like(gy) if yact is not None else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw, gb, sums = _new((k, c), x), _new((k, c), x), _new((c, 2), x)
        check(L.ganlab_cbn_bwd_f32(_p(gy), _p(x), _p(mean), _p(rstd), _p(weight), _p(labels), _p(yact), _p(gz), _p(gx), _p(gw),
                                   _p(gb), _p(sums), n, c, hw, k, int(ctx.batch_stats),
                                   float(ctx.act_slope) if yact is not None else 1.0, ctypes.c_void_p(ws.data_ptr()),
                                   ws.numel() * 8, _st()), 'cbn_bwd')
        want_p = _want_param_grads()
        return (gx, gw if (want_p and ctx.needs_input_grad[1]) else None, gb if (want_p and ctx.needs_input_grad[2]) else None,
                None, None, None, None, None)


def cond_batch_norm(x, weight, bias, labels, running_mean, running_var, training, momentum=0.1, eps=1e-5, batches=None,
                    act_slope=None):
    """Class-conditional BatchNorm: ``batch_norm`` whose affine is row ``labels[n]`` of the (K, C) tables ``weight`` / ``bias``
    for sample n.  Training mode: batch statistics and the running-estimate / counter bookkeeping on ``batch_norm``'s own
    kernels (3 launches), then one apply pass; eval mode: the same apply pass with the running statistics."""
    x, weight, bias = _c(x, 'cond_batch_norm input'), _c(weight, 'cond_batch_norm weight'), _c(bias, 'cond_batch_norm bias')
    n, c, hw = _nchw(x)
    labels = _labels(labels, n, 'cond_batch_norm')
    if weight.dim() != 2 or weight.shape[1] != c or bias.shape != weight.shape:
        raise ValueError(f'cond_batch_norm: weight / bias must be (num_classes, {c}) tables (got {tuple(weight.shape)}, '
                         f'{tuple(bias.shape)})')
    slope = None if act_slope is None else float(act_slope)
    if not training:
        mean, rstd = _c(running_mean), torch.rsqrt(running_var + eps)
        return _CondBatchNorm.apply(x, weight, bias, labels, mean, rstd, slope, False)
    fin = _bn_batch_stats(x, running_mean, running_var, momentum, eps, batches)
    return _CondBatchNorm.apply(x, weight, bias, labels, fin[0], fin[2], slope, True)
