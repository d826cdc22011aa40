"""Counter-based random draws and the critic-input augmentations: DiffAugment and ADA (warp + color, then filter / noise /
cutout), each with its parameter rows, launchers and the Function pair forward / adjoint.

Drives the Philox entry points of csrc/pointwise.hip, csrc/sample.hip (``trunc_randn``), csrc/augment.hip, csrc/ada.hip and
csrc/ada_filter.hip; composed in gan_lab_amd/rng.py, augment.py, ada.py and sampling.py.  Re-exported by ``gan_lab_amd.ops``."""
import ctypes

import numpy as np

import torch
from torch.autograd import Function

from .. import _lib
from .._lib import check
from .core import _c, _gpu_device, _p, _st


def randn(shape, seed, offset, device):
    """Counter-based N(0,1) (Philox4x32-10 + Box-Muller) - replaces torch.randn for latents
    (utils/latent_utils.py:15) and per-layer noise (stylegan/architectures.py:115-116)."""
    _gpu_device(device, 'randn')
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_randn_f32(_p(out), out.numel(), int(seed) & (2 ** 64 - 1), int(offset), _st()), 'randn')
    return out


def check_truncation(threshold, what='threshold'):
    """The truncation threshold of ``trunc_randn`` as a float: finite and > 0, else ValueError."""
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f'{what} must be a finite number > 0 (got {threshold!r})') from None
    if isinstance(threshold, bool) or not (0.0 < t < float('inf')) or float(np.float32(t)) in (0.0, float('inf')):
        raise ValueError(f'{what} must be a finite number > 0 (got {threshold!r})')
    return t


def trunc_randn(shape, threshold, seed, offset, device):
    """Counter-based draws of N(0,1) truncated to [-threshold, threshold] by inverse CDF (csrc/sample.hip): ``randn``'s Philox
    counters - element i is word i % 4 of counter ``offset + i // 4`` - and its advance of ceil(n / 4), no rejection loop."""
    t = check_truncation(threshold)
    out = _c(torch.empty(shape, dtype=torch.float32, device=device), 'trunc_randn output')
    check(_lib.lib().ganlab_trunc_randn_f32(_p(out), out.numel(), t, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                            _st()), 'trunc_randn')
    return out


def randn_dev(shape, seed, base, delta, device):
    """``randn`` at stream position ``*base + delta`` (``base``: the step-scalar block of graphs.GraphedStep)."""
    _gpu_device(device, 'randn_dev')
    if not isinstance(base, torch.Tensor) or not base.is_cuda:
        raise TypeError(f'gan_lab_amd.ops: randn_dev base must be the step-scalar block, a tensor on the GPU (got '
                        f'{type(base).__name__}, {getattr(base, "device", None)}); the HIP path has no CPU fallback')
    if not base.is_contiguous() or base.numel() * base.element_size() < 8:
        raise ValueError(f'gan_lab_amd.ops: randn_dev base must be contiguous and hold the 8-byte stream position (got '
                         f'{base.numel()} x {base.dtype}, strides {base.stride()})')
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_randn_dev_f32(_p(out), out.numel(), int(seed) & (2 ** 64 - 1), _p(base), int(delta), _st()),
          'randn_dev')
    return out


def diffaug_params(n, h, w, seed, offset, device):
    """(n, 8) DiffAugment parameter rows (b, s, c, tx, ty, ox, oy, 0) from the Philox stream at ``offset`` (2 counters per row;
    csrc/augment.hip)."""
    out = torch.empty((int(n), 8), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_diffaug_params_f32(_p(out), int(n), int(h), int(w), int(seed) & (2 ** 64 - 1), int(offset), _st()),
          'diffaug_params')
    return out


def diffaug_params_dev(n, h, w, seed, base, delta, device):
    """``diffaug_params`` at stream position ``*base + delta`` (``base``: the step-scalar block of graphs.GraphedStep)."""
    out = torch.empty((int(n), 8), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_diffaug_params_dev_f32(_p(out), int(n), int(h), int(w), int(seed) & (2 ** 64 - 1), _p(base),
                                                   int(delta), _st()), 'diffaug_params_dev')
    return out


def k_diffaug(x, params, policy, adjoint=False):
    """DiffAugment of an (N, 3, H, W) batch (``adjoint``: the transpose of its linear part, applied to a cotangent)."""
    x, params = _c(x, 'diff_augment input'), _c(params, 'diff_augment params')
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[3] % 4 != 0 or tuple(params.shape) != (x.shape[0], 8):
        raise ValueError(f'diff_augment: needs an (N, 3, H, W) batch with W % 4 == 0 and (N, 8) params, got '
                         f'{tuple(x.shape)} and {tuple(params.shape)}')
    n, _, h, w = x.shape
    L = _lib.lib()
    nbytes = (L.ganlab_diffaug_bwd_workspace if adjoint else L.ganlab_diffaug_fwd_workspace)(n, h, w, int(policy))
    ws = torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    fn = L.ganlab_diffaug_bwd_f32 if adjoint else L.ganlab_diffaug_fwd_f32
    check(fn(_p(x), _p(params), _p(out), n, h, w, int(policy), _p(ws), ws.numel() * 4, _st()),
          'diffaug_bwd' if adjoint else 'diffaug_fwd')
    return out


ADA_ROW, ADA_COUNTERS = _lib.DEFINES['GANLAB_ADA_ROW'], _lib.DEFINES['GANLAB_ADA_COUNTERS']


def ada_params(n, h, w, state, policy, seed, offset, device):
    """(n, 32) ADA parameter rows (M, G, C, gates and raw geometric draws; csrc/ada.hip) from the Philox stream at ``offset``
    (8 counters per row).  ``state``: the device block whose first float is p; ``policy``: bit mask (``ada.parse_policy``)."""
    state = _c(state, 'ada_params state')
    out = torch.empty((int(n), ADA_ROW), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_ada_params_f32(_p(out), int(n), int(h), int(w), _p(state), int(policy), int(seed) & (2 ** 64 - 1),
                                           int(offset), _st()), 'ada_params')
    return out


def ada_params_dev(n, h, w, state, policy, seed, base, delta, device):
    """``ada_params`` at stream position ``*base + delta`` (``base``: the step-scalar block of graphs.GraphedStep)."""
    state = _c(state, 'ada_params state')
    out = torch.empty((int(n), ADA_ROW), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_ada_params_dev_f32(_p(out), int(n), int(h), int(w), _p(state), int(policy),
                                               int(seed) & (2 ** 64 - 1), _p(base), int(delta), _st()), 'ada_params_dev')
    return out


def k_ada(x, params, adjoint=False):
    """ADA warp + color matrix of an (N, 3, H, W) batch (``adjoint``: the transpose of its linear part, applied to a
    cotangent)."""
    x, params = _c(x, 'ada_augment input'), _c(params, 'ada_augment params')
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[3] % 4 != 0 or tuple(params.shape) != (x.shape[0], ADA_ROW):
        raise ValueError(f'ada_augment: needs an (N, 3, H, W) batch with W % 4 == 0 and (N, {ADA_ROW}) params, got '
                         f'{tuple(x.shape)} and {tuple(params.shape)}')
    n, _, h, w = x.shape
    out = torch.empty_like(x)
    L = _lib.lib()
    fn = L.ganlab_ada_bwd_f32 if adjoint else L.ganlab_ada_fwd_f32
    check(fn(_p(x), _p(params), _p(out), n, h, w, _st()), 'ada_bwd' if adjoint else 'ada_fwd')
    return out


ADA_EXT_ROW, ADA_EXT_COUNTERS, ADA_FILTER_TAPS, ADA_FILTER, ADA_NOISE, ADA_CUTOUT = (
    _lib.DEFINES['GANLAB_ADA_' + n] for n in ('EXT_ROW', 'EXT_COUNTERS', 'FILTER_TAPS', 'FILTER', 'NOISE', 'CUTOUT'))
ADA_NEW_GROUPS = ADA_FILTER | ADA_NOISE | ADA_CUTOUT


class AdaDraw(object):
    """What one ADA draw with a filter, noise or cutout group holds: the (N, 32) ``params`` rows, the (N, 16) ``ext`` rows and the
    (N, 3, H, W) ``noise`` field (None without the noise group).  Slicing along the batch slices all three, so a learner hands
    rows [0, B) to one batch and [B, 2B) to the other as it does with a plain tensor of rows."""

    def __init__(self, params, ext, noise=None):
        self.params, self.ext, self.noise = params, ext, noise

    def __getitem__(self, rows):
        if not isinstance(rows, slice):
            raise TypeError('AdaDraw: only slices along the batch are supported')
        return AdaDraw(self.params[rows], self.ext[rows], None if self.noise is None else self.noise[rows])

    def __len__(self):
        return self.params.shape[0]


def ada_filter_bank():
    """The library's (4, 43) float64 filter bank (csrc/ada_filter_bank.h), on the host."""
    out = torch.empty((4, ADA_FILTER_TAPS), dtype=torch.float64)
    check(_lib.lib().ganlab_ada_filter_bank(ctypes.c_void_p(out.data_ptr())), 'ada_filter_bank')
    return out


def ada_ext_params(n, h, w, state, policy, seed, offset, device):
    """(n, 16) ``ext`` rows of ADA's filter, noise and cutout groups (csrc/ada_filter.hip) from the Philox stream at ``offset``
    (4 counters per row): the position right after the main block of the batch, i.e. ``ada_params``' offset + 8 n."""
    state = _c(state, 'ada_ext_params state')
    out = torch.empty((int(n), ADA_EXT_ROW), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_ada_ext_params_f32(_p(out), int(n), int(h), int(w), _p(state), int(policy),
                                               int(seed) & (2 ** 64 - 1), int(offset), _st()), 'ada_ext_params')
    return out


def ada_ext_params_dev(n, h, w, state, policy, seed, base, delta, device):
    """``ada_ext_params`` at stream position ``*base + delta`` (``base``: the step-scalar block of graphs.GraphedStep)."""
    state = _c(state, 'ada_ext_params state')
    out = torch.empty((int(n), ADA_EXT_ROW), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_ada_ext_params_dev_f32(_p(out), int(n), int(h), int(w), _p(state), int(policy),
                                                   int(seed) & (2 ** 64 - 1), _p(base), int(delta), _st()),
          'ada_ext_params_dev')
    return out


def k_ada_ext(x, ext, noise=None, adjoint=False):
    """cutout(noise(filter(x))) of an (N, 3, H, W) batch under the (N, 16) ``ext`` rows (``adjoint``: F^T (mask o x), the
    transpose of its linear part, applied to a cotangent; ``noise`` is not read)."""
    x, ext = _c(x, 'ada_augment input'), _c(ext, 'ada_augment ext')
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[3] % 4 != 0 or x.shape[2] < 2 or \
            tuple(ext.shape) != (x.shape[0], ADA_EXT_ROW):
        raise ValueError(f'ada_augment: needs an (N, 3, H, W) batch with H >= 2, W % 4 == 0 and (N, {ADA_EXT_ROW}) ext rows, '
                         f'got {tuple(x.shape)} and {tuple(ext.shape)}')
    n, _, h, w = x.shape
    out = torch.empty_like(x)
    L = _lib.lib()
    if adjoint:
        check(L.ganlab_ada_ext_bwd_f32(_p(x), _p(ext), _p(out), n, h, w, _st()), 'ada_ext_bwd')
        return out
    if noise is not None:
        noise = _c(noise, 'ada_augment noise')
        if tuple(noise.shape) != tuple(x.shape):
            raise ValueError(f'ada_augment: the noise field must have the batch\'s shape {tuple(x.shape)}, got '
                             f'{tuple(noise.shape)}')
    check(L.ganlab_ada_ext_fwd_f32(_p(x), _p(ext), _p(noise) if noise is not None else None, _p(out), n, h, w, _st()),
          'ada_ext_fwd')
    return out


def ada_update(state, logits, interval, step_size, target):
    """The ADA controller (csrc/ada.hip) on the device block ``state`` = (p, acc_sum, acc_n, calls); ``logits`` None only
    counts the call.  In place, no host read: capturable."""
    state = _c(state, 'ada_update state')
    if tuple(state.shape) != (4,):
        raise ValueError(f'ada_update: state must be 4 floats (p, acc_sum, acc_n, calls), got {tuple(state.shape)}')
    n = 0
    if logits is not None:
        logits = _c(logits, 'ada_update logits').reshape(-1)
        n = logits.numel()
    check(_lib.lib().ganlab_ada_update_f32(_p(state), _p(logits) if n else None, n, int(interval), float(step_size),
                                           float(target), _st()), 'ada_update')
    return state


class _DiffAugment(Function):
    """DiffAugment (csrc/augment.hip): affine in x, so the backward is the adjoint of its linear part."""

    @staticmethod
    def forward(ctx, x, params, policy):
        ctx.params, ctx.policy = params, policy
        return k_diffaug(x, params, policy)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return _DiffAugmentAdjoint.apply(g, ctx.params, ctx.policy), None, None


class _DiffAugmentAdjoint(Function):
    @staticmethod
    def forward(ctx, g, params, policy):
        return k_diffaug(g, params, policy, adjoint=True)

    @staticmethod
    def backward(ctx, gg):
        raise NotImplementedError('diff_augment: double backward is not implemented (the penalties differentiate at the '
                                  'augmented batch, not through the augmentation)')


class _AdaAugment(Function):
    """ADA warp + color matrix (csrc/ada.hip), then with ``ext`` the filter, noise and cutout of csrc/ada_filter.hip: affine in
    x, so the backward is the adjoint of its linear part."""

    @staticmethod
    def forward(ctx, x, params, ext=None, noise=None):
        ctx.params, ctx.ext = params, ext
        y = k_ada(x, params)
        return y if ext is None else k_ada_ext(y, ext, noise)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return _AdaAugmentAdjoint.apply(g, ctx.params, ctx.ext), None, None, None


class _AdaAugmentAdjoint(Function):
    @staticmethod
    def forward(ctx, g, params, ext=None):
        if ext is not None:
            g = k_ada_ext(g, ext, adjoint=True)
        return k_ada(g, params, adjoint=True)

    @staticmethod
    def backward(ctx, gg):
        raise NotImplementedError('ada_augment: double backward is not implemented (the penalties differentiate at the '
                                  'augmented batch, not through the augmentation)')


def diff_augment(x, params, policy):
    """DiffAugment (Zhao et al. 2020) of an (N, 3, H, W) fp32 batch on the GPU: ``params`` (N, 8) rows
    (b, s, c, tx, ty, ox, oy, 0) (``rng.augment_params``), ``policy`` a bit mask (``augment.parse_policy``).  Differentiable
    once in ``x``."""
    for t, what in ((x, 'diff_augment input'), (params, 'diff_augment params')):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            _c(t, what)                 # raises TypeError: there is no CPU path
    return _DiffAugment.apply(x, params.detach(), int(policy))


def ada_augment(x, params, ext=None, noise=None):
    """ADA (Karras et al. 2020) of an (N, 3, H, W) fp32 batch on the GPU: affine bilinear warp with zero fill, then a 3x4
    color matrix, per sample from the (N, 32) ``params`` rows (``rng.ada_params`` or ``ada.rows_from_matrices``).  With
    ``ext`` ((N, 16) rows: ``rng.ada_params`` under a policy with filter, noise or cutout, or ``ada.ext_rows``) the result
    goes on through the per-sample 43-tap filter, ``sigma * noise`` (``noise``: an (N, 3, H, W) field of standard normals;
    None adds none, whatever sigma says) and the cutout rectangle; with ``ext`` None nothing further is launched.
    Differentiable once in ``x``."""
    for t, what in ((x, 'ada_augment input'), (params, 'ada_augment params')) + \
            (((ext, 'ada_augment ext'),) if ext is not None else ()) + (((noise, 'ada_augment noise'),) if noise is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            _c(t, what)                 # raises TypeError: there is no CPU path
    if ext is None:
        if noise is not None:
            raise ValueError('ada_augment: a noise field needs ext rows (their sigma scales it)')
        return _AdaAugment.apply(x, params.detach())
    return _AdaAugment.apply(x, params.detach(), ext.detach(), None if noise is None else noise.detach())
