"""Projection into StyleGAN's latent space: the multi-scale reconstruction loss, the moments of W, the latent update.

Drives csrc/project.hip; composed in gan_lab_amd/project.py.  Re-exported by ``gan_lab_amd.ops``."""
import ctypes

import numpy as np

import torch
from torch.autograd import Function

from .. import _lib
from .._lib import check
from .core import _aligned16, _c, _inplace, _new, _p, _st
from .cr import _first_order


# ---------------------------------------------------------------------------------------------- #
# projection into StyleGAN's latent space (csrc/project.hip; project.py): the multi-scale reconstruction loss, the moments of W,
# the latent update
# ---------------------------------------------------------------------------------------------- #
PYRAMID_MAX_LEVELS = _lib.DEFINES['GANLAB_PYRAMID_MAX_LEVELS']
PROJECT_SCHEDULE = {'lr0': 0.1, 'initial_noise_factor': 0.05, 'lr_rampdown_length': 0.25, 'lr_rampup_length': 0.05,
                    'noise_ramp_length': 0.75}       # the StyleGAN2 projector's defaults


def pyramid_max_levels(res):
    """Levels ``pyramid_mse`` allows at resolution ``res``: min(6, log2(res) + 1); ValueError unless ``res`` is a power of two in
    [4, 1024]."""
    if isinstance(res, bool) or not isinstance(res, (int, np.integer)) or not 4 <= res <= 1024 or res & (res - 1):
        raise ValueError(f'pyramid_mse: the resolution must be a power of two in [4, 1024] (got {res!r})')
    return min(PYRAMID_MAX_LEVELS, int(res).bit_length())


def check_pyramid_weights(weights, res, what='weights'):
    """``weights`` of ``pyramid_mse`` at resolution ``res`` as a tuple of floats: 1 to ``pyramid_max_levels(res)`` finite
    non-negative numbers, else a ValueError that names ``what``."""
    top = pyramid_max_levels(res)
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError(f'{what} must be a sequence of non-negative numbers (got {weights!r})') from None
    if not 1 <= len(w) <= top:
        raise ValueError(f'{what} must hold 1 to {top} values at {res}x{res}, one per pyramid level (got {len(w)})')
    if any(isinstance(v, bool) for v in weights) or not all(0.0 <= v <= 3.0e38 for v in w):
        raise ValueError(f'{what} must be finite and non-negative (got {weights!r})')
    return w


class _PyramidMse(Function):
    """(loss (N,), terms (N, Lv)) of x against t; the gradient in x is formed by the forward's launch and saved.  First order only,
    no gradient for t."""

    @staticmethod
    def forward(ctx, x, t, weights):
        L = _lib.lib()
        n, c, r, _ = x.shape
        lv = len(weights)
        ws = torch.empty((L.ganlab_pyramid_mse_workspace(n, c, r, lv) + 7) // 8, dtype=torch.float64, device=x.device)
        g, loss, terms = torch.empty_like(x), _new((n,), x), _new((n, lv), x)
        host_w = (ctypes.c_float * lv)(*weights)
        check(L.ganlab_pyramid_mse_f32(_p(x), _p(t), ctypes.cast(host_w, ctypes.c_void_p), lv, _p(g), _p(loss), _p(terms), n, c, r,
                                       _p(ws), ws.numel() * 8, _st()), 'pyramid_mse')
        ctx.save_for_backward(x, g)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, gloss, _gterms):
        x, g = ctx.saved_tensors
        s = _c(gloss.detach(), 'pyramid_mse cotangent')
        gx = torch.empty_like(g)
        check(_lib.lib().ganlab_scale_rows_f32(_p(g), _p(s), _p(gx), g.shape[0], g[0].numel(), _st()), 'pyramid_mse_bwd')
        return _first_order('pyramid_mse', (x, gloss), (gx,))[0], None, None


def pyramid_mse(x, t, weights):
    """Multi-scale mean squared error of two (N, C, R, R) batches, R a power of two in [4, 1024]: with ``d_0 = x - t`` and
    ``d_{l+1}`` the 2x2 mean of ``d_l``, ``loss[n] = sum_l weights[l] * mean_{c,h,w} d_l[n]^2`` over ``len(weights)`` levels (at
    most ``pyramid_max_levels(R)``).  Returns ``(loss (N,), terms (N, Lv))``, ``terms[n, l]`` the unweighted level means
    (detached).  One launch reads x and t once, forms every level inside 32x32 tiles in LDS, sums the squares in fp64 and writes
    the gradient; a second adds the per-tile partials in a fixed order (csrc/project.hip; no atomics, bitwise reproducible).
    Differentiable ONCE in ``x`` (a second differentiation raises), not in ``t``."""
    x, t = _c(x, 'pyramid_mse x'), _c(t, 'pyramid_mse t')
    if x.dim() != 4 or x.shape[2] != x.shape[3] or x.shape != t.shape or x.device != t.device or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f'pyramid_mse: needs two equal (N, C, R, R) batches (got {tuple(x.shape)} on {x.device}, '
                         f'{tuple(t.shape)} on {t.device})')
    if t.requires_grad and torch.is_grad_enabled():
        raise RuntimeError('pyramid_mse has no gradient for its target: detach it')
    weights = check_pyramid_weights(weights, int(x.shape[2]), 'pyramid_mse: weights')
    return _PyramidMse.apply(_aligned16(x), _aligned16(t), weights)


def w_moments(ws):
    """``(w_avg (D,), w_std 0-dim)`` of (M, D) dlatent rows as the StyleGAN2 projector defines them: the column means and
    ``sqrt(sum (w - w_avg)^2 / M)`` over all entries; two passes, fp64, a fixed summation order; device tensors, no gradient."""
    ws = _c(ws, 'w_moments rows').detach()
    if ws.dim() != 2 or ws.shape[0] < 1 or ws.shape[1] < 1:
        raise ValueError(f'w_moments: needs (M, D) rows with M, D >= 1 (got {tuple(ws.shape)})')
    L = _lib.lib()
    m, d = ws.shape
    work = torch.empty((L.ganlab_w_moments_workspace(d) + 7) // 8, dtype=torch.float64, device=ws.device)
    w_avg, w_std = _new((d,), ws), _new((), ws)
    check(L.ganlab_w_moments_f32(_p(ws), _p(w_avg), _p(w_std), m, d, _p(work), work.numel() * 8, _st()), 'w_moments')
    return w_avg, w_std


def check_project_schedule(num_steps, schedule, what='project_step'):
    """The six doubles ``project_step`` takes - (lr0, initial_noise_factor, lr_rampdown_length, lr_rampup_length,
    noise_ramp_length, num_steps) - from ``num_steps`` and a dict over ``PROJECT_SCHEDULE``'s keys (missing: the default).
    ValueError naming the key: an unknown one, lr0 or initial_noise_factor not finite and >= 0, a length outside (0, 1]."""
    unknown = sorted(set(schedule) - set(PROJECT_SCHEDULE))
    if unknown:
        raise ValueError(f'{what}: unknown schedule value {unknown[0]!r} (known: {", ".join(PROJECT_SCHEDULE)})')
    if isinstance(num_steps, bool) or not isinstance(num_steps, (int, np.integer)) or not 1 <= num_steps < 2 ** 31:
        raise ValueError(f'{what}: steps must be an integer >= 1 (got {num_steps!r})')
    out = []
    for key, default in PROJECT_SCHEDULE.items():
        raw = schedule.get(key, default)
        try:
            val = float(raw)
        except (TypeError, ValueError):
            val = float('nan')
        lo_ok = val >= 0.0 if key in ('lr0', 'initial_noise_factor') else 0.0 < val <= 1.0
        if isinstance(raw, bool) or not (lo_ok and val < float('inf')):
            rng_txt = 'finite and >= 0' if key in ('lr0', 'initial_noise_factor') else 'in (0, 1]'
            raise ValueError(f'{what}: {key} must be {rng_txt} (got {raw!r})')
        out.append(val)
    return tuple(out) + (float(num_steps),)


def project_step(w_opt, grad_ws, m, v, step, noise, w_std, w_in, hyper):
    """One update of the projected dlatents in ONE launch (csrc/project.hip).  ``step``: 1-element int32 device tensor, the
    iteration count k.  W+ space: ``w_opt``, ``m``, ``v``, ``noise`` are (N, L, D) like ``grad_ws`` and ``w_in``; W space: they
    are (N, D), the gradient is ``grad_ws`` summed over L in layer order and ``w_in`` is broadcast over L.  Adam's update k + 1
    (betas 0.9 / 0.999, eps 1e-8, bias-corrected) with the learning rate of the StyleGAN2 projector's schedule at
    ``t = k / num_steps``, then ``step = k + 1`` and ``w_in = w_opt + scale((k + 1) / num_steps) * noise`` - the next forward's
    input.  ``grad_ws=None``: no update, ``w_in`` at the current count (the first forward's input).  ``hyper``:
    ``check_project_schedule``'s tuple.  Everything is updated in place; nothing is read back by the host."""
    w_in = _inplace(w_in, 'project_step w_in')
    if w_in.dim() != 3:
        raise ValueError(f'project_step: w_in must be (N, L, D) (got {tuple(w_in.shape)})')
    n, l, d = w_in.shape
    if w_opt.dim() not in (2, 3) or tuple(w_opt.shape) not in ((n, d), (n, l, d)):
        raise ValueError(f'project_step: w_opt must be ({n}, {d}) (W) or ({n}, {l}, {d}) (W+) (got {tuple(w_opt.shape)})')
    w_plus = w_opt.dim() == 3
    for name, t in (('w_opt', w_opt), ('m', m), ('v', v), ('noise', noise)):
        _inplace(t, f'project_step {name}')
        if t.shape != w_opt.shape:
            raise ValueError(f'project_step: {name} must have the shape of w_opt, {tuple(w_opt.shape)} (got {tuple(t.shape)})')
    if grad_ws is not None:
        grad_ws = _c(grad_ws, 'project_step grad_ws')
        if grad_ws.shape != w_in.shape:
            raise ValueError(f'project_step: grad_ws must be {tuple(w_in.shape)} (got {tuple(grad_ws.shape)})')
    if not isinstance(step, torch.Tensor) or not step.is_cuda or step.dtype != torch.int32 or step.numel() != 1:
        raise TypeError('gan_lab_amd.ops: project_step step must be a 1-element int32 tensor on the GPU; the HIP path has no CPU '
                        'fallback')
    w_std = _c(w_std, 'project_step w_std')
    if w_std.numel() != 1 or len(hyper) != 6:
        raise ValueError('project_step: w_std must hold one value and hyper six (check_project_schedule)')
    host_h = (ctypes.c_double * 6)(*[float(h) for h in hyper])
    check(_lib.lib().ganlab_project_step_f32(_p(w_opt), _p(grad_ws), _p(m), _p(v), ctypes.c_void_p(step.data_ptr()), _p(noise),
                                             _p(w_std), _p(w_in), n, l, int(w_plus), d, ctypes.cast(host_h, ctypes.c_void_p),
                                             _st()), 'project_step')
    return w_in
