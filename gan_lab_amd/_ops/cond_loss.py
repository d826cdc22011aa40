"""Classifier-based class conditioning: AC-GAN's cross-entropy, ContraGAN's 2C and ReACGAN's D2D-CE losses.

Drives csrc/cond_loss.hip; composed in gan_lab_amd/conditional.py.  Re-exported by ``gan_lab_amd.ops``."""
import numpy as np

import torch
from torch.autograd import Function

from .. import _lib
from .._lib import check
from .core import _c, _new, _p, _st, _want_param_grads
from .cond import _labels
from .cr import _first_order


# ---------------------------------------------------------------------------------------------- #
# classifier-based class conditioning (csrc/cond_loss.hip; conditional.py): AC-GAN's cross-entropy, ContraGAN's 2C, ReACGAN's D2D-CE
# ---------------------------------------------------------------------------------------------- #
CL_MODES = {'2c': 0, 'd2d': 1}
CL_MAX_N, CL_MAX_E, CL_MAX_K = 8192, 1024, 65536


def _cl_range(what, n, k, e=None):
    if not 1 <= n <= CL_MAX_N or not 2 <= k <= CL_MAX_K or (e is not None and not 1 <= e <= CL_MAX_E):
        raise ValueError(f'{what}: supported are 1 <= N <= {CL_MAX_N}, 2 <= K <= {CL_MAX_K}' +
                         (f', 1 <= E <= {CL_MAX_E} (got N = {n}, E = {e}, K = {k})' if e is not None else f' (got N = {n}, K = {k})'))


class _ClassCrossEntropy(Function):
    """mean_i (LSE_k z_ik - z[i, y_i]) -> 0-dim tensor; first order only."""

    @staticmethod
    def forward(ctx, z, labels):
        n, k = z.shape
        out, lse = _new((), z), _new((n,), z)
        check(_lib.lib().ganlab_class_ce_fwd_f32(_p(z), _p(labels), _p(out), _p(lse), n, k, _st()), 'class_ce_fwd')
        ctx.save_for_backward(z, labels, lse)
        return out

    @staticmethod
    def backward(ctx, gout):
        z, labels, lse = ctx.saved_tensors
        n, k = z.shape
        dz = torch.empty_like(z)
        g1 = _c(gout.detach()).reshape(1)
        check(_lib.lib().ganlab_class_ce_bwd_f32(_p(z), _p(labels), _p(lse), _p(g1), _p(dz), n, k, _st()), 'class_ce_bwd')
        return _first_order('class_cross_entropy', (z, gout), (dz,))[0], None


class _ClassContrastive(Function):
    """The 2C / D2D-CE mean over rows -> (0-dim loss, (4, N) rows = l, D, M, s); first order only."""

    @staticmethod
    def forward(ctx, h, proxy, labels, mode, tau, mp, mn):
        n, e = h.shape
        k = proxy.shape[0]
        out, rows = _new((), h), _new((4, n), h)
        check(_lib.lib().ganlab_cl_fwd_f32(_p(h), _p(proxy), _p(labels), _p(out), _p(rows), n, e, k, mode, tau, mp, mn, _st()),
              'cl_fwd')
        ctx.save_for_backward(h, proxy, labels, rows)
        ctx.params = (mode, tau, mp, mn)
        ctx.mark_non_differentiable(rows)
        return out, rows

    @staticmethod
    def backward(ctx, gout, _grows):
        h, proxy, labels, rows = ctx.saved_tensors
        n, e = h.shape
        k = proxy.shape[0]
        L = _lib.lib()
        dh, dp = torch.empty_like(h), torch.empty_like(proxy)
        ws = _new(((L.ganlab_cl_bwd_workspace(n, e, k) + 3) // 4,), h)
        g1 = _c(gout.detach()).reshape(1)
        check(L.ganlab_cl_bwd_f32(_p(h), _p(proxy), _p(labels), _p(rows), _p(g1), _p(dh), _p(dp), n, e, k, *ctx.params, _p(ws),
                                  ws.numel() * 4, _st()), 'cl_bwd')
        dh, dp = _first_order('class_contrastive', (h, proxy, gout), (dh, dp))
        return dh, dp if _want_param_grads() else None, None, None, None, None, None


def class_cross_entropy(logits, labels):
    """AC-GAN's auxiliary classification loss (Odena et al. 2017): the mean over the N rows of ``logsumexp(logits[i]) -
    logits[i, labels[i]]`` for (N, K) logits, as a 0-dim device tensor; one launch forward, one backward, a fixed summation order
    (bitwise reproducible).  Differentiable ONCE; a second differentiation raises."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError('class_cross_entropy: logits must be an (N, K) tensor')
    z = _c(logits, 'class_cross_entropy logits')
    _cl_range('class_cross_entropy', z.shape[0], z.shape[1])
    return _ClassCrossEntropy.apply(z, _labels(labels, z.shape[0], 'class_cross_entropy'))


def class_contrastive(h, proxy_weight, labels, mode='2c', temperature=1.0, margin_pos=0.98, margin_neg=0.02, return_rows=False):
    """ContraGAN's conditional contrastive loss (``mode='2c'``; Kang & Park 2020) or ReACGAN's data-to-data cross-entropy
    (``mode='d2d'``; Kang et al. 2021) of (N, E) embeddings ``h`` and the (K, E) class proxies ``proxy_weight``, both normalised
    to unit rows inside: the mean over rows as a 0-dim device tensor (csrc/cond_loss.hip: the N x N similarities are formed tile
    by tile on the exact-fp32 MFMA and never stored; 2 launches forward, 3 backward, bitwise reproducible).  The margins are
    D2D-CE's.  ``return_rows``: also the (N,) per-row losses (detached).  Differentiable ONCE in ``h`` and ``proxy_weight``."""
    if not isinstance(h, torch.Tensor) or h.dim() != 2 or not isinstance(proxy_weight, torch.Tensor) or proxy_weight.dim() != 2 \
            or h.shape[1] != proxy_weight.shape[1]:
        raise ValueError(f'class_contrastive: embeddings (N, E) and proxies (K, E) do not fit (got '
                         f'{tuple(getattr(h, "shape", ()))}, {tuple(getattr(proxy_weight, "shape", ()))})')
    if mode not in CL_MODES:
        raise ValueError(f"class_contrastive: mode must be '2c' or 'd2d' (got {mode!r})")
    tau, mp, mn = float(temperature), float(margin_pos), float(margin_neg)
    if not (tau > 0 and np.isfinite(tau) and np.isfinite(mp) and np.isfinite(mn)):
        raise ValueError(f'class_contrastive: needs a finite temperature > 0 and finite margins (got {tau}, {mp}, {mn})')
    h, proxy_weight = _c(h, 'class_contrastive embeddings'), _c(proxy_weight, 'class_contrastive proxies')
    _cl_range('class_contrastive', h.shape[0], proxy_weight.shape[0], h.shape[1])
    loss, rows = _ClassContrastive.apply(h, proxy_weight, _labels(labels, h.shape[0], 'class_contrastive'), CL_MODES[mode], tau,
                                         mp, mn)
    return (loss, rows[0]) if return_rows else loss
