"""The minibatch-stddev statistic with its explicit second order, and the scalar reductions / losses.

Re-exported by ``gan_lab_amd.ops``."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import check
from .core import _c, _nchw, _new, _p, _st
from .pointwise import k_scale_dev, k_sum, mul


# ---------------------------------------------------------------------------------------------- #
# minibatch stddev statistic with explicit second order (discriminator, R1 path)
# ---------------------------------------------------------------------------------------------- #
class _MbstdStat(Function):
    @staticmethod
    def forward(ctx, x, gs, eps):
        x = _c(x)
        b = x.shape[0]
        G, F = b // gs, x.numel() // b
        stat = _new((G,), x)
        check(_lib.lib().ganlab_mbstd_fwd_f32(_p(x), _p(stat), G, gs, F, eps, _st()), 'mbstd_fwd')
        ctx.save_for_backward(x)
        ctx.gs, ctx.eps = gs, eps
        return stat

    @staticmethod
    def backward(ctx, gstat):
        x, = ctx.saved_tensors
        return _MbstdBwd.apply(x, gstat, ctx.gs, ctx.eps), None, None


class _MbstdBwd(Function):
    @staticmethod
    def forward(ctx, x, gstat, gs, eps):
        x, gstat = _c(x), _c(gstat)
        b = x.shape[0]
        G, F = b // gs, x.numel() // b
        gx = torch.empty_like(x)
        check(_lib.lib().ganlab_mbstd_bwd_f32(_p(x), _p(gstat), _p(gx), G, gs, F, eps, _st()), 'mbstd_bwd')
        ctx.save_for_backward(x, gstat)
        ctx.gs, ctx.eps = gs, eps
        return gx

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        x, gstat = ctx.saved_tensors
        ggx = _c(ggx)
        b = x.shape[0]
        G, F = b // ctx.gs, x.numel() // b
        g_gstat, g_x = _new((G,), x), torch.empty_like(x)
        check(_lib.lib().ganlab_mbstd_bwdbwd_f32(_p(x), _p(gstat), _p(ggx), _p(g_gstat), _p(g_x), G, ctx.gs, F,
                                                 ctx.eps, _st()), 'mbstd_bwdbwd')
        return g_x, g_gstat, None, None


# ---------------------------------------------------------------------------------------------- #
# scalar reductions / losses (first-order)
# ---------------------------------------------------------------------------------------------- #
class _Sum(Function):
    """scale * sum(x) or scale * sum(x^2) -> 0-dim tensor; the cotangent never leaves the device."""

    @staticmethod
    def forward(ctx, x, scale, squared):
        ctx.save_for_backward(x if squared else None)
        ctx.scale, ctx.squared, ctx.shape = scale, squared, x.shape
        return k_sum(x, scale, squared)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        if ctx.squared:
            return k_scale_dev(x, gout.reshape(1), 2.0 * ctx.scale), None, None
        return k_scale_dev(None, gout.reshape(1), ctx.scale, ctx.shape), None, None


class _BceMean(Function):
    @staticmethod
    def forward(ctx, x, target):
        x = _c(x)
        out = _new((), x)
        check(_lib.lib().ganlab_bce_logits_fwd_f32(_p(x), _p(out), x.numel(), target, _st()), 'bce_fwd')
        ctx.save_for_backward(x)
        ctx.target = target
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        g1 = _c(gout).reshape(1)
        check(_lib.lib().ganlab_bce_logits_bwd_f32(_p(x), _p(g1), _p(gx), x.numel(), ctx.target, _st()), 'bce_bwd')
        return gx, None


class _HingeMean(Function):
    """mean(max(a + b*x, 0)) -> 0-dim tensor (the hinge loss terms: backprop_utils.hinge_loss_disc)."""

    @staticmethod
    def forward(ctx, x, a, b):
        x = _c(x)
        out = _new((), x)
        check(_lib.lib().ganlab_hinge_fwd_f32(_p(x), _p(out), x.numel(), a, b, _st()), 'hinge_fwd')
        ctx.save_for_backward(x)
        ctx.a, ctx.b = a, b
        return out

    @staticmethod
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        return _HingeBwd.apply(x, gout, ctx.a, ctx.b), None, None


class _HingeBwd(Function):
    """gx = gout * [a + b*x > 0] * b / n: piecewise constant in x (its derivative towards x is zero), linear in gout."""

    @staticmethod
    def forward(ctx, x, gout, a, b):
        gx = torch.empty_like(x)
        g1 = _c(gout).reshape(1)
        check(_lib.lib().ganlab_hinge_bwd_f32(_p(x), _p(g1), _p(gx), x.numel(), a, b, _st()), 'hinge_bwd')
        ctx.save_for_backward(x)
        ctx.a, ctx.b = a, b
        return gx

    @staticmethod
    def backward(ctx, gg):
        x, = ctx.saved_tensors
        ggout = None
        if ctx.needs_input_grad[1]:
            one = torch.ones(1, dtype=torch.float32, device=x.device)
            ggout = sum_all(mul(_c(gg), _HingeBwd.apply(x, one, ctx.a, ctx.b)))
        return torch.zeros_like(x), ggout, None, None


class _ChNormPenalty(Function):
    """scale * sum_{n,hw} (||g[n,:,hw]||_2 - gamma)^2  (WGAN-GP, resnetgan/learner.py:817-823)."""

    @staticmethod
    def forward(ctx, g, gamma, scale):
        g = _c(g)
        n, c, hw = _nchw(g)
        L = _lib.lib()
        ws = torch.empty((L.ganlab_sum_workspace(n * hw) + 3) // 4, dtype=torch.float32, device=g.device)
        out = _new((), g)
        check(L.ganlab_chnorm_penalty_fwd_f32(_p(g), _p(out), n, c, hw, gamma, scale, _p(ws), ws.numel() * 4, _st()),
              'chnorm_penalty_fwd')
        ctx.save_for_backward(g)
        ctx.gamma, ctx.scale = gamma, scale
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        g, = ctx.saved_tensors
        n, c, hw = _nchw(g)
        gg = torch.empty_like(g)
        g1 = _c(gout).reshape(1)
        check(_lib.lib().ganlab_chnorm_penalty_bwd_f32(_p(g), _p(g1), _p(gg), n, c, hw, ctx.gamma, ctx.scale, _st()),
              'chnorm_penalty_bwd')
        return gg, None, None


def mbstd_stat(x, group_size, eps=1e-8):
    return _MbstdStat.apply(x, int(group_size), float(eps))


def sum_all(x, scale=1.0):
    return _Sum.apply(x, float(scale), False)


def sumsq_all(x, scale=1.0):
    return _Sum.apply(x, float(scale), True)


def bce_logits_mean(x, target):
    return _BceMean.apply(x, float(target))


def hinge_mean(x, a, b):
    """mean(relu(a + b*x)) with its first derivative; the double backward towards ``x`` is zero."""
    return _HingeMean.apply(x, float(a), float(b))


def chnorm_penalty(g, gamma, scale):
    return _ChNormPenalty.apply(g, float(gamma), float(scale))
