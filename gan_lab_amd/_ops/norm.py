"""BatchNorm (training mode) and LayerNorm on fused kernels, and the same operators composed from the per-channel ops (the
cross-check of the fused kernels in the tests).

Drives csrc/norm.hip.  ``batch_norm`` itself stays in ``gan_lab_amd/ops.py`` (its eval path reads ``bias_act``).  Re-exported by
``gan_lab_amd.ops``."""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import ACT_LRELU, ACT_NONE, check
from .core import _c, _nchw, _new, _p, _row_workspace, _st, _want_param_grads
from .pointwise import chan_affine, channel_sum, k_act_bwd, mul


class _BatchNormTrain(Function):
    """nn.BatchNorm2d in training mode on fused kernels (csrc/norm.hip): batch statistics (2 launches), the C-element
    bookkeeping - rstd, scale, running estimates, batch counter - in one (``bn_finalize``), normalise + affine (1);
    backward sums = the parameter gradients (2) and the input gradient (1).  First order only - the generator is never
    inside a gradient penalty.  Returns (y, batch mean, biased batch variance)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, running_mean, running_var, momentum, batches, act_slope):
        x = _c(x)
        n, c, hw = _nchw(x)
        m = n * hw
        L = _lib.lib()
        ws = _row_workspace(c, m, x.device)
        mom = _new((c, 3), x)
        check(L.ganlab_bn_stats_f32(_p(x), _p(mom), n, c, hw, ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _st()),
              'bn_stats')
        fin = _new((4, c), x)                                # mean, var, rstd, scale = rstd * weight
        for buf in (running_mean, running_var, batches):
            assert buf is None or (buf.is_contiguous() and buf.device == x.device)
        assert batches is None or batches.dtype == torch.int64
        check(L.ganlab_bn_finalize_f32(_p(mom), _p(_c(weight)) if weight is not None else None,
                                       _p(running_mean) if running_mean is not None else None,
                                       _p(running_var) if running_var is not None else None,
                                       ctypes.c_void_p(batches.data_ptr()) if batches is not None else None, _p(fin), c,
                                       float(eps), float(momentum), m / max(m - 1, 1), _st()), 'bn_finalize')
        mean, var, rstd, scale = fin[0], fin[1], fin[2], fin[3]
        y = torch.empty_like(x)
        # act_slope: the LeakyReLU / ReLU behind the normalisation (resnetgan/resblocks.py:48-49) applied by the same pass;
        # its backward is applied by bn_bwd_sums as it loads the gradient (sign(y) = sign of the pre-activation)
        check(L.ganlab_bn_apply_f32(_p(x), _p(mean), _p(scale), _p(_c(bias)) if bias is not None else None, _p(y), n, c,
                                    hw, ACT_LRELU if act_slope is not None else ACT_NONE,
                                    float(act_slope) if act_slope is not None else 1.0, _st()), 'bn_apply')
        ctx.save_for_backward(x, mean, rstd, scale, y if act_slope is not None else None)
        ctx.act_slope = act_slope
        ctx.has_weight, ctx.has_bias = weight is not None, bias is not None
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gm, _gv):
        x, mean, rstd, scale, yact = ctx.saved_tensors
        gy = _c(gy)
        n, c, hw = _nchw(x)
        L = _lib.lib()
        ws = _row_workspace(c, n * hw, x.device)
        sums = _new((c, 3), x)
        gz = torch.empty_like(gy) if yact is not None else None      # gy * lrelu'(y), written by the sums pass
        check(L.ganlab_bn_bwd_sums_f32(_p(gy), _p(x), _p(mean), _p(rstd), _p(sums), n, c, hw,
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _p(yact), _p(gz),
                                       float(ctx.act_slope) if yact is not None else 1.0, _st()), 'bn_bwd_sums')
        if gz is not None:
            gy = gz
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            check(L.ganlab_bn_bwd_apply_f32(_p(gy), _p(x), _p(mean), _p(rstd), _p(sums), _p(scale), _p(gx), n, c, hw,
                                            _st()), 'bn_bwd_apply')
        want_p = _want_param_grads()
        gw = sums[:, 1] if (ctx.has_weight and want_p and ctx.needs_input_grad[1]) else None
        gb = sums[:, 0] if (ctx.has_bias and want_p and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None, None, None, None, None, None


def batch_norm_composed(x, weight, bias, eps=1e-5):
    """Training-mode BatchNorm composed from channel sums / per-channel affines / products (any order of
    differentiation through autograd): the cross-check of the fused kernels in the tests."""
    n, c, hw = _nchw(x)
    m = n * hw
    mean = channel_sum(x) / m
    xc = chan_affine(x, None, -mean)
    var = channel_sum(mul(xc, xc)) / m
    rstd = torch.rsqrt(var + eps)
    return chan_affine(xc, rstd * weight if weight is not None else rstd, bias)


def _ln_rowsums(a, wa, x, mean, rstd, n, m, b2=None, w2=None, yact=None, gz=None, slope=1.0):
    """[N][3] row sums (see ganlab_ln_rowsums_f32): sum a*wa, sum a*wa*xhat, sum a*b2*w2; with ``yact`` a is first multiplied
    by lrelu'(yact) and that product is also written to ``gz``."""
    L = _lib.lib()
    nbytes = L.ganlab_ln_rowsums_workspace(n, m)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    out = _new((n, 3), x)
    check(L.ganlab_ln_rowsums_f32(_p(a), _p(wa), _p(x), _p(mean), _p(rstd), _p(b2), _p(w2), _p(out), n, m,
                                  ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _p(yact), _p(gz), float(slope), _st()),
          'ln_rowsums')
    return out


def _ln_project(a, wa, x, mean, rstd, sums, wo, n, m):
    """wo * P_x(a * wa) with P_x(g) = rstd * (g - mean(g) - xhat * mean(g * xhat)) per row."""
    out = torch.empty_like(x)
    check(_lib.lib().ganlab_ln_project_f32(_p(a), _p(wa), _p(x), _p(mean), _p(rstd), _p(sums), _p(wo), _p(out), n, m,
                                           _st()), 'ln_project')
    return out


class _LayerNorm(Function):
    """nn.LayerNorm(x.shape[1:]) with elementwise affine on fused kernels (csrc/norm.hip): 2 launches forward,
    4 backward, 7 for the backward of the backward (WGAN-GP through the critic)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, act_slope):
        x = _c(x)
        n = x.shape[0]
        m = x.numel() // n
        w = _c(weight).reshape(m) if weight is not None else None
        b = _c(bias).reshape(m) if bias is not None else None
        L = _lib.lib()
        mean, rstd = _new((n,), x), _new((n,), x)
        nbytes = L.ganlab_row_stats_workspace(n, m)
        ws = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.float64, device=x.device)
        check(L.ganlab_row_stats_f32(_p(x), _p(mean), _p(rstd), n, m, eps, _p(ws), ws.numel() * 8, _st()), 'ln_stats')
        y = torch.empty_like(x)
        # act_slope: the LeakyReLU / ReLU behind the normalisation (resnetgan/resblocks.py:48-49) in the same pass; the
        # backward applies its derivative while loading the gradient for the row sums (sign(y) = sign of the pre-activation)
        check(L.ganlab_ln_affine_fwd_f32(_p(x), _p(mean), _p(rstd), _p(w), _p(b), _p(y), n, m,
                                         ACT_LRELU if act_slope is not None else ACT_NONE,
                                         float(act_slope) if act_slope is not None else 1.0, _st()), 'ln_affine_fwd')
        # the weight INPUT is saved: the double backward reaches the parameter
        ctx.save_for_backward(x, weight, mean, rstd, y if act_slope is not None else None)
        ctx.act_slope = act_slope
        ctx.wshape = weight.shape if weight is not None else None
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, rstd, yact = ctx.saved_tensors
        w = weight.reshape(-1) if weight is not None else None      # tracked under create_graph
        want_p = _want_param_grads() and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        gx, gw, gb = _LayerNormBwd.apply(gy, x, w, mean, rstd, want_p, yact, ctx.act_slope)
        if gw is not None and ctx.wshape is not None:
            gw = gw.reshape(ctx.wshape)
            gb = gb.reshape(ctx.wshape) if ctx.has_bias else None
        else:
            gw = gb = None
        return gx, gw, gb if ctx.has_bias else None, None, None


class _LayerNormBwd(Function):
    """(gy, x, w) -> (gx, gw, gb); its own backward is the analytic double backward for a cotangent of gx (the
    gradient-penalty pass never keeps gw / gb: ops.input_grad_only).  With ``yact`` (the output of a LayerNorm fused with
    its LeakyReLU) gy is the gradient BEHIND the activation: gz = gy * lrelu'(yact) is formed by the row-sums pass and takes
    gy's place everywhere below; lrelu'' = 0, so the double backward only gains the same mask on its d/d gy."""

    @staticmethod
    def forward(ctx, gy, x, w, mean, rstd, want_param_grads, yact=None, act_slope=None):
        gy = _c(gy)
        w = _c(w) if w is not None else None
        n = x.shape[0]
        m = x.numel() // n
        L = _lib.lib()
        if yact is not None:
            gz = torch.empty_like(gy)
            sums = _ln_rowsums(gy, w, x, mean, rstd, n, m, yact=yact, gz=gz, slope=act_slope)
            gy = gz
        else:
            sums = _ln_rowsums(gy, w, x, mean, rstd, n, m)             # a = mean(ghat), beta = mean(ghat * xhat)
        gw = gb = None
        if want_param_grads and w is not None:       # projection and parameter gradients in one pass over (gy, x)
            gx, gw, gb = torch.empty_like(x), _new((m,), x), _new((m,), x)
            check(L.ganlab_ln_bwd_cols_f32(_p(gy), _p(w), _p(x), _p(mean), _p(rstd), _p(sums), _p(gx), _p(gw), _p(gb), n, m,
                                           _st()), 'ln_bwd_cols')
        else:
            gx = _ln_project(gy, w, x, mean, rstd, sums, None, n, m)   # P_x(gy * w)
        ctx.save_for_backward(gy, x, w, mean, rstd, gx, sums, yact)
        ctx.act_slope = act_slope
        ctx.set_materialize_grads(False)
        return gx, gw, gb

    @staticmethod
    @once_differentiable
    def backward(ctx, u, ggw, ggb):
        gy, x, w, mean, rstd, gx, sums, yact = ctx.saved_tensors
        if ggw is not None or ggb is not None:
            raise NotImplementedError('LayerNorm double backward through the parameter gradients is not needed by the '
                                      'GAN losses (the penalty differentiates the INPUT gradient only)')
        if u is None:
            return None, None, None, None, None, None, None, None
        u = _c(u)
        n = x.shape[0]
        m = x.numel() // n
        L = _lib.lib()
        usums = _ln_rowsums(u, None, x, mean, rstd, n, m, b2=gy, w2=w)   # sum u, sum u*xhat, sum u*ghat
        pu = _ln_project(u, None, x, mean, rstd, usums, None, n, m)      # P_x(u)
        g_w = None
        if w is not None:
            g_gy = torch.empty_like(gy)
            check(L.ganlab_colscale_f32(_p(pu), _p(w), _p(g_gy), n, m, _st()), 'ln_colscale')
            if _want_param_grads() and ctx.needs_input_grad[2]:
                g_w = _new((m,), x)
                check(L.ganlab_coldot_f32(_p(gy), _p(pu), None, None, _p(g_w), None, n, m, _st()), 'ln_coldot')
        else:
            g_gy = pu
        g_x = torch.empty_like(x)       # the per-row coefficients come from (sums, usums) inside the kernel
        check(L.ganlab_ln_bwdbwd_apply_f32(_p(x), _p(mean), _p(rstd), _p(pu), _p(gx), _p(sums), _p(usums), _p(g_x),
                                           n, m, _st()), 'ln_bwdbwd_apply')
        if yact is not None:
            g_gy = k_act_bwd(g_gy, yact, ctx.act_slope)
        return g_gy, g_x, g_w, None, None, None, None, None


def layer_norm(x, weight, bias, eps=1e-5, act_slope=None):
    """nn.LayerNorm(normalized_shape = x.shape[1:]) semantics: per-sample statistics over all features (biased
    variance), then the elementwise affine - fused kernels with an analytic double backward (csrc/norm.hip).
    ``act_slope``: LeakyReLU(act_slope) (0 = ReLU) of the result in the same passes, forward and backward."""
    return _LayerNorm.apply(x, weight, bias, float(eps), None if act_slope is None else float(act_slope))


def layer_norm_composed(x, weight, bias, eps=1e-5):
    """The same operator composed from channel sums / per-channel affines / products (every piece closed under
    differentiation, so autograd derives any order): the cross-check of the fused kernels in the tests."""
    shape = x.shape
    n = shape[0]
    f = x.numel() // n
    xr = x.reshape(1, n, f)
    mean = channel_sum(xr) / f
    xc = chan_affine(xr, None, -mean)
    var = channel_sum(mul(xc, xc)) / f
    y = chan_affine(xc, torch.rsqrt(var + eps), None)
    if weight is not None:
        y = chan_affine(y.reshape(n, f, 1), weight.reshape(f), bias.reshape(f) if bias is not None else None)
    return y.reshape(shape)
