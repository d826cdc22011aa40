"""Plain pointwise, resampling and per-channel ops: launchers, their Functions (each backward written with Functions of this
module, so any order of differentiation stays on HIP kernels) and the functional wrappers.

Drives the blur / up2 / pool2 / resample2d / bias_act / act_bwd / channel_sum / axpby / scale_dev / sum / u8 decode / pixelnorm /
chan_affine / mul / tanh kernels.  ``k_act_bwd_bias`` and ``k_channel_sum`` write parameter gradients and take their output
through ``core._take``.  Re-exported by ``gan_lab_amd.ops``."""
import numpy as np

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import check
from .core import _c, _nchw, _new, _p, _st, _take


# ---------------------------------------------------------------------------------------------- #
# kernel launchers
# ---------------------------------------------------------------------------------------------- #
def k_blur(x):
    x = _c(x)
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    check(_lib.lib().ganlab_blur3x3_f32(_p(x), _p(y), n * c, h, w, _st()), 'blur3x3')
    return y


def decode_u8(images_u8_nhwc, res, mean, std, flip=None):
    """Real-image input path on the device: (N,Hs,Ws,C) uint8 -> box-downsample by the
    power-of-two factor Hs/res (bit-exact with PIL's BOX resize) -> (N,C,res,res) fp32 ``(v/255 - mean)/std``
    (data_config.py:307-341).  ``flip``: optional (N,) uint8/bool mask, horizontal mirror per image."""
    x = images_u8_nhwc
    if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 4:
        raise TypeError('decode_u8 needs a (N,H,W,C) uint8 tensor on the GPU')
    x = x.contiguous()
    n, hs, ws, c = x.shape
    if hs % res or ws % res or hs // res != ws // res:
        raise ValueError(f'cannot box-resize {hs}x{ws} to {res}x{res}')
    mean = torch.as_tensor(mean, dtype=torch.float32, device=x.device).contiguous()
    std = torch.as_tensor(std, dtype=torch.float32, device=x.device).contiguous()
    assert mean.numel() == c and std.numel() == c
    if flip is not None:
        flip = flip.to(device=x.device, dtype=torch.uint8).contiguous()
        assert flip.numel() == n
    out = torch.empty((n, c, res, res), dtype=torch.float32, device=x.device)
    check(_lib.lib().ganlab_u8_box_decode_f32(x.data_ptr(), _p(out), n, hs, ws, c, hs // res, _p(mean), _p(std),
                                              flip.data_ptr() if flip is not None else None, _st()), 'u8_box_decode')
    return out


def k_up2(x, scale=1.0):
    x = _c(x)
    n, c, h, w = x.shape
    y = _new((n, c, 2 * h, 2 * w), x)
    check(_lib.lib().ganlab_up2_f32(_p(x), _p(y), n * c, h, w, scale, _st()), 'up2')
    return y


def k_pool2(x, scale=0.25):
    x = _c(x)
    n, c, h, w = x.shape
    assert h % 2 == 0 and w % 2 == 0
    y = _new((n, c, h // 2, w // 2), x)
    check(_lib.lib().ganlab_pool2_f32(_p(x), _p(y), n * c, h // 2, w // 2, scale, _st()), 'pool2')
    return y


# ---- table-driven resamplers: nn.Upsample(mode='bilinear'), NearestPool2d, BilinearPool2d (custom_layers.py:59-75) ---
RESAMPLE_MODES = ('bilinear_up', 'bilinear_down', 'nearest_down')


_RESAMPLE_TABLES = {}


def resample_matrix(mode, align_corners, n_in):
    """1-D interpolation matrix (n_out x n_in, float64 entries that are float32 numbers) of ``F.interpolate`` at scale
    2 / 0.5, with ATen's source-index arithmetic in float32: align_corners -> src = dst * (n_in-1)/(n_out-1); else
    src = (dst + .5) / scale - .5 clamped at 0 (bilinear), floor(dst / scale) (nearest)."""
    if mode not in RESAMPLE_MODES:
        raise ValueError(f'resampler mode {mode!r}: one of {RESAMPLE_MODES}')
    f32 = np.float32
    n_out = 2 * n_in if mode == 'bilinear_up' else n_in // 2
    if n_out < 1 or (mode != 'bilinear_up' and n_in % 2):
        raise ValueError(f'{mode}: size {n_in} has no 0.5x / 2x counterpart')
    m = np.zeros((n_out, n_in), np.float64)
    inv = f32(0.5) if mode == 'bilinear_up' else f32(2.0)
    for o in range(n_out):
        if mode == 'nearest_down':
            m[o, min(int(np.floor(f32(o) * inv)), n_in - 1)] = 1.0
            continue
        if align_corners:
            r = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
            src = r * f32(o)
        else:
            src = max(inv * (f32(o) + f32(0.5)) - f32(0.5), f32(0))
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = f32(src) - f32(i0)
        m[o, i0] += float(f32(1) - l1)
        m[o, i1] += float(l1)
    return m


def _taps(m):
    nz = [np.nonzero(row)[0] for row in m]
    t = max(1, max(len(v) for v in nz))
    if t > 6:
        raise ValueError(f'resampler needs {t} taps per output (the kernel holds 6)')
    idx, w = np.zeros((m.shape[0], t), np.int32), np.zeros((m.shape[0], t), np.float32)
    for o, v in enumerate(nz):
        idx[o, :len(v)] = v
        w[o, :len(v)] = m[o, v]
    return idx, w, t


def _resample_tables(mode, align, n_in, adjoint, device):
    key = (mode, bool(align), int(n_in), bool(adjoint), str(device))
    tab = _RESAMPLE_TABLES.get(key)
    if tab is None:
        m = resample_matrix(mode, align, n_in)
        idx, w, t = _taps(m.T if adjoint else m)
        tab = (torch.from_numpy(idx).to(device), torch.from_numpy(w).to(device), t, idx.shape[0])
        _RESAMPLE_TABLES[key] = tab
    return tab


def k_resample(x, mode, align, hin, win, adjoint):
    """``adjoint=False``: (N, C, hin, win) -> the resampled map; ``True``: a map of the resampled size -> (N, C, hin, win)
    through the transposed interpolation matrices (the layer's backward; its own backward is the forward again)."""
    x = _c(x)
    n, c, h, w = x.shape
    iy, wy, ty, ho = _resample_tables(mode, align, hin, adjoint, x.device)
    ix, wx, tx, wo = _resample_tables(mode, align, win, adjoint, x.device)
    exp_h = hin if not adjoint else (2 * hin if mode == 'bilinear_up' else hin // 2)
    exp_w = win if not adjoint else (2 * win if mode == 'bilinear_up' else win // 2)
    if (h, w) != (exp_h, exp_w):
        raise ValueError(f'resample {mode} (adjoint={adjoint}): input {h}x{w}, expected {exp_h}x{exp_w}')
    y = _new((n, c, ho, wo), x)
    check(_lib.lib().ganlab_resample2d_f32(_p(x), _p(y), _p(iy), _p(wy), _p(ix), _p(wx), n * c, h, w, ho, wo, ty, tx,
                                           _st()), 'resample2d')
    return y


def k_bias_act(x, bias, noise, noise_w, bias_scale, act, slope):
    x = _c(x)
    n, c, hw = _nchw(x)
    y = torch.empty_like(x)
    bias = _c(bias) if bias is not None else None
    noise = _c(noise) if noise is not None else None
    noise_w = _c(noise_w) if noise_w is not None else None
    if noise is not None:
        assert noise.numel() == n * hw and noise_w.numel() == c
    check(_lib.lib().ganlab_bias_act_f32(_p(x), _p(bias), _p(noise), _p(noise_w), _p(y), n, c, hw, bias_scale, act,
                                         slope, _st()), 'bias_act')
    return y


def k_act_bwd(gy, y, slope):
    gy, y = _c(gy), _c(y)
    assert gy.shape == y.shape
    gz = torch.empty_like(gy)
    check(_lib.lib().ganlab_act_bwd_f32(_p(gy), _p(y), _p(gz), gy.numel(), slope, _st()), 'act_bwd')
    return gz


def k_act_bwd_bias(gy, y, slope, scale):
    gy, y = _c(gy), _c(y)
    assert gy.shape == y.shape
    n, c, hw = _nchw(gy)
    L = _lib.lib()
    ws = torch.empty((L.ganlab_channel_sum_workspace(n, c, hw) + 3) // 4, dtype=torch.float32, device=gy.device)
    gz, gb = torch.empty_like(gy), _take('gb', (c,), gy)
    check(L.ganlab_act_bwd_bias_f32(_p(gy), _p(y), _p(gz), _p(gb), n, c, hw, slope, scale, _p(ws), ws.numel() * 4,
                                    _st()), 'act_bwd_bias')
    return gz, gb


def k_channel_sum(a, b=None, scale=1.0, sink=None):
    a = _c(a)
    n, c, hw = _nchw(a)
    L = _lib.lib()
    nbytes = L.ganlab_channel_sum_workspace(n, c, hw)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=a.device)
    out = _take(sink, (c,), a) if sink is not None else _new((c,), a)
    b = _c(b) if b is not None else None
    check(L.ganlab_channel_sum_f32(_p(a), _p(b), _p(out), n, c, hw, scale, _p(ws), ws.numel() * 4, _st()),
          'channel_sum')
    return out


def k_axpby(x, y, a, b, out=None):
    """a*x + b*y; ``out`` may be ``y`` itself (running averages updated in place: a captured step must write the buffer
    the next replay reads)."""
    x = _c(x)
    y = _c(y) if y is not None else None
    if y is not None:
        assert x.shape == y.shape
    if out is None:
        out = torch.empty_like(x)
    assert out.is_contiguous() and out.shape == x.shape
    check(_lib.lib().ganlab_axpby_f32(_p(x), _p(y), _p(out), x.numel(), a, b, _st()), 'axpby')
    return out


def k_scale_dev(x, gout, a, shape=None):
    gout = _c(gout)
    x = _c(x) if x is not None else None
    out = torch.empty_like(x) if x is not None else _new(shape, gout)
    check(_lib.lib().ganlab_scale_dev_f32(_p(x), _p(gout), _p(out), out.numel(), a, _st()), 'scale_dev')
    return out


def k_sum(x, scale=1.0, squared=False):
    x = _c(x)
    L = _lib.lib()
    ws = torch.empty((L.ganlab_sum_workspace(x.numel()) + 3) // 4, dtype=torch.float32, device=x.device)
    out = _new((), x)
    check(L.ganlab_sum_f32(_p(x), _p(out), x.numel(), scale, int(squared), _p(ws), ws.numel() * 4, _st()), 'sum')
    return out


# ---------------------------------------------------------------------------------------------- #
# Functions: each backward is written with Functions of this module
# ---------------------------------------------------------------------------------------------- #
class _ActBwd(Function):
    """gz = gy * lrelu'(y) from the saved OUTPUT y (sign(y) == sign(pre-activation))."""

    @staticmethod
    def forward(ctx, gy, y, slope):
        ctx.save_for_backward(y)
        ctx.slope = slope
        return k_act_bwd(gy, y, slope)

    @staticmethod
    def backward(ctx, gg):
        y, = ctx.saved_tensors
        return _ActBwd.apply(gg, y, ctx.slope), None, None


class _ActBwdBias(Function):
    """(gz, gb) = (gy * lrelu'(y), bias_scale * sum_{n,hw} gz) in one pass over the tensors."""

    @staticmethod
    def forward(ctx, gy, y, slope, bias_scale):
        ctx.save_for_backward(y)
        ctx.slope, ctx.bias_scale = slope, bias_scale
        gz, gb = k_act_bwd_bias(gy, y, slope, bias_scale)
        return gz, gb

    @staticmethod
    def backward(ctx, ggz, ggb):
        y, = ctx.saved_tensors
        g = ggz
        if ggb is not None:
            shape = y.shape
            view = [1, shape[1]] + [1] * (len(shape) - 2)
            b = _Scale.apply(ggb.view(view).expand(shape), ctx.bias_scale)
            g = b if g is None else _Axpby.apply(g, b, 1.0, 1.0)
        return (_ActBwd.apply(g, y, ctx.slope) if g is not None else None), None, None, None


class _ChanSum(Function):
    """(N,C,...) -> (C,) sum, optionally weighted by a (N,1,...) map (noise-weight gradient)."""

    @staticmethod
    def forward(ctx, a, b, scale, sink=None):
        ctx.shape, ctx.scale = a.shape, scale
        ctx.has_b = b is not None
        return k_channel_sum(a, b, scale, sink)

    @staticmethod
    def backward(ctx, g):
        if ctx.has_b:
            raise NotImplementedError('double backward through the noise-weighted channel sum')
        shape = ctx.shape
        view = [1, shape[1]] + [1] * (len(shape) - 2)
        return _Scale.apply(g.view(view).expand(shape), ctx.scale), None, None, None


class _GroupBroadcast(Function):
    """(G,) -> (G*gs, 1, h, w): every sample of group g gets stat[g] on its whole plane (the minibatch-stddev feature map,
    custom_layers.py:135-139).  Its adjoint is a per-group sum: a channel-sum launch instead of the ATen reduction that
    autograd derives for ``expand``; the pair is closed under differentiation (R1 differentiates through it)."""

    @staticmethod
    def forward(ctx, stat, gs, h, w):
        ctx.dims = (stat.shape[0], gs, h, w)
        G = stat.shape[0]
        return stat.view(G, 1, 1, 1, 1).expand(G, gs, 1, h, w).reshape(G * gs, 1, h, w)

    @staticmethod
    def backward(ctx, g):
        G, gs, h, w = ctx.dims
        return _ChanSum.apply(g.reshape(1, G, gs * h * w), None, 1.0), None, None, None


class _Blur(Function):
    @staticmethod
    def forward(ctx, x):
        return k_blur(x)

    @staticmethod
    def backward(ctx, g):
        return _Blur.apply(g)  # symmetric taps + zero padding -> self-adjoint


class _Pool2(Function):
    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return k_pool2(x, scale)

    @staticmethod
    def backward(ctx, g):
        return _Up2.apply(g, ctx.scale), None


class _Up2(Function):
    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return k_up2(x, scale)

    @staticmethod
    def backward(ctx, g):
        return _Pool2.apply(g, ctx.scale), None


class _Resample(Function):
    """Linear map x -> M_y x M_x^T; backward is the adjoint gather, whose backward is the forward (R1 reaches the critic's
    pooler through a double backward)."""

    @staticmethod
    def forward(ctx, x, mode, align, hin, win, adjoint):
        ctx.args = (mode, align, hin, win, adjoint)
        return k_resample(x, mode, align, hin, win, adjoint)

    @staticmethod
    def backward(ctx, g):
        mode, align, hin, win, adjoint = ctx.args
        return _Resample.apply(g, mode, align, hin, win, not adjoint), None, None, None, None, None


class _Scale(Function):
    @staticmethod
    def forward(ctx, x, a):
        ctx.a = a
        return k_axpby(x, None, a, 0.0)

    @staticmethod
    def backward(ctx, g):
        return _Scale.apply(g, ctx.a), None


class _Axpby(Function):
    """out = a*x + b*y (fade-in blends, progan/architectures.py:163-167, :311-315)."""

    @staticmethod
    def forward(ctx, x, y, a, b):
        ctx.a, ctx.b = a, b
        return k_axpby(x, y, a, b)

    @staticmethod
    def backward(ctx, g):
        gx = _Scale.apply(g, ctx.a) if ctx.needs_input_grad[0] else None
        gy = _Scale.apply(g, ctx.b) if ctx.needs_input_grad[1] else None
        return gx, gy, None, None


class _PixelNorm(Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = _c(x)
        n, c, hw = _nchw(x)
        y = torch.empty_like(x)
        check(_lib.lib().ganlab_pixelnorm_fwd_f32(_p(x), _p(y), n, c, hw, eps, _st()), 'pixelnorm_fwd')
        ctx.save_for_backward(x)
        ctx.eps = eps
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gy = _c(gy)
        n, c, hw = _nchw(x)
        gx = torch.empty_like(x)
        check(_lib.lib().ganlab_pixelnorm_bwd_f32(_p(gy), _p(x), _p(gx), n, c, hw, ctx.eps, _st()), 'pixelnorm_bwd')
        return gx, None


# ---------------------------------------------------------------------------------------------- #
# BatchNorm / LayerNorm building blocks (ResNet GAN path): every piece is closed under differentiation,
# so torch.autograd composes first and second derivatives (WGAN-GP through LayerNorm) from HIP kernels.
# ---------------------------------------------------------------------------------------------- #
class _ChanAffine(Function):
    """y[n,c,...] = x[n,c,...] * scale[c] + shift[c]  (scale / shift may be None)."""

    @staticmethod
    def forward(ctx, x, scale, shift):
        x = _c(x)
        n, c, hw = _nchw(x)
        sc = _c(scale) if scale is not None else None
        sh = _c(shift) if shift is not None else None
        y = torch.empty_like(x)
        check(_lib.lib().ganlab_chan_affine_f32(_p(x), _p(sc), _p(sh), _p(y), n, c, hw, _st()), 'chan_affine')
        ctx.save_for_backward(x, sc)
        ctx.has = (scale is not None, shift is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, sc = ctx.saved_tensors
        gx = _ChanAffine.apply(g, sc, None) if ctx.needs_input_grad[0] else None
        gs = _ChanSum.apply(_Mul.apply(g, x), None, 1.0) if (ctx.has[0] and ctx.needs_input_grad[1]) else None
        gt = _ChanSum.apply(g, None, 1.0) if (ctx.has[1] and ctx.needs_input_grad[2]) else None
        return gx, gs, gt


class _Mul(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        assert a.shape == b.shape
        out = torch.empty_like(a)
        check(_lib.lib().ganlab_mul_f32(_p(a), _p(b), _p(out), a.numel(), _st()), 'mul')
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return (_Mul.apply(g, b) if ctx.needs_input_grad[0] else None,
                _Mul.apply(g, a) if ctx.needs_input_grad[1] else None)


class _Tanh(Function):
    """nn.Tanh: the ResNet generators' output layer, and the hidden activation of ``--nonlinearity tanh``
    (config.py:208,254; resnetgan/learner.py:180-181).  The backward is a Function of its own so that a gradient penalty
    differentiates through it (a critic with tanh activations under WGAN-GP / R1)."""
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        y = torch.empty_like(x)
        check(_lib.lib().ganlab_tanh_fwd_f32(_p(x), _p(y), x.numel(), _st()), 'tanh_fwd')
        ctx.save_for_backward(y)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None
        y, = ctx.saved_tensors
        return _TanhBwd.apply(g, y)


class _TanhBwd(Function):
    """gx = g * (1 - y^2), y = tanh(x): linear in g, and d gx / d y = -2 g y (the second order of tanh)."""
    @staticmethod
    def forward(ctx, g, y):
        g, y = _c(g), _c(y)
        gx = torch.empty_like(g)
        check(_lib.lib().ganlab_tanh_bwd_f32(_p(g), _p(y), _p(gx), g.numel(), _st()), 'tanh_bwd')
        ctx.save_for_backward(g, y)
        return gx

    @staticmethod
    def backward(ctx, go):
        g, y = ctx.saved_tensors
        gg = _TanhBwd.apply(go, y) if ctx.needs_input_grad[0] else None
        gy = scale(mul(mul(go, g), y), -2.0) if ctx.needs_input_grad[1] else None
        return gg, gy


# ---------------------------------------------------------------------------------------------- #
# functional API
# ---------------------------------------------------------------------------------------------- #
def chan_affine(x, scale=None, shift=None):
    return _ChanAffine.apply(x, scale, shift)


def mul(a, b):
    return _Mul.apply(a, b)


def tanh(x):
    return _Tanh.apply(x)


def channel_sum(x):
    return _ChanSum.apply(x, None, 1.0)


def blur(x):
    return _Blur.apply(x)


def avg_pool2(x):
    return _Pool2.apply(x, 0.25)


def upsample2(x):
    return _Up2.apply(x, 1.0)


def resample(x, mode, align_corners=False):
    """``F.interpolate`` at scale 2 (``'bilinear_up'``) / 0.5 (``'bilinear_down'``, ``'nearest_down'``) of an NCHW map:
    nn.Upsample(mode='bilinear') / BilinearPool2d / NearestPool2d of the reference (custom_layers.py:59-75)."""
    if x.dim() == 3:
        x = x.view(-1, *x.shape)
    return _Resample.apply(x, mode, bool(align_corners), int(x.shape[2]), int(x.shape[3]), False)


def lerp(a, b, alpha):
    """a*(1-alpha) + b*alpha."""
    return _Axpby.apply(a, b, float(1.0 - alpha), float(alpha))


def scale(x, a):
    return _Scale.apply(x, float(a))


def add(a, b):
    """Residual sum a + b."""
    return _Axpby.apply(a, b, 1.0, 1.0)


def global_avg_pool(x):
    """nn.AvgPool2d(kernel_size=H) on an (N,C,H,H) map -> (N,C,1,1): plane sums through the channel-sum kernel."""
    n, c, h, w = x.shape
    return (_ChanSum.apply(x.reshape(1, n * c, h * w), None, 1.0 / (h * w))).view(n, c, 1, 1)


def pixelnorm(x, eps=1e-8):
    return _PixelNorm.apply(x, float(eps))


def group_broadcast(stat, group_size, h, w):
    return _GroupBroadcast.apply(stat, int(group_size), int(h), int(w))
