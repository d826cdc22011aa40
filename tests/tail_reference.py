"""Float64 restatement of the StyleGAN layer tail (the image-space half of csrc/pointwise.hip) and the per-element error bounds
the GPU tests hold the kernels to.  Written from the reference semantics - the blur of custom_layers.py:41-51, the layer tail
of stylegan/architectures.py:497-526 - in plain numpy; no kernel is ported.  Users: tests/test_tail_host.py (the restatement
against autograd and oracle.ops, and every bound against the mistakes it must catch), tests/test_gpu_tail.py (the kernels).

Conventions.  Arrays are float64 NCHW whose values are float32 numbers (``f32``), so the reference and the kernel read the same
operands; per-plane quantities are (N, C, 1, 1).  ``style`` is (N, 2C) = [ys | yb], ``noise`` (N, 1, H, W).  Every test feeds
a kernel its own exact inputs (a later stage gets the earlier kernel's fp32 output), so a LeakyReLU mask is always read from a
tensor both sides hold exactly.

Bounds.  u = 2^-24; ``gamma(k)`` = ku / (1 - ku) bounds k chained fp32 roundings (FMA contraction only removes some);
``half_ulp(v)`` is the error of the one rounding of an fp64 value v to fp32.  Sums that a kernel accumulates in fp64 get
``L_SUM * 2^-53`` times the sum of magnitudes: no thread of these kernels adds more than 128 terms (blur_fused_kernel<.., 8> with
statistics: 4 trips x 8 rows x 4 columns), the wave and block trees add 8 levels, the finishing kernels at most 16 partials at the
shapes tested - 160 covers them.  Nothing measured enters a bound."""
import numpy as np

U = 2.0 ** -24
D = 2.0 ** -53
L_SUM = 160
EPS = float(np.float32(1e-8))
SLOPE = float(np.float32(0.2))


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(a):
    """The float32 rounding of ``a`` as float64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def half_ulp(v):
    """Largest error of rounding the fp64 value(s) ``v`` to fp32 (half the spacing of fp32 at |v|, subnormals included)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64) * 0.5


def _plane(v):
    return v.sum(axis=(2, 3), keepdims=True)


def _per_channel(c):
    return None if c is None else np.asarray(c, dtype=np.float64).reshape(1, -1, 1, 1)


# ---- blur, up2, pool2 ---------------------------------------------------------------------------------------------------------
def blur(x):
    """[1 2 1] x [1 2 1] / 16 per plane, zero padding (custom_layers.py:41-51); symmetric taps, so it is its own adjoint."""
    p = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    h = p[..., :, :-2] + 2.0 * p[..., :, 1:-1] + p[..., :, 2:]
    return (h[..., :-2, :] + 2.0 * h[..., 1:-1, :] + h[..., 2:, :]) / 16.0


def blur_bound(x):
    """Every blur kernel adds the row taps l + 2c + r (2c exact: 2 roundings), then three rows the same way (2 more); / 16 is
    exact.  4 roundings on a path whose terms add up to blur(|x|)."""
    return gamma(4) * blur(np.abs(x))


def up2(x, scale):
    """Nearest-neighbour 2x upsampling times ``scale``; its adjoint is ``pool2`` with the same scale."""
    return scale * x.repeat(2, axis=2).repeat(2, axis=3)


def up2_bound(x, scale):
    """One product per output."""
    return U * np.abs(up2(x, scale))


def pool2(x, scale):
    """``scale`` times the sum of each 2x2 block (0.25: AvgPool2d(2))."""
    n, c, h, w = x.shape
    return scale * x.reshape(n, c, h // 2, 2, w // 2, 2).sum(axis=(3, 5))


def pool2_bound(x, scale):
    """(a + b) + (c + d), then the product: 3 roundings on scale * sum |x|."""
    return gamma(3) * pool2(np.abs(x), abs(scale))


# ---- sign bits ----------------------------------------------------------------------------------------------------------------
def sign_bits(x):
    """int32 words: bit e % 32 of word e // 32 is set iff element e of the NCHW-linear order is > 0."""
    b = (np.asarray(x).reshape(-1) > 0).astype(np.uint64).reshape(-1, 32)
    words = (b << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return words.view(np.int32)


def mask_from_bits(words, shape):
    w = np.asarray(words).view(np.uint32).astype(np.uint64)
    return (((w[:, None] >> np.arange(32, dtype=np.uint64)) & 1) != 0).reshape(shape)


# ---- bias, noise, activation ----------------------------------------------------------------------------------------------------
def bias_act(x, bias, noise, noise_w, bias_scale, slope):
    """y = act(x + noise_w[c] noise[n, hw] + bias[c] bias_scale); ``slope`` None: no activation.  Returns (y, z, mag): the
    pre-activation z and the sum of the magnitudes of its three terms."""
    z, mag = x.copy(), np.abs(x)
    if bias is not None:
        z = z + _per_channel(bias) * bias_scale
        mag = mag + np.abs(_per_channel(bias) * bias_scale)
    if noise is not None:
        z = z + _per_channel(noise_w) * noise
        mag = mag + np.abs(_per_channel(noise_w) * noise)
    y = z if slope is None else np.where(z > 0, z, slope * z)
    return y, z, mag


def bias_act_bound(z, mag, slope, pre=None):
    """bias * bias_scale (1 rounding), + x (1), + noise_w * noise (2, or 1 fused), * slope (1): at most 5 roundings of terms that
    add up to ``mag`` - scaled by the slope on the negative side, unless z lies within that bound of zero, where the kernel may
    stand on the other side of the kink (the difference is then below (1 - slope) |z| <= the unscaled bound).  ``pre``: a bound
    on the error x already carries (the fused blur in front)."""
    b = gamma(5) * mag + (0.0 if pre is None else pre)
    if slope is None:
        return b
    return np.where(z < -b, abs(slope), 1.0) * b


def near_kink_share(z, mag, slope):
    """Share of elements whose pre-activation lies within its forward bound of zero."""
    return float((np.abs(z) <= gamma(5) * mag).mean())


def act_bwd(gy, mask, noise, slope, bias_scale):
    """Backward of ``bias_act`` from the mask (y > 0): gz = gy where set, slope * gy elsewhere (so the slope side at y == 0,
    -0.0 included: the derivative nn.LeakyReLU uses); gb = bias_scale * sum_{n, hw} gz, gnw = sum_{n, hw} gz * noise."""
    gz = np.where(mask, gy, slope * gy)
    gb = bias_scale * gz.sum(axis=(0, 2, 3))
    gnw = (gz * noise).sum(axis=(0, 2, 3)) if noise is not None else None
    return gz, gb, gnw


def act_bwd_bounds(gy, mask, noise, slope, bias_scale):
    """gz: one product on the slope side, exact on the other.  gb and gnw as act_bwd_bias_stage1 / channel_sum_stage1 form them:
    the fp32 gz (rounded on the slope side only) is added in fp64 and the scaled sum rounded once; gnw multiplies the fp32 gz
    by the noise in fp64 (exact products)."""
    gz = np.where(mask, gy, slope * gy)
    gz_b = np.where(mask, 0.0, U * np.abs(gz))
    ch = lambda v: v.sum(axis=(0, 2, 3))                                    # noqa: E731
    gb = bias_scale * ch(gz)
    gb_b = half_ulp(gb) + abs(bias_scale) * (ch(gz_b) + L_SUM * D * ch(np.abs(gz)))
    gnw_b = None
    if noise is not None:
        gnw_b = half_ulp(ch(gz * noise)) + ch(gz_b * np.abs(noise)) + L_SUM * D * ch(np.abs(gz * noise))
    return gz_b, gb_b, gnw_b


def channel_sum(a, b, scale):
    """scale * sum_{n, hw} a[n, c, hw] * (b[n, hw] or 1), and its bound: fp64 sums of exact products, one rounding."""
    t = a * b if b is not None else a
    s = scale * t.sum(axis=(0, 2, 3))
    return s, half_ulp(s) + abs(scale) * L_SUM * D * np.abs(t).sum(axis=(0, 2, 3))


# ---- InstanceNorm statistics ----------------------------------------------------------------------------------------------------
def instnorm_stats(x, eps=EPS):
    """(mean, var, rstd) per plane: biased variance, rstd = 1 / sqrt(var + eps) (nn.InstanceNorm2d, custom_layers.py:98-99)."""
    mean = x.mean(axis=(2, 3), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(2, 3), keepdims=True)
    return mean, var, 1.0 / np.sqrt(var + eps)


def stats_bounds(x, eps=EPS):
    """The kernels add x and x^2 (exact in fp64) in fp64, form var = E[x^2] - mean^2 in fp64 and store fp32 (mean, rstd).
    mean: one rounding to fp32 plus the fp64 sum.  rstd: one rounding, plus the fp64 error of var - relative to E[x^2] + mean^2,
    so it grows as var shrinks against mean^2 (the near-constant planes) - through d rstd / d var = -rstd / (2 (var + eps))."""
    mean, var, rstd = instnorm_stats(x, eps)
    ex2 = (x ** 2).mean(axis=(2, 3), keepdims=True)
    mean_b = half_ulp(mean) + L_SUM * D * np.abs(x).mean(axis=(2, 3), keepdims=True)
    var_b = (L_SUM + 4) * D * (ex2 + mean ** 2)
    rstd_b = half_ulp(rstd) + rstd * (0.5 * var_b / (var + eps) + 4 * D)
    return mean_b, rstd_b


def _style_parts(style, n, c):
    if style is None:
        return np.ones((n, c, 1, 1)), np.zeros((n, c, 1, 1))
    st = np.asarray(style, dtype=np.float64).reshape(n, 2, c, 1, 1)
    return st[:, 0] + 1.0, st[:, 1]


# ---- InstanceNorm + style -------------------------------------------------------------------------------------------------------
def instnorm_style(x, style, eps=EPS):
    """y = (x - mean) rstd (ys + 1) + yb (stylegan/architectures.py:524-526); style None: the plain normalisation."""
    n, c = x.shape[:2]
    mean, _, rstd = instnorm_stats(x, eps)
    ys1, yb = _style_parts(style, n, c)
    return (x - mean) * rstd * ys1 + yb


def instnorm_style_bound(x, style, eps=EPS):
    """The forward kernels read the fp32 (mean^, rstd^) and compute (x - mean^) * (rstd^ * (ys + 1)) + yb in fp32:
      rstd |ys + 1| |mean^ - mean|        the stored mean's rounding, amplified by rstd: it dominates on near-constant planes
                                           and belongs to the design (statistics are kept in fp32);
      |xhat (ys + 1)| (e_r + gamma(5))    the stored rstd's relative error e_r, and the roundings of x - mean^, ys + 1,
                                           rstd^ * (ys + 1), the product and the final sum;
      u |yb|                              the final sum's share of yb."""
    n, c = x.shape[:2]
    mean, _, rstd = instnorm_stats(x, eps)
    mean_b, rstd_b = stats_bounds(x, eps)
    ys1, yb = _style_parts(style, n, c)
    xhat = (x - mean) * rstd
    return rstd * np.abs(ys1) * mean_b + np.abs(xhat * ys1) * (rstd_b / rstd + gamma(5)) + U * np.abs(yb)


def instnorm_style_bwd(gy, x, style, eps=EPS):
    """Closed form of the backward: s1 = sum gy, s2 = sum gy xhat per plane, gx = rstd (ys + 1) (gy - s1 / HW - xhat s2 / HW),
    dstyle = [s2 | s1] (d / d ys, d / d yb).  Returns (gx, dstyle, s1, s2)."""
    n, c, h, w = x.shape
    mean, _, rstd = instnorm_stats(x, eps)
    ys1, _ = _style_parts(style, n, c)
    xhat = (x - mean) * rstd
    s1, s2 = _plane(gy), _plane(gy * xhat)
    gx = rstd * ys1 * (gy - s1 / (h * w) - xhat * s2 / (h * w))
    dstyle = np.concatenate([s2.reshape(n, c), s1.reshape(n, c)], axis=1)
    return gx, dstyle, s1, s2


def instnorm_bwd_bounds(gy, x, style, eps=EPS, g_err=None, fp64_apply=False):
    """Bounds (gx_b, s1_b, s2_b) of the backward kernels, which read the stored fp32 (mean^, rstd^) and write fp32 (s1^, s2^).
    With e_m = |mean^ - mean|, e_r = |rstd^ - rstd| / rstd from ``stats_bounds`` and HW the plane size:

    s1 (instnorm_bwd_reduce_kernel, and the toRGB-folded form): fp64 sum of the fp32 gy, one rounding.
    s2: fp64 sum of gy * xhat^ with xhat^ = fl(fl(x - mean^) * rstd^) formed in fp32 (2 roundings), the product exact in fp64:
        the mean's error enters as rstd e_m |sum gy|, rstd's as e_r |s2| (both are common to the plane), the two roundings as
        gamma(2) sum |gy xhat|.
    The input errors then propagate into gx = k I, k = rstd (ys + 1), I = gy - s1 / HW - xhat s2 / HW, as
        P = |k| (s1_b / HW + (rstd e_m + |xhat| e_r) |s2| / HW + |xhat| s2_b / HW + g_err) + e_r |gx|.
    ``fp64_apply`` (instnorm_bwd_apply_act_kernel and its blur / toRGB forms): the element formula runs in fp64 on those inputs
    and is rounded once - P + a dozen fp64 roundings here, plus u |gx| for ys + 1, which the plain and the toRGB form add in fp32
    before they widen it (the blur form adds it in fp64); the one fp32 rounding of the result is added by
    ``layer_tail_bwd_bounds`` (after the slope).  Otherwise (instnorm_bwd_apply_kernel, all fp32):
        |k| (gamma(2) T2 + gamma(5) T3 + gamma(2) (T1 + T2 + T3)) + gamma(3) |gx|,   T1 = |gy|, T2 = |s1| / HW, T3 = |xhat s2| / HW:
    fl(1 / HW) and the product in a1 = s1^ / HW and a2; x - mean^, * rstd^, * a2 on top of a2's two; the two subtractions; ys + 1,
    rstd^ * (ys + 1) and the last product.
    ``g_err``: a per-element bound on an error gy itself carries (the toRGB fold recomputes gy in fp32)."""
    n, c, h, w = x.shape
    hw = h * w
    mean, _, rstd = instnorm_stats(x, eps)
    mean_b, rstd_b = stats_bounds(x, eps)
    e_m, e_r = mean_b, rstd_b / rstd
    ys1, _ = _style_parts(style, n, c)
    xhat = (x - mean) * rstd
    ge = np.zeros_like(gy) if g_err is None else g_err
    s1, s2 = _plane(gy), _plane(gy * xhat)
    s1_b = half_ulp(s1) + L_SUM * D * _plane(np.abs(gy)) + _plane(ge)
    s2_b = half_ulp(s2) + L_SUM * D * _plane(np.abs(gy * xhat)) + rstd * e_m * np.abs(s1) + e_r * np.abs(s2) + \
        gamma(2) * _plane(np.abs(gy * xhat)) + _plane(ge * np.abs(xhat))
    k = np.abs(rstd * ys1)
    t1, t2, t3 = np.abs(gy), np.abs(s1) / hw, np.abs(xhat * s2) / hw
    gx = rstd * ys1 * (gy - s1 / hw - xhat * s2 / hw)
    p = k * (s1_b / hw + (rstd * e_m + np.abs(xhat) * e_r) * np.abs(s2) / hw + np.abs(xhat) * s2_b / hw + ge) + e_r * np.abs(gx)
    if fp64_apply:
        gx_b = p + 12 * D * k * (t1 + t2 + t3) + (U * np.abs(gx) if style is not None else 0.0)
    else:
        gx_b = p + k * (gamma(2) * t2 + gamma(5) * t3 + gamma(2) * (t1 + t2 + t3)) + gamma(3) * np.abs(gx)
    return gx_b, s1_b, s2_b


# ---- the whole tail, backward ---------------------------------------------------------------------------------------------------
def layer_tail_bwd(gout, y, style, noise, slope, bias_scale, eps=EPS, with_blur=False):
    """Backward of out = InstanceNorm(y) (ys + 1) + yb with y = act(blur?(x) + noise_w noise + bias bias_scale), from the
    activated tensor y (mask y > 0; ``slope`` None: no activation): gz = mask' * d/dy, returned blurred when the layer has a blur
    in front; gb = bias_scale sum gz, gnw = sum gz noise, dstyle = [s2 | s1].  Returns (gx, gb, gnw, dstyle, gz)."""
    gy_in, dstyle, _, _ = instnorm_style_bwd(gout, y, style, eps)
    mask = (y > 0) if slope is not None else np.ones(y.shape, dtype=bool)
    gz, gb, gnw = act_bwd(gy_in, mask, noise, 1.0 if slope is None else slope, bias_scale)
    return (blur(gz) if with_blur else gz), gb, gnw, dstyle, gz


def layer_tail_bwd_bounds(gout, y, style, noise, slope, bias_scale, eps=EPS, with_blur=False, g_err=None):
    """instnorm_bwd_apply_act_kernel (and its blur / toRGB forms): z in fp64 from the fp32 inputs, times the slope in fp64, rounded
    once -> ``instnorm_bwd_bounds(fp64_apply=True)`` scaled by the slope where the mask is clear.  gb and gnw add the UNROUNDED
    fp64 z: one rounding of the scaled sum, plus the propagated input errors of every addend (without their own rounding).
    Blurred: the fp32 z goes through the blur's 4 roundings.  Returns (gx_b, gb_b, gnw_b, s1_b, s2_b)."""
    zb, s1_b, s2_b = instnorm_bwd_bounds(gout, y, style, eps, g_err=g_err, fp64_apply=True)
    _, gb, gnw, _, gz = layer_tail_bwd(gout, y, style, noise, slope, bias_scale, eps)
    sf = np.where(y > 0, 1.0, abs(slope)) if slope is not None else 1.0
    prop = zb * sf + L_SUM * D * np.abs(gz)                                 # what an addend of the fp64 sums carries
    zb = zb * sf + half_ulp(gz)
    ch = lambda v: v.sum(axis=(0, 2, 3))                                    # noqa: E731
    gb_b = half_ulp(gb) + abs(bias_scale) * ch(prop)
    gnw_b = half_ulp(gnw) + ch(prop * np.abs(noise)) if noise is not None else None
    gx_b = blur(zb) + gamma(4) * blur(np.abs(gz)) if with_blur else zb
    return gx_b, gb_b, gnw_b, s1_b, s2_b


# ---- blur fused with the activation backward (the critic's conv -> LeakyReLU -> blur) --------------------------------------------
def blur_act_bwd(g, mask, slope, bias_scale):
    """out = lrelu'(mask) * blur(g), gb = bias_scale sum out: the backward of blur(lrelu(.)) (the blur is its own adjoint)."""
    out = np.where(mask, 1.0, slope) * blur(g)
    return out, bias_scale * out.sum(axis=(0, 2, 3))


def blur_act_bwd_bounds(g, mask, slope, bias_scale):
    """blur_fused_kernel<BF_A>: the blur's 4 roundings and the slope product; gb adds the ROUNDED fp32 outputs in fp64."""
    out, gb = blur_act_bwd(g, mask, slope, bias_scale)
    out_b = gamma(5) * np.where(mask, 1.0, abs(slope)) * blur(np.abs(g))
    ch = lambda v: v.sum(axis=(0, 2, 3))                                    # noqa: E731
    return out_b, half_ulp(gb) + abs(bias_scale) * (ch(out_b) + L_SUM * D * ch(np.abs(out)))


def act_bwd_blur(g, mask, noise, slope, bias_scale):
    """Its adjoint, the backward of act(blur(x) + ...): z = lrelu'(mask) g, out = blur(z), gb = bias_scale sum z, gnw = sum z noise."""
    z, gb, gnw = act_bwd(g, mask, noise, slope, bias_scale)
    return blur(z), gb, gnw


def act_bwd_blur_bounds(g, mask, noise, slope, bias_scale):
    """blur_fused_kernel<BF_AT>: the masked operand is rounded (slope side), then blurred (4 roundings); the sums add the fp32
    masked values in fp64 like ``act_bwd_bounds``."""
    z = np.where(mask, g, slope * g)
    z_b, gb_b, gnw_b = act_bwd_bounds(g, mask, noise, slope, bias_scale)
    return blur(z_b) + gamma(4) * blur(np.abs(z)), gb_b, gnw_b


# ---- toRGB (1x1) on the normalised tensor -----------------------------------------------------------------------------------------
def torgb(b, w, bias, scale, bias_scale):
    """rgb[n, k] = scale sum_c w[k, c] b[n, c] + bias[k] bias_scale."""
    return scale * np.einsum('kc,nchw->nkhw', w, b) + _per_channel(bias) * bias_scale


def torgb_input_grad(grgb, w, scale):
    """gy = scale W^T grgb and the bound of its fp32 recomputation inside the folded kernels (gl_few_dot: the K image channels in
    order, starting from 0), term by term: term k carries the rounding of the packed weight fl(w * scale), of its product, and
    of every sum it then passes through - K - 1 for k = 0 (its own sum with the 0 start is exact), K - k after that; channels past
    K have zero weights and add nothing.  For K = 3: gamma(4), gamma(4), gamma(3) on |scale w[k, c] grgb[n, k]| (the same counts
    hold fused or not: an FMA only drops the product's rounding).  The sums over a plane inherit this once per element."""
    kk = w.shape[0]
    gy = scale * np.einsum('kc,nkhw->nchw', w, grgb)
    g_err = np.zeros_like(gy)
    for k in range(kk):
        passes = 2 + (kk - 1 if k == 0 else kk - k)
        g_err += gamma(passes) * np.abs(scale * w[k][None, :, None, None] * grgb[:, k:k + 1])
    return gy, g_err


# ---- operands -------------------------------------------------------------------------------------------------------------------
REGIMES = ('normal', 'near3', 'near1')
TAIL_SHAPES = [(32, 32), (36, 228), (6, 172), (512, 8), (16, 16), (5, 7)]      # the layer-tail cases of test_gpu_tail.py


def tail_seed(h, w):
    return 7 * h + w


def regime_plane(rng, shape, regime):
    """Statistics-bearing operands: unit normal; near-constant planes (offset 3 with std 1e-2, offset 1 with std 3e-4)."""
    offset, std = {'normal': (0.0, 1.0), 'near3': (3.0, 1e-2), 'near1': (1.0, 3e-4)}[regime]
    return f32(offset + std * rng.standard_normal(shape)), std


def tail_operands(seed, n, c, h, w, regime='normal', noise=True, bias=True, style=True):
    """(x, bias, noise, noise_w, style, gout) of one layer-tail case.  In the near-constant regimes the bias and the noise weight
    are scaled with the plane's spread, so the activated plane stays near-constant (and positive)."""
    rng = np.random.RandomState(seed)
    x, std = regime_plane(rng, (n, c, h, w), regime)
    return (x,
            f32(std * 0.5 * rng.standard_normal(c)) if bias else None,
            f32(rng.standard_normal((n, 1, h, w))) if noise else None,
            f32(std * 0.3 * rng.standard_normal(c)) if noise else None,
            f32(0.5 * rng.standard_normal((n, 2 * c))) if style else None,
            f32(rng.standard_normal((n, c, h, w))))
