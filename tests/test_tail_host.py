"""CPU checks of tests/tail_reference.py, the float64 restatement behind tests/test_gpu_tail.py:

* the forward formulas equal ``oracle.ops`` evaluated in float64, and every closed-form backward equals torch autograd in
  float64 on the composed forward, to 1e-12 relative;
* each mistake the GPU tests are meant to catch, applied to the reference itself, falls OUTSIDE the bound the GPU test uses, at
  the shape that test uses - a bound that let one of them pass would be decoration."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_reference as ref
from oracle import ops as O

EPS, SLOPE, BS = ref.EPS, ref.SLOPE, float(np.float32(0.7))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))                     # noqa: E731


def _close(what, a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300), (what, np.abs(a - b).max())


def _outside(what, wrong, right, bound, margin=2.0):
    """The perturbed result leaves the bound somewhere, and by a margin (twice the bound unless said otherwise)."""
    ratio = np.abs(np.asarray(wrong) - np.asarray(right)) / np.maximum(np.asarray(bound), 1e-300)
    print(f'tail host | {what}: worst error / bound {ratio.max():.3g}')
    assert ratio.max() > margin, (what, float(ratio.max()))


def _composed(x, bias, noise, noise_w, style, with_blur, act=True):
    """The layer tail with torch ops in float64 (stylegan/architectures.py:497-526): returns (activated tensor, output)."""
    c = x.shape[1]
    z = O.blur_binomial(x) if with_blur else x
    z = O.add_noise(z, noise_w.view(1, c, 1, 1), noise) + bias.view(1, c, 1, 1) * BS
    y = O.lrelu(z, SLOPE) if act else z
    return y, O.adain_affine(O.instancenorm(y, EPS), style)


# ---- the restatement is right -------------------------------------------------------------------------------------------------------
def test_forward_equals_the_oracle_in_float64():
    x, b, nz, nw, style, _ = ref.tail_operands(1, 2, 3, 6, 10)
    _close('blur', ref.blur(x), O.blur_binomial(T(x)))
    _close('pool2', ref.pool2(x, 0.25), O.avgpool2(T(x)))
    _close('up2', ref.up2(x, 1.0), O.upsample2(T(x)))
    _close('instancenorm', ref.instnorm_style(x, None), O.instancenorm(T(x), EPS))
    _close('adain', ref.instnorm_style(x, style), O.adain_affine(O.instancenorm(T(x), EPS), T(style)))
    for with_blur in (False, True):
        y, out = _composed(T(x), T(b), T(nz), T(nw), T(style), with_blur)
        yr, _, _ = ref.bias_act(ref.blur(x) if with_blur else x, b, nz, nw, BS, SLOPE)
        _close('bias_act', yr, y)
        _close('tail', ref.instnorm_style(yr, style), out)
    m, v, r = ref.instnorm_stats(x)
    _close('mean', m, T(x).mean(dim=(2, 3), keepdim=True))
    _close('rstd', r, 1.0 / torch.sqrt(T(x).var(dim=(2, 3), unbiased=False, keepdim=True) + EPS))


def test_sign_bit_packing():
    x = ref.f32(np.random.RandomState(0).standard_normal((2, 3, 2, 32)))
    x.reshape(-1)[[0, 31, 32, 95]] = [0.0, -0.0, 1.0, -1.0]
    bits = ref.sign_bits(x)
    assert bits.dtype == np.int32 and bits.shape == (x.size // 32,)
    flat = x.reshape(-1)
    for e in (0, 1, 31, 32, 33, 95, 96, 383):
        assert bool((int(bits.view(np.uint32)[e // 32]) >> (e % 32)) & 1) == bool(flat[e] > 0), e
    assert np.array_equal(ref.mask_from_bits(bits, x.shape), x > 0)


@pytest.mark.parametrize('with_blur', [False, True])
@pytest.mark.parametrize('hw', [(5, 7), (6, 8)])
def test_closed_form_backwards_equal_autograd(hw, with_blur):
    h, w = hw
    x, b, nz, nw, style, gout = ref.tail_operands(h, 2, 3, h, w)
    leaves = [T(t).clone().requires_grad_(True) for t in (x, b, nw, style)]
    xt, bt, nwt, st = leaves
    y, out = _composed(xt, bt, T(nz), nwt, st, with_blur)
    ya = y.detach().numpy()
    # InstanceNorm + style alone, from the activated tensor
    gy_t, gs_t = torch.autograd.grad(out, (y, st), T(gout), retain_graph=True)
    gy, dstyle, s1, s2 = ref.instnorm_style_bwd(gout, ya, style)
    _close('instnorm gx', gy, gy_t)
    _close('dstyle', dstyle, gs_t)
    yl = T(ya).clone().requires_grad_(True)
    gp, = torch.autograd.grad(O.instancenorm(yl, EPS), yl, T(gout))
    _close('plain instnorm gx', ref.instnorm_style_bwd(gout, ya, None)[0], gp)
    # the whole tail
    gx_t, gb_t, gnw_t, gs_t = torch.autograd.grad(out, leaves, T(gout), retain_graph=True)
    gx, gb, gnw, dstyle, _ = ref.layer_tail_bwd(gout, ya, style, nz, SLOPE, BS, with_blur=with_blur)
    for nm, a, t in (('gx', gx, gx_t), ('gb', gb, gb_t), ('gnw', gnw, gnw_t), ('dstyle', dstyle, gs_t)):
        _close(f'tail {nm}', a, t)
    # bias_act backward alone (and, blurred, the act'-then-blur pass)
    gx_t, gb_t, gnw_t = torch.autograd.grad(y, (xt, bt, nwt), T(gout), retain_graph=True)
    fn = ref.act_bwd_blur if with_blur else ref.act_bwd
    for nm, a, t in zip(('gx', 'gb', 'gnw'), fn(gout, ya > 0, nz, SLOPE, BS), (gx_t, gb_t, gnw_t)):
        _close(f'bias_act {nm}', a, t)
    # blur-then-activation backward: blur(lrelu(a + bias))
    a_t, b2 = T(x).clone().requires_grad_(True), T(b).clone().requires_grad_(True)
    act = O.lrelu(a_t + b2.view(1, -1, 1, 1) * BS, SLOPE)
    ga, gb2 = torch.autograd.grad(O.blur_binomial(act), (a_t, b2), T(gout))
    o, gb = ref.blur_act_bwd(gout, act.detach().numpy() > 0, SLOPE, BS)
    _close('blur_act_bwd out', o, ga)
    _close('blur_act_bwd gb', gb, gb2)
    # blur, up2, pool2 adjoints
    xl = T(x).clone().requires_grad_(True)
    _close('blur adjoint', ref.blur(gout), torch.autograd.grad(O.blur_binomial(xl), xl, T(gout))[0])
    if h % 2 == 0:
        g_small = gout[:, :, :h // 2, :w // 2]
        _close('pool2 adjoint', ref.up2(g_small, 0.3), torch.autograd.grad(0.3 * 4 * O.avgpool2(xl), xl, T(g_small))[0])
        xs = T(g_small).clone().requires_grad_(True)
        _close('up2 adjoint', ref.pool2(gout, 0.3), torch.autograd.grad(0.3 * O.upsample2(xs), xs, T(gout))[0])


def test_torgb_fold_equals_autograd():
    n, c, h, w = 2, 5, 4, 6
    x, b, nz, nw, style, _ = ref.tail_operands(9, n, c, h, w)
    rng = np.random.RandomState(1)
    wr, br, grgb = rng.standard_normal((3, c)), rng.standard_normal(3), rng.standard_normal((n, 3, h, w))
    leaves = [T(t).clone().requires_grad_(True) for t in (x, b, nw, style)]
    y, out = _composed(leaves[0], leaves[1], T(nz), leaves[2], leaves[3], False)
    rgb = 0.4 * F.conv2d(out, T(wr).view(3, c, 1, 1)) + T(br).view(1, 3, 1, 1)
    _close('torgb', ref.torgb(out.detach().numpy(), wr, br, 0.4, 1.0), rgb)
    gy_t, = torch.autograd.grad(rgb, out, T(grgb), retain_graph=True)
    gy, _ = ref.torgb_input_grad(grgb, wr, 0.4)
    _close('torgb input gradient', gy, gy_t)
    grads = torch.autograd.grad(rgb, leaves, T(grgb))
    gx, gb, gnw, dstyle, _ = ref.layer_tail_bwd(gy, y.detach().numpy(), style, nz, SLOPE, BS)
    for nm, a, t in zip(('gx', 'gb', 'gnw', 'dstyle'), (gx, gb, gnw, dstyle), grads):
        _close(f'folded {nm}', a, t)


def test_the_gpu_cases_keep_clear_of_the_kink():
    """The seeds of test_gpu_tail.py: fewer than 1e-3 of the pre-activations lie within their forward bound of zero."""
    for h, w in ref.TAIL_SHAPES:
        for regime in ref.REGIMES:
            x, b, nz, nw, _, _ = ref.tail_operands(ref.tail_seed(h, w), 2, 3, h, w, regime)
            for xin in (x, ref.blur(x)):
                _, z, mag = ref.bias_act(xin, b, nz, nw, BS, SLOPE)
                assert ref.near_kink_share(z, mag, SLOPE) < 1e-3, (h, w, regime)


# ---- the bounds have teeth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(5, 7), (12, 16), (1, 9), (9, 1)])
def test_a_border_blurred_with_the_wrong_padding(hw):
    x = ref.f32(np.random.RandomState(2).standard_normal((3, 8) + hw))
    for axis, pad in ((2, ((0, 0), (0, 0), (0, 1), (0, 0))), (3, ((0, 0), (0, 0), (0, 0), (0, 1)))):
        grown = np.pad(x, pad, mode='edge')                                # the row / column past the border repeats the last one
        wrong = ref.blur(grown)[:, :, :hw[0], :hw[1]]
        _outside(f'blur {hw} edge-padded axis {axis}', wrong, ref.blur(x), ref.blur_bound(x))


def test_up2_and_pool2_without_their_scale():
    x = ref.f32(np.random.RandomState(3).standard_normal((2, 3, 6, 10)))
    s = float(np.float32(0.3))
    _outside('up2 scale', ref.up2(x, 1.0), ref.up2(x, s), ref.up2_bound(x, s))
    _outside('pool2 scale', ref.pool2(x, 1.0), ref.pool2(x, s), ref.pool2_bound(x, s))


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('hw', [(4, 6), (32, 32), (36, 228)])
def test_bias_act_mistakes(hw, regime):
    h, w = hw
    x, b, nz, nw, _, _ = ref.tail_operands(ref.tail_seed(h, w), 2, 3, h, w, regime)
    y, z, mag = ref.bias_act(x, b, nz, nw, BS, SLOPE)
    bound = ref.bias_act_bound(z, mag, SLOPE)
    skipped = y.copy()
    skipped.reshape(2, 3, -1)[:, :, -4:] = np.where(x > 0, x, SLOPE * x).reshape(2, 3, -1)[:, :, -4:]   # bias and noise never added
    _outside(f'bias_act {hw} {regime}: last float4 of a plane skipped', skipped, y, bound)
    shifted, _, _ = ref.bias_act(x, b, np.roll(nz, 1, axis=0), nw, BS, SLOPE)
    _outside(f'bias_act {hw} {regime}: noise of the neighbouring image', shifted, y, bound)


def test_slope_on_the_wrong_side_of_zero():
    rng = np.random.RandomState(4)
    gy, y = ref.f32(rng.standard_normal((2, 3, 4, 6))), ref.f32(rng.standard_normal((2, 3, 4, 6)))
    y.reshape(-1)[::7] = 0.0
    y.reshape(-1)[3::11] = -0.0
    gz, gb, _ = ref.act_bwd(gy, y > 0, None, SLOPE, BS)
    gz_b, gb_b, _ = ref.act_bwd_bounds(gy, y > 0, None, SLOPE, BS)
    wrong, wrong_gb, _ = ref.act_bwd(gy, y >= 0, None, SLOPE, BS)
    _outside('act_bwd at y == 0', wrong, gz, np.maximum(gz_b, ref.U * np.abs(gz)))
    _outside('act_bwd_bias at y == 0', wrong_gb, gb, gb_b)


def test_one_sign_bit_word_shifted():
    x = ref.f32(np.random.RandomState(5).standard_normal((2, 3, 6, 32)))
    bits = ref.sign_bits(x)
    assert not np.array_equal(np.roll(bits, 1), bits)
    moved = bits.copy()
    moved[[7, 8]] = moved[[8, 7]]                                          # one row's word lands in its neighbour's place
    assert not np.array_equal(moved, bits)
    g = ref.f32(np.random.RandomState(6).standard_normal(x.shape))
    out, gb = ref.blur_act_bwd(g, x > 0, SLOPE, BS)
    out_b, gb_b = ref.blur_act_bwd_bounds(g, x > 0, SLOPE, BS)
    wrong, wrong_gb = ref.blur_act_bwd(g, ref.mask_from_bits(moved, x.shape), SLOPE, BS)
    _outside('BF_A with a shifted mask word', wrong, out, out_b)
    _outside('BF_A gb with a shifted mask word', wrong_gb, gb, gb_b)


def _chunk1(hw4):
    """Elements of the second contiguous chunk of a plane of ``hw4`` float4 cut in two (chunk_range of csrc/pointwise.hip)."""
    rows = (hw4 + 255) // 256
    per = (rows + 1) // 2
    return slice(per * 256 * 4, hw4 * 4)


@pytest.mark.parametrize('regime', ref.REGIMES)
def test_statistics_mistakes(regime):
    """36x228: 2052 float4 per plane, two chunks, the second ragged; 33x33: a plane size that is no power of two."""
    n, c, h, w = 2, 3, 36, 228
    x, _ = ref.regime_plane(np.random.RandomState(7), (n, c, h, w), regime)
    mean, var, rstd = ref.instnorm_stats(x)
    mean_b, rstd_b = ref.stats_bounds(x)
    flat = x.reshape(n, c, -1)
    cut = flat.copy()
    cut[:, :, _chunk1(h * w // 4)] = 0.0
    m2 = cut.sum(axis=2).reshape(n, c, 1, 1) / (h * w)
    v2 = (cut ** 2).sum(axis=2).reshape(n, c, 1, 1) / (h * w) - m2 ** 2
    _outside(f'{regime}: mean without the second chunk', m2, mean, mean_b)
    _outside(f'{regime}: rstd without the second chunk', 1.0 / np.sqrt(np.maximum(v2, 0) + EPS), rstd, rstd_b)
    last = flat.copy()
    last[:, :, -4:] = 0.0
    _outside(f'{regime}: mean without the last float4', last.sum(axis=2).reshape(n, c, 1, 1) / (h * w), mean, mean_b)
    # the mean rounded twice: the plane sum stored as fp32 before the division (33x33 = 1089 elements)
    x33, _ = ref.regime_plane(np.random.RandomState(8), (4, 8, 33, 33), regime)
    m33, _, _ = ref.instnorm_stats(x33)
    twice = ref.f32(ref.f32(x33.sum(axis=(2, 3), keepdims=True)) * ref.f32(1.0 / 1089))
    # (a second rounding can only add another half ulp or so: outside the bound on some of the 32 planes, by no wide margin)
    _outside(f'{regime}: mean rounded twice', twice, m33, ref.stats_bounds(x33)[0], margin=1.25)
    if regime != 'normal':
        # variance as fp32 E[x^2] - mean^2: the cancellation the fp64 sums exist to avoid
        x32 = x.astype(np.float32)
        m32 = x32.mean(axis=(2, 3), keepdims=True, dtype=np.float32)
        v32 = (x32 * x32).mean(axis=(2, 3), keepdims=True, dtype=np.float32) - m32 * m32
        r32 = 1.0 / np.sqrt(np.maximum(v32.astype(np.float64), 0) + EPS)
        _outside(f'{regime}: fp32 variance by E[x^2] - mean^2', r32, rstd, rstd_b)
        y = ref.instnorm_style(x, None)
        _outside(f'{regime}: output with that rstd', (x - mean) * r32, y, ref.instnorm_style_bound(x, None))


@pytest.mark.parametrize('regime', ref.REGIMES)
def test_a_dropped_chunk_in_the_backward_sums(regime):
    n, c, h, w = 2, 3, 36, 228
    x, b, nz, nw, style, gout = ref.tail_operands(ref.tail_seed(h, w), n, c, h, w, regime)
    y, _, _ = ref.bias_act(x, b, nz, nw, BS, SLOPE)
    y = ref.f32(y)
    keep = np.ones((1, 1, h * w))
    keep[:, :, _chunk1(h * w // 4)] = 0.0
    keep = keep.reshape(1, 1, h, w)
    # s1, s2 of the reduce pass -> dstyle, and the input gradient that inherits them
    gx, dstyle, s1, s2 = ref.instnorm_style_bwd(gout, y, style)
    for fp64_apply in (False, True):
        gx_b, s1_b, s2_b = ref.instnorm_bwd_bounds(gout, y, style, fp64_apply=fp64_apply)
        mean, _, rstd = ref.instnorm_stats(y)
        xhat = (y - mean) * rstd
        w1, w2 = (gout * keep).sum(axis=(2, 3), keepdims=True), (gout * xhat * keep).sum(axis=(2, 3), keepdims=True)
        _outside(f'{regime}: s1 without a chunk', w1, s1, s1_b)
        _outside(f'{regime}: s2 without a chunk', w2, s2, s2_b)
        ys1 = style.reshape(n, 2, c, 1, 1)[:, 0] + 1.0
        wrong = rstd * ys1 * (gout - w1 / (h * w) - xhat * s2 / (h * w))
        _outside(f'{regime}: gx from that s1', wrong, gx, gx_b + ref.half_ulp(gx))
    # gb, gnw of the fused apply pass
    _, gb, gnw, _, gz = ref.layer_tail_bwd(gout, y, style, nz, SLOPE, BS)
    _, gb_b, gnw_b, _, _ = ref.layer_tail_bwd_bounds(gout, y, style, nz, SLOPE, BS)
    _outside(f'{regime}: tail gb without a chunk', BS * (gz * keep).sum(axis=(0, 2, 3)), gb, gb_b)
    _outside(f'{regime}: tail gnw without a chunk', (gz * keep * nz).sum(axis=(0, 2, 3)), gnw, gnw_b)
    # gb, gnw of bias_act's own backward at N HW = 8200 (41x100): the interleaved second chunk of channel_chunks
    x, b, nz, nw, _, gy = ref.tail_operands(17 + 100, 2, 3, 41, 100)
    mask = ref.bias_act(x, b, nz, nw, BS, SLOPE)[0] > 0
    gz, gb, gnw = ref.act_bwd(gy, mask, nz, SLOPE, BS)
    _, gb_b, gnw_b = ref.act_bwd_bounds(gy, mask, nz, SLOPE, BS)
    idx = np.arange(2 * 4100 // 4)
    keep4 = ((idx // 256) % 2 == 0).repeat(4).reshape(2, 1, 41, 100)
    _outside('act_bwd_bias gb without a chunk', BS * (gz * keep4).sum(axis=(0, 2, 3)), gb, gb_b)
    _outside('channel_sum gnw without a chunk', (gz * keep4 * nz).sum(axis=(0, 2, 3)), gnw, gnw_b)


def test_blurred_tail_with_a_wrong_border():
    """The blur inside the fused backward (instnorm_bwd_act_blur_kernel) and forward (BF_FWD) with an edge-padded last column."""
    n, c, h, w = 2, 3, 6, 172
    x, b, nz, nw, style, gout = ref.tail_operands(ref.tail_seed(h, w), n, c, h, w)
    y = ref.f32(ref.bias_act(ref.blur(x), b, nz, nw, BS, SLOPE)[0])
    gx, _, _, _, gz = ref.layer_tail_bwd(gout, y, style, nz, SLOPE, BS, with_blur=True)
    gx_b = ref.layer_tail_bwd_bounds(gout, y, style, nz, SLOPE, BS, with_blur=True)[0]
    wrong = ref.blur(np.pad(gz, ((0, 0), (0, 0), (0, 0), (0, 1)), mode='edge'))[..., :w]
    _outside('blurred tail gx', wrong, gx, gx_b)
    yr, z, mag = ref.bias_act(ref.blur(x), b, nz, nw, BS, SLOPE)
    wrong = ref.bias_act(ref.blur(np.pad(x, ((0, 0), (0, 0), (0, 0), (0, 1)), mode='edge'))[..., :w], b, nz, nw, BS, SLOPE)[0]
    _outside('blurred forward', wrong, yr, ref.bias_act_bound(z, mag, SLOPE, pre=ref.blur_bound(x)))


def test_folded_sums_without_the_last_float4():
    """The toRGB-folded passes at their GPU shape (16 channels, 32x32: one chunk per image): the bound that carries the fp32
    recomputation of gy still rejects sums that miss a plane's last four elements."""
    n, c, h, w = 2, 16, 32, 32
    x, b, nz, nw, style, _ = ref.tail_operands(c + h, n, c, h, w)
    rng = np.random.RandomState(c)
    wr, grgb = ref.f32(rng.standard_normal((3, c)) * 0.5), ref.f32(rng.standard_normal((n, 3, h, w)))
    y = ref.f32(ref.bias_act(x, b, nz, nw, BS, SLOPE)[0])
    gy, g_err = ref.torgb_input_grad(grgb, wr, 0.25)
    _, gb, gnw, dstyle, gz = ref.layer_tail_bwd(gy, y, style, nz, SLOPE, BS)
    _, gb_b, gnw_b, s1_b, s2_b = ref.layer_tail_bwd_bounds(gy, y, style, nz, SLOPE, BS, g_err=g_err)
    keep = np.ones((1, 1, h * w))
    keep[:, :, -4:] = 0.0
    keep = keep.reshape(1, 1, h, w)
    _outside('folded gb', BS * (gz * keep).sum(axis=(0, 2, 3)), gb, gb_b)
    _outside('folded gnw', (gz * keep * nz).sum(axis=(0, 2, 3)), gnw, gnw_b)
    _, _, s1, s2 = ref.instnorm_style_bwd(gy, y, style)
    mean, _, rstd = ref.instnorm_stats(y)
    _outside('folded s1', (gy * keep).sum(axis=(2, 3), keepdims=True), s1, s1_b)
    _outside('folded s2', (gy * (y - mean) * rstd * keep).sum(axis=(2, 3), keepdims=True), s2, s2_b)


def test_the_smallest_mistake_the_sum_bounds_reject():
    """The bounds of the per-channel and per-plane sums add every addend's worst case, so the kernels' own errors - roundings of
    either sign - fill a small share of them.  What they still reject is an error of ONE sign: the same offset on every addend
    grows like the count, as the bound does.  An offset of 4 roundings of the mean addend (4 u mean |addend|) is outside the
    bound of every plain sum; the toRGB-folded sums, whose addends are recomputed with up to 4 roundings of their products, reject
    16 u of the products' mean magnitude.  (Errors of random sign below the worst case pass: no bound on a sum can tell them
    from rounding.)"""
    ch = lambda v: v.sum(axis=(0, 2, 3))                                    # noqa: E731
    # bias_act's backward at 41x100 (act_bwd_bias_stage1 / channel_sum)
    x, b, nz, nw, _, gy = ref.tail_operands(17 + 100, 2, 3, 41, 100)
    mask = ref.bias_act(x, b, nz, nw, BS, SLOPE)[0] > 0
    gz, gb, gnw = ref.act_bwd(gy, mask, nz, SLOPE, BS)
    _, gb_b, gnw_b = ref.act_bwd_bounds(gy, mask, nz, SLOPE, BS)
    off = 4 * ref.U * np.abs(gz).mean()
    _outside('act_bwd_bias gb, offset addends', BS * ch(gz + off), gb, gb_b, margin=1.25)
    _outside('channel_sum gnw, offset addends', ch((gz + off * np.sign(nz)) * nz), gnw, gnw_b, margin=1.25)
    # blur-then-activation backward at 256x32 (BF_A)
    rng = np.random.RandomState(256 + 32)
    g, y = ref.f32(rng.standard_normal((2, 3, 256, 32))), ref.f32(rng.standard_normal((2, 3, 256, 32)))
    out, gb = ref.blur_act_bwd(g, y > 0, SLOPE, BS)
    _, gb_b = ref.blur_act_bwd_bounds(g, y > 0, SLOPE, BS)
    _outside('BF_A gb, offset addends', BS * ch(out + 4 * ref.U * np.abs(g).mean()), gb, gb_b, margin=1.25)
    # the fused tail and its toRGB-folded form at 32x32
    n, c, h, w = 2, 16, 32, 32
    x, b, nz, nw, style, gout = ref.tail_operands(c + h, n, c, h, w)
    y = ref.f32(ref.bias_act(x, b, nz, nw, BS, SLOPE)[0])
    wr, grgb = ref.f32(np.random.RandomState(c).standard_normal((3, c)) * 0.5), ref.f32(np.random.RandomState(1).standard_normal((n, 3, h, w)))
    gy, g_err = ref.torgb_input_grad(grgb, wr, 0.25)
    mean, _, rstd = ref.instnorm_stats(y)
    xhat = (y - mean) * rstd
    for what, cot, ge, off in (('tail', gout, None, 4 * ref.U * np.abs(gout).mean()),
                               ('folded', gy, g_err, 16 * ref.U * (0.25 * np.einsum('kc,nkhw->nchw', np.abs(wr), np.abs(grgb))).mean())):
        _, gb, gnw, _, gz = ref.layer_tail_bwd(cot, y, style, nz, SLOPE, BS)
        _, gb_b, gnw_b, s1_b, s2_b = ref.layer_tail_bwd_bounds(cot, y, style, nz, SLOPE, BS, g_err=ge)
        _, _, s1, s2 = ref.instnorm_style_bwd(cot, y, style)
        _outside(f'{what} s1, offset addends', (cot + off).sum(axis=(2, 3), keepdims=True), s1, s1_b, margin=1.25)
        _outside(f'{what} s2, offset addends', ((cot + off * np.sign(xhat)) * xhat).sum(axis=(2, 3), keepdims=True), s2, s2_b, margin=1.25)
        k = np.abs(rstd * (style.reshape(n, 2, c, 1, 1)[:, 0] + 1.0)) * np.where(y > 0, 1.0, SLOPE)
        _outside(f'{what} gb, offset addends', BS * ch(gz + k * off), gb, gb_b, margin=1.25)
        _outside(f'{what} gnw, offset addends', ch((gz + k * off * np.sign(nz)) * nz), gnw, gnw_b, margin=1.25)
