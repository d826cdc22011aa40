"""GPU tests of the StyleGAN layer-tail kernels (the image-space half of csrc/pointwise.hip) against the float64 restatement of
tests/tail_reference.py, one case per branch of the launchers: blur / up2 / pool2, bias_act and its backward, the channel sums,
the InstanceNorm + style kernels (statistics, forward, reduce, both apply forms, the blur and toRGB folds), the blur-fused passes
with and without statistics and sign bits.

Every case names the kernel instantiation it must reach and reads what the library launched (``_lib.launches_since``; backward
launches happen on autograd's device thread and are read there, from tensor hooks) - a case that lands on another branch fails.
``test_every_listed_instantiation_was_launched`` closes the module over ``REQUIRED``.

Every kernel is fed exact fp32 inputs (a later stage gets the earlier kernel's own output), and every bound is a per-element
count of roundings on the reference's own quantities, derived in tail_reference.py next to the formula it bounds; nothing is
normalised by a maximum.  Every check prints ``worst error / bound`` before it asserts.  tests/test_tail_host.py shows on the
CPU that each bound rejects the mistakes it is meant to catch.

Measured on the MI355X (worst error / bound over the cases of a test) - see each test's docstring."""
import ctypes

import numpy as np
import pytest
import torch

import tail_reference as ref

pytestmark = pytest.mark.gpu

EPS, SLOPE = ref.EPS, ref.SLOPE
BIAS_SCALE = float(np.float32(0.7))
SEEN = set()

# every kernel instantiation the branch map of the launchers lists (spaces removed from the demangled symbols)
REQUIRED = (
    ['blur3x3_kernel('] + [f'blur3x3_vec_kernel<{r},{b}>' for r in (2, 4, 8) for b in ('false', 'true')] +
    ['up2_kernel(', 'pool2_kernel(', 'bias_act_kernel<1>', 'bias_act_kernel<4>', 'act_bwd_kernel(', 'act_bwd_bias_stage1(',
     'channel_sum_stage1(', 'channel_sum_stage2(', 'bias_act_stats_kernel(', 'act_stats_finish_kernel('] +
    [f'blur_fused_kernel<0,{r},{s},false>' for r in (2, 4, 8) for s in ('false', 'true')] +
    [f'blur_fused_kernel<1,{r},false,{b}>' for r in (2, 4, 8) for b in ('false', 'true')] +
    [f'blur_fused_kernel<2,{r},false,{b}>' for r in (2, 4) for b in ('false', 'true')] +
    ['instnorm_stats_kernel<64>', 'instnorm_stats_kernel<256>', 'instnorm_style_fwd_kernel<1>', 'instnorm_style_fwd_kernel<4>',
     'instnorm_style_fwd_chunk_kernel<2>', 'instnorm_bwd_reduce_kernel<64>', 'instnorm_bwd_reduce_kernel<256>',
     'instnorm_bwd_apply_kernel<1>', 'instnorm_bwd_apply_kernel<4>', 'instnorm_bwd_apply_act_kernel(',
     'instnorm_bwd_act_blur_kernel<2>', 'instnorm_bwd_act_blur_kernel<4>', 'instnorm_bwd_reduce_rgb_kernel<true>',
     'instnorm_bwd_reduce_rgb_kernel<false>', 'instnorm_bwd_reduce_rgb_finish_kernel(',
     'instnorm_bwd_apply_act_rgb_kernel<true>', 'instnorm_bwd_apply_act_rgb_kernel<false>'])


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def _g(a, offset=False):
    """float64 array -> fp32 CUDA tensor; ``offset``: a contiguous view that starts 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).float()
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _n(t):
    return t.detach().double().cpu().numpy()


def _note(launches, want, what):
    syms = [s.replace(' ', '') for s, _ in launches]
    SEEN.update(syms)
    for w in want:
        assert any(w in s for s in syms), f'{what}: {w} was not launched; launched {syms}'
    return syms


class _launched(object):
    """The launches of the calling thread inside the block must show every symbol of ``want``."""

    def __init__(self, what, *want):
        self.what, self.want = what, want

    def __enter__(self):
        from gan_lab_amd import _lib
        self.c0 = _lib.launch_count()
        return self

    def __exit__(self, et, ev, tb):
        from gan_lab_amd import _lib
        if et is None:
            self.syms = _note(_lib.launches_since(self.c0), self.want, self.what)
        return False


def _backward(what, want, outs, gouts, leaves):
    """Gradients of ``leaves`` (their .grad), with the launches read on autograd's device thread: a hook on the first output
    takes the thread's counter before the first node runs, hooks on the leaves read the ring after the node that feeds them."""
    from gan_lab_amd import _lib
    rec = {'launches': []}

    def before(_):
        rec.setdefault('c0', _lib.launch_count())

    def after(_):
        rec['launches'] = _lib.launches_since(rec['c0'])

    handles = [outs[0].register_hook(before)] + [t.register_hook(after) for t in leaves]
    for t in leaves:
        t.grad = None
    torch.autograd.backward(outs, gouts)
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    assert 'c0' in rec, what
    _note(rec['launches'], want, what + ' backward')
    return [t.grad for t in leaves]


def _check(what, got, want, tol):
    """|got - want| <= tol elementwise; prints the worst ratio first and returns it."""
    got = _n(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    got = got.reshape(want.shape)
    assert np.isfinite(got).all(), what
    err, tol = np.abs(got - want), np.broadcast_to(np.asarray(tol, dtype=np.float64), want.shape)
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    print(f'tail | {what}: max error {err.max():.3e}, worst error / bound {ratio.max():.3f}')
    assert (err <= tol).all(), (what, float(err.max()), float(ratio.max()))
    return float(ratio.max())


def _with_zeros(x):
    """Plant exact zeros and -0.0 (the LeakyReLU kink) into a copy of ``x``."""
    x = x.copy()
    flat = x.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return x


# ---- blur -------------------------------------------------------------------------------------------------------------------------
BLUR_CASES = [((5, 7), 'blur3x3_kernel('), ((6, 10), 'blur3x3_kernel('), ((1, 9), 'blur3x3_kernel('), ((9, 1), 'blur3x3_kernel('),
              ((6, 8), 'blur3x3_vec_kernel<2,false>'), ((4, 4), 'blur3x3_vec_kernel<4,false>'),
              ((12, 16), 'blur3x3_vec_kernel<4,false>'), ((256, 8), 'blur3x3_vec_kernel<8,false>')]


@pytest.mark.parametrize('hw,symbol', BLUR_CASES, ids=[f'{h}x{w}' for (h, w), _ in BLUR_CASES])
def test_blur_forward_and_backward(hw, symbol):
    """3 x 8 planes (a second, ragged block at 12x16 and 256x8).  The backward is the blur of the cotangent (self-adjoint).
    Bound: ``blur_bound`` (4 roundings on blur(|x|)).  Measured: worst error / bound 0.56."""
    from gan_lab_amd import ops
    rng = np.random.RandomState(31 * hw[0] + hw[1])
    x, g = (ref.f32(rng.standard_normal((3, 8) + hw)) for _ in range(2))
    xg = _g(x).requires_grad_(True)
    with _launched(f'blur {hw}', symbol):
        y = ops.blur(xg)
    _check(f'blur {hw} y', y, ref.blur(x), ref.blur_bound(x))
    gx, = _backward(f'blur {hw}', [symbol], [y], [_g(g)], [xg])
    _check(f'blur {hw} gx', gx, ref.blur(g), ref.blur_bound(g))


def test_blur_of_an_offset_view_takes_the_scalar_kernel():
    """8x8 would take vec<4>; 4 bytes past a 16-byte boundary it must not.  Measured: 0.37."""
    from gan_lab_amd import ops
    x = ref.f32(np.random.RandomState(5).standard_normal((2, 3, 8, 8)))
    with _launched('blur offset', 'blur3x3_kernel('):
        y = ops.blur(_g(x, offset=True))
    _check('blur offset view', y, ref.blur(x), ref.blur_bound(x))
    with _launched('blur aligned', 'blur3x3_vec_kernel<4,false>'):
        ops.blur(_g(x))


BITS_CASES = [((2, 32), 2), ((6, 32), 2), ((12, 32), 4), ((256, 32), 8)]


@pytest.mark.parametrize('hw,rows', BITS_CASES, ids=[f'{h}x{w}' for (h, w), _ in BITS_CASES])
def test_blur_with_sign_bits(hw, rows):
    """The blur within ``blur_bound``; the bits exactly the packing of the kernel's own input, zeros and -0.0 included.
    Measured: 0.62."""
    from gan_lab_amd import ops
    x = _with_zeros(ref.f32(np.random.RandomState(rows + hw[0]).standard_normal((2, 3) + hw)))
    with _launched(f'blur bits {hw}', f'blur3x3_vec_kernel<{rows},true>'):
        y, bits = ops.k_blur_bits(_g(x))
    _check(f'blur bits {hw} y', y, ref.blur(x), ref.blur_bound(x))
    assert bits.dtype == torch.int32 and torch.equal(bits.cpu(), torch.from_numpy(ref.sign_bits(x)))


# ---- up2 / pool2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (8, 8)], ids=['1x1', '3x5', '8x8'])
def test_up2_and_pool2_with_a_scale(hw):
    """Forward and backward of both (each is the other's adjoint with the same scale), scale 0.3 - which only the Functions behind
    ``ops.upsample2`` / ``ops.avg_pool2`` take; the public pair follows with its own scales.  Bounds: one rounding (up2),
    three (pool2).  Measured: up2 0.92, pool2 0.68; avg_pool2 0.50, upsample2 exact."""
    from gan_lab_amd import ops
    scale = float(np.float32(0.3))
    rng = np.random.RandomState(hw[0])
    small, big = ref.f32(rng.standard_normal((2, 3) + hw)), ref.f32(rng.standard_normal((2, 3, 2 * hw[0], 2 * hw[1])))
    xs, xb = _g(small).requires_grad_(True), _g(big).requires_grad_(True)
    with _launched(f'up2 {hw}', 'up2_kernel('):
        up = ops._Up2.apply(xs, scale)
    with _launched(f'pool2 {hw}', 'pool2_kernel('):
        down = ops._Pool2.apply(xb, scale)
    _check(f'up2 {hw}', up, ref.up2(small, scale), ref.up2_bound(small, scale))
    _check(f'pool2 {hw}', down, ref.pool2(big, scale), ref.pool2_bound(big, scale))
    g, = _backward(f'up2 {hw}', ['pool2_kernel('], [up], [_g(big)], [xs])
    _check(f'up2 {hw} backward', g, ref.pool2(big, scale), ref.pool2_bound(big, scale))
    g, = _backward(f'pool2 {hw}', ['up2_kernel('], [down], [_g(small)], [xb])
    _check(f'pool2 {hw} backward', g, ref.up2(small, scale), ref.up2_bound(small, scale))
    # the public pair carries fixed scales (1 and 1 / 4): the same kernels, checked the same way
    with _launched(f'upsample2 {hw}', 'up2_kernel('):
        up = ops.upsample2(xs)
    with _launched(f'avg_pool2 {hw}', 'pool2_kernel('):
        down = ops.avg_pool2(xb)
    assert torch.equal(up.detach(), _g(ref.up2(small, 1.0)))
    _check(f'avg_pool2 {hw}', down, ref.pool2(big, 0.25), ref.pool2_bound(big, 0.25))
    g, = _backward(f'upsample2 {hw}', ['pool2_kernel('], [up], [_g(big)], [xs])
    _check(f'upsample2 {hw} backward', g, ref.pool2(big, 1.0), ref.pool2_bound(big, 1.0))
    g, = _backward(f'avg_pool2 {hw}', ['up2_kernel('], [down], [_g(small)], [xb])
    _check(f'avg_pool2 {hw} backward', g, ref.up2(small, 0.25), ref.up2_bound(small, 0.25))


# ---- bias_act, act_bwd, act_bwd_bias, channel_sum ---------------------------------------------------------------------------------
# (H, W), noise, bias, offset view, zeros planted, forward kernel
BIAS_ACT_CASES = [((5, 7), True, True, False, False, 'bias_act_kernel<1>'), ((4, 6), True, True, False, False, 'bias_act_kernel<4>'),
                  ((4, 6), False, True, False, False, 'bias_act_kernel<4>'), ((4, 6), True, False, False, False, 'bias_act_kernel<4>'),
                  ((4, 6), False, False, False, True, 'bias_act_kernel<4>'), ((5, 7), False, False, False, True, 'bias_act_kernel<1>'),
                  ((4, 6), True, True, True, False, 'bias_act_kernel<1>'), ((41, 100), True, True, False, False, 'bias_act_kernel<4>'),
                  ((41, 101), True, True, False, False, 'bias_act_kernel<1>')]


@pytest.mark.parametrize('hw,noise,bias,offset,zeros,symbol', BIAS_ACT_CASES,
                         ids=[f'{h}x{w}-{"n" if a else ""}{"b" if b else ""}{"-offset" if o else ""}{"-zeros" if z else ""}'
                              for (h, w), a, b, o, z, _ in BIAS_ACT_CASES])
def test_bias_act_and_its_backward(hw, noise, bias, offset, zeros, symbol):
    """N = 2, C = 3; 41x100 and 41x101 put N HW just above 8192, so the channel sums run two chunks with a ragged second one.
    Forward within ``bias_act_bound``; with planted zeros and no bias / noise the pre-activation IS +-0 and the output must be
    exactly zero.  Backward from the kernel's own output as mask (``act_bwd_bounds``): gz, the bias gradient (one pass with gz
    when there is a bias), the noise-weight gradient (channel_sum with the noise as second operand).
    Measured: y 0.47, gz 0.95, gb 0.43, gnw 0.39 (0.016 and 0.051 at 41x100: the bound of a sum adds the worst case of 8200
    roundings that walk at random; a dropped chunk misses it by 1e6, test_tail_host.py)."""
    from gan_lab_amd import ops
    x, b, nz, nw, _, gy = ref.tail_operands(17 + hw[1], 2, 3, hw[0], hw[1], noise=noise, bias=bias)
    if zeros:
        x = _with_zeros(x)
    what = f'bias_act {hw} noise={noise} bias={bias} offset={offset}'
    xg = _g(x, offset).requires_grad_(True)
    bg, nwg = (_g(t).requires_grad_(True) if t is not None else None for t in (b, nw))
    nzg = _g(nz, offset) if noise else None
    with _launched(what, symbol):
        y = ops.bias_act(xg, bg, nzg, nwg, BIAS_SCALE, 'lrelu', SLOPE)
    yr, z, mag = ref.bias_act(x, b, nz, nw, BIAS_SCALE, SLOPE)
    assert ref.near_kink_share(z, mag, SLOPE) < 1e-3 or zeros
    _check(what + ' y', y, yr, ref.bias_act_bound(z, mag, SLOPE))
    if zeros:
        assert bool((y.detach().reshape(-1)[::7] == 0).all()) and bool((y.detach().reshape(-1)[3::11] == 0).all())
    mask = _n(y) > 0
    want = (['act_bwd_bias_stage1(', 'channel_sum_stage2('] if bias else ['act_bwd_kernel(']) + (['channel_sum_stage1('] if noise else [])
    leaves = [t for t in (xg, bg, nwg) if t is not None]
    grads = _backward(what, want, [y], [_g(gy, offset)], leaves)      # (an offset cotangent: act_bwd_bias_stage1 goes scalar)
    gz, gb, gnw = ref.act_bwd(gy, mask, nz, SLOPE, BIAS_SCALE)
    gz_b, gb_b, gnw_b = ref.act_bwd_bounds(gy, mask, nz, SLOPE, BIAS_SCALE)
    _check(what + ' gz', grads.pop(0), gz, gz_b)
    if bias:
        _check(what + ' gb', grads.pop(0), gb, gb_b)
    if noise:
        _check(what + ' gnw', grads.pop(0), gnw, gnw_b)


@pytest.mark.parametrize('n', [1201, 1202, 1203, 1200, 3], ids=str)
def test_act_bwd_scalar_tail(n):
    """Element counts of every residue mod 4 (and fewer than 4): float4 body plus scalar tail, and the all-scalar form of an
    offset view.  The saved output holds zeros and -0.0: the slope side.  Measured: 0.95 (one rounding)."""
    from gan_lab_amd import ops
    rng = np.random.RandomState(n)
    gy, y = ref.f32(rng.standard_normal(n)), _with_zeros(ref.f32(rng.standard_normal(n)))
    want, _, _ = ref.act_bwd(gy.reshape(1, 1, 1, n), y.reshape(1, 1, 1, n) > 0, None, SLOPE, 1.0)
    bound, _, _ = ref.act_bwd_bounds(gy.reshape(1, 1, 1, n), y.reshape(1, 1, 1, n) > 0, None, SLOPE, 1.0)
    for offset in (False, True):
        with _launched(f'act_bwd {n}', 'act_bwd_kernel('):
            gz = ops.k_act_bwd(_g(gy, offset), _g(y, offset), SLOPE)
        _check(f'act_bwd n={n} offset={offset}', gz, want.reshape(n), bound.reshape(n))


@pytest.mark.parametrize('hw,offset', [((4, 6), False), ((5, 7), False), ((4, 6), True), ((41, 100), False), ((41, 101), False)],
                         ids=['4x6', '5x7', '4x6-offset', '41x100', '41x101'])
def test_channel_sum_plain_and_weighted(hw, offset):
    """float4 and scalar loads, one chunk and two with a ragged second; fp64 sums of exact products, rounded once.
    Measured: 0.90."""
    from gan_lab_amd import ops
    rng = np.random.RandomState(hw[1])
    a, b = ref.f32(rng.standard_normal((2, 3) + hw)), ref.f32(rng.standard_normal((2, 1) + hw))
    for second in (None, b):
        with _launched(f'channel_sum {hw}', 'channel_sum_stage1(', 'channel_sum_stage2('):
            got = ops.k_channel_sum(_g(a, offset), _g(second, offset) if second is not None else None, BIAS_SCALE)
        again = ops.k_channel_sum(_g(a, offset), _g(second, offset) if second is not None else None, BIAS_SCALE)
        assert torch.equal(got, again)
        want, bound = ref.channel_sum(a, second, BIAS_SCALE)
        _check(f'channel_sum {hw} weighted={second is not None} offset={offset}', got, want, bound)


# ---- InstanceNorm statistics, style forward, backward (reduce + apply) ------------------------------------------------------------
def _stats_abi(x):
    """ganlab_instnorm_stats_f32 on an (N, C, H, W) tensor -> (mean, rstd) as (N, C, 1, 1) tensors."""
    from gan_lab_amd import _lib
    n, c, h, w = x.shape
    mean, rstd = (torch.full((n, c, 1, 1), float('nan'), device='cuda') for _ in range(2))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().ganlab_instnorm_stats_f32(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(mean.data_ptr()),
                                             ctypes.c_void_p(rstd.data_ptr()), n * c, h * w, EPS, st)
    assert rc == 0
    return mean, rstd


# N, C, (H, W), offset view -> T of statistics / reduce, forward kernel, VEC of apply
IN_CASES = [(1, 3, (4, 4), False, 64, 'instnorm_style_fwd_kernel<4>', 4), (1, 5, (4, 4), False, 64, 'instnorm_style_fwd_kernel<4>', 4),
            (2, 3, (5, 7), False, 64, 'instnorm_style_fwd_kernel<1>', 1), (2, 3, (33, 33), False, 256, 'instnorm_style_fwd_kernel<1>', 1),
            (2, 3, (32, 32), False, 256, 'instnorm_style_fwd_kernel<4>', 4),
            (2, 3, (64, 128), False, 256, 'instnorm_style_fwd_chunk_kernel<2>', 4),
            (2, 3, (5, 7), True, 64, 'instnorm_style_fwd_kernel<1>', 1), (2, 3, (33, 33), True, 256, 'instnorm_style_fwd_kernel<1>', 1),
            # offset views of planes that would take the float4 / chunk forms: the pointers decide
            (2, 3, (4, 4), True, 64, 'instnorm_style_fwd_kernel<1>', 1), (2, 3, (32, 32), True, 256, 'instnorm_style_fwd_kernel<1>', 1),
            (2, 3, (64, 128), True, 256, 'instnorm_style_fwd_kernel<1>', 1)]


def _instnorm_case(what, x, style, gy, offset, t, fwd, vec):
    from gan_lab_amd import ops
    xg = _g(x, offset).requires_grad_(True)
    sg = _g(style).requires_grad_(True) if style is not None else None
    with _launched(what + ' stats', f'instnorm_stats_kernel<{t}>'):
        mean, rstd = _stats_abi(xg.detach())
    m, _, r = ref.instnorm_stats(x)
    m_b, r_b = ref.stats_bounds(x)
    _check(what + ' mean', mean, m, m_b)
    _check(what + ' rstd', rstd, r, r_b)
    with _launched(what, f'instnorm_stats_kernel<{t}>', fwd):
        y = ops.instnorm_style(xg, sg, EPS)
    _check(what + ' y', y, ref.instnorm_style(x, style), ref.instnorm_style_bound(x, style))
    leaves = [xg] + ([sg] if sg is not None else [])
    grads = _backward(what, [f'instnorm_bwd_reduce_kernel<{t}>', f'instnorm_bwd_apply_kernel<{vec}>'], [y], [_g(gy, offset)], leaves)
    gx, dstyle, _, _ = ref.instnorm_style_bwd(gy, x, style)
    gx_b, s1_b, s2_b = ref.instnorm_bwd_bounds(gy, x, style)
    _check(what + ' gx', grads[0], gx, gx_b)
    if style is not None:
        n, c = x.shape[:2]
        _check(what + ' dstyle', grads[1], dstyle, np.concatenate([s2_b.reshape(n, c), s1_b.reshape(n, c)], axis=1))
    return (mean, rstd, y.detach()) + tuple(grads)


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('n,c,hw,offset,t,fwd,vec', IN_CASES,
                         ids=[f'{n}x{c}x{h}x{w}{"-offset" if o else ""}' for n, c, (h, w), o, _, _, _ in IN_CASES])
def test_instnorm_style_against_float64(n, c, hw, offset, t, fwd, vec, regime):
    """Statistics through the C ABI (``stats_bounds``: half an ulp of the stored value plus the fp64 cancellation), then
    ``ops.instnorm_style`` forward (``instnorm_style_bound``) and backward (``instnorm_bwd_bounds``, the all-fp32 apply kernel),
    with a style and without, in the three operand regimes.  3 and 5 planes of 4x4 leave the four-planes-per-block kernels a
    ragged block.  Two runs give the same bits.
    Measured: mean 1.00, rstd 0.95, y 1.00, gx 0.93, dstyle 1.00 (largest over all cases and regimes; 1.00 is a plane sum that
    lands half an ulp from an fp32 number, and on a near-constant plane the output that inherits that mean)."""
    rng = np.random.RandomState(n * 100 + c * 10 + hw[1])
    x, _ = ref.regime_plane(rng, (n, c) + hw, regime)
    style, gy = ref.f32(0.5 * rng.standard_normal((n, 2 * c))), ref.f32(rng.standard_normal((n, c) + hw))
    for st in (style, None):
        what = f'instnorm {n}x{c}x{hw[0]}x{hw[1]} {regime} style={st is not None} offset={offset}'
        a = _instnorm_case(what, x, st, gy, offset, t, fwd, vec)
        b = _instnorm_case(what + ' again', x, st, gy, offset, t, fwd, vec)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), what


@pytest.mark.parametrize('hw', [(4, 4), (5, 7), (32, 32), (64, 128)], ids=['4x4', '5x7', '32x32', '64x128'])
def test_constant_planes_normalise_to_exactly_zero(hw):
    """A constant plane has variance 0: the statistics are exact (mean the constant, rstd 1 / sqrt(eps)), the plain
    normalisation is exactly 0, and every gradient is finite - through ``instnorm_style`` and through ``layer_tail``."""
    from gan_lab_amd import ops
    n, c = 2, 3
    vals = ref.f32(np.array([1.5, -0.37, 3.0, 1e-3, 7.25, -2.0])).reshape(n, c, 1, 1)
    x = np.broadcast_to(vals, (n, c) + hw).copy()
    gy = ref.f32(np.random.RandomState(3).standard_normal((n, c) + hw))
    xg = _g(x).requires_grad_(True)
    mean, rstd = _stats_abi(xg.detach())
    assert np.array_equal(_n(mean), vals)
    _check(f'const {hw} rstd', rstd, np.full((n, c, 1, 1), 1.0 / np.sqrt(EPS)), ref.half_ulp(1.0 / np.sqrt(EPS)))
    y = ops.instnorm_style(xg, None, EPS)
    assert bool((y == 0).all())
    gx, = torch.autograd.grad(y, xg, _g(gy))
    assert bool(torch.isfinite(gx).all())
    bias = torch.zeros(c, device='cuda', requires_grad=True)
    out = ops.layer_tail(xg, bias, None, None, None, 1.0, 'lrelu', SLOPE, False, EPS)
    assert bool((out == 0).all())
    gx, gb = torch.autograd.grad(out, (xg, bias), _g(gy))
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gb).all())


# ---- the layer tail ---------------------------------------------------------------------------------------------------------------
def _rows(h, floor8):
    return 8 if (h % 8 == 0 and h >= floor8) else (4 if h % 4 == 0 else 2)


TAIL_SHAPES = ref.TAIL_SHAPES


def _tail_forward_symbols(hw, with_blur, stats):
    h, w = hw
    fusable, vec = h % 2 == 0 and w % 4 == 0, (h * w) % 4 == 0
    if with_blur and fusable:
        return [f'blur_fused_kernel<0,{_rows(h, 512)},{"true" if stats else "false"},false>'] + (['act_stats_finish_kernel('] if stats else [])
    first = ['blur3x3_kernel('] if with_blur else []
    if stats:
        return first + ['bias_act_stats_kernel(', 'act_stats_finish_kernel(']
    return first + [f'bias_act_kernel<{4 if vec else 1}>']


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('with_blur', [False, True], ids=['plain', 'blur'])
@pytest.mark.parametrize('hw', TAIL_SHAPES, ids=[f'{h}x{w}' for h, w in TAIL_SHAPES])
def test_bias_act_with_statistics_then_instnorm_style(hw, with_blur, regime):
    """``ops.bias_act(..., stats_eps)`` -> ``ops.instnorm_style(stats=...)``, stage by stage.  32x32: one chunk, rows 4; 36x228:
    2052 float4 per plane, two chunks with a ragged second (772); 6x172: rows 2; 512x8: BF_FWD rows 8; 16x16: below
    STATS_MIN_PLANE (no fused statistics); 5x7: nothing fuses.  Stages: y (``bias_act_bound``, with ``blur_bound`` in front when
    blurred), the fused statistics of the kernel's own y (``stats_bounds``), out and the InstanceNorm gradients from that y, and
    the backward of the first stage from its own output as mask - ``act_bwd_bounds`` or, blurred, ``act_bwd_blur_bounds``
    (blur_fused_kernel<BF_AT>; 36x228 runs it in two chunks - the only blurred pass that does: with statistics the forward cuts
    each plane on its own, 513 strips at 36x228, one chunk, and more than 1024 strips per plane lie beyond the sizes of this module).  Each reduction-bearing stage runs twice: equal bits.
    Measured: y 0.50, mean 0.95, rstd 0.99, out 1.00, d/dy 0.99, dstyle 1.00, gx 0.95, gb 0.99, gnw 0.95."""
    from gan_lab_amd import ops
    h, w = hw
    n, c = 2, 3
    x, b, nz, nw, style, gout = ref.tail_operands(ref.tail_seed(h, w), n, c, h, w, regime)
    what = f'tail stages {h}x{w} blur={with_blur} {regime}'
    fused_stats = h * w >= ops.STATS_MIN_PLANE and (h * w) % 4 == 0
    xg, bg, nwg = (_g(t).requires_grad_(True) for t in (x, b, nw))

    def forward():
        with _launched(what, *_tail_forward_symbols(hw, with_blur, fused_stats)):
            return ops.bias_act(xg, bg, _g(nz), nwg, BIAS_SCALE, 'lrelu', SLOPE, with_blur, stats_eps=EPS)
    y, stats = forward()
    y2, stats2 = forward()
    assert torch.equal(y, y2) and (stats is None) == (not fused_stats)
    xin = ref.blur(x) if with_blur else x
    yr, z, mag = ref.bias_act(xin, b, nz, nw, BIAS_SCALE, SLOPE)
    assert ref.near_kink_share(z, mag, SLOPE) < 1e-3
    _check(what + ' y', y, yr, ref.bias_act_bound(z, mag, SLOPE, pre=ref.blur_bound(x) if with_blur else None))
    ya = _n(y)
    if fused_stats:
        assert torch.equal(stats[0], stats2[0]) and torch.equal(stats[1], stats2[1])
        m, _, r = ref.instnorm_stats(ya)
        m_b, r_b = ref.stats_bounds(ya)
        _check(what + ' mean', stats[0], m, m_b)
        _check(what + ' rstd', stats[1], r, r_b)
    # second stage on the first one's output as a leaf
    yl, sg = y.detach().clone().requires_grad_(True), _g(style).requires_grad_(True)
    out = ops.instnorm_style(yl, sg, EPS, stats)
    _check(what + ' out', out, ref.instnorm_style(ya, style), ref.instnorm_style_bound(ya, style))
    t = 256 if h * w >= 1024 else 64
    gyl, gs = _backward(what + ' norm', [f'instnorm_bwd_reduce_kernel<{t}>'], [out], [_g(gout)], [yl, sg])
    gx, dstyle, _, _ = ref.instnorm_style_bwd(gout, ya, style)
    gx_b, s1_b, s2_b = ref.instnorm_bwd_bounds(gout, ya, style)
    _check(what + ' d/dy', gyl, gx, gx_b)
    _check(what + ' dstyle', gs, dstyle, np.concatenate([s2_b.reshape(n, c), s1_b.reshape(n, c)], axis=1))
    # backward of the first stage
    fusable = h % 2 == 0 and w % 4 == 0
    want = [f'blur_fused_kernel<2,{_rows(h, 1 << 30)},false,false>'] if (with_blur and fusable) else ['act_bwd_bias_stage1(', 'channel_sum_stage1(']
    grads = _backward(what + ' act', want, [y], [_g(gout)], [xg, bg, nwg])
    again = [g.clone() for g in _backward(what + ' act', want, [forward()[0]], [_g(gout)], [xg, bg, nwg])]
    assert all(torch.equal(p, q) for p, q in zip(grads, again))
    mask = ya > 0
    if with_blur:
        wants, bounds = ref.act_bwd_blur(gout, mask, nz, SLOPE, BIAS_SCALE), ref.act_bwd_blur_bounds(gout, mask, nz, SLOPE, BIAS_SCALE)
    else:
        wants, bounds = ref.act_bwd(gout, mask, nz, SLOPE, BIAS_SCALE), ref.act_bwd_bounds(gout, mask, nz, SLOPE, BIAS_SCALE)
    for nm, got, wv, bv in zip(('gx', 'gb', 'gnw'), grads, wants, bounds):
        _check(f'{what} {nm}', got, wv, bv)


def _composed_tail_bounds(gout, ya, style, nz, with_blur):
    """The fallback of ``layer_tail`` (small or ragged planes) chains the fp32 kernels: the all-fp32 InstanceNorm apply
    (``instnorm_bwd_bounds``), the slope product on top (u |gz|), the sums over the fp32 gz, then the blur's 4 roundings."""
    gin_b, s1_b, s2_b = ref.instnorm_bwd_bounds(gout, ya, style)
    _, gb, gnw, _, gz = ref.layer_tail_bwd(gout, ya, style, nz, SLOPE, BIAS_SCALE)
    gz_b = np.where(ya > 0, 1.0, SLOPE) * gin_b + ref.U * np.abs(gz)
    ch = lambda v: v.sum(axis=(0, 2, 3))                                    # noqa: E731
    gb_b = ref.half_ulp(gb) + BIAS_SCALE * (ch(gz_b) + ref.L_SUM * ref.D * ch(np.abs(gz)))
    gnw_b = ref.half_ulp(gnw) + ch(gz_b * np.abs(nz)) + ref.L_SUM * ref.D * ch(np.abs(gz * nz))
    gx_b = ref.blur(gz_b) + ref.gamma(4) * ref.blur(np.abs(gz)) if with_blur else gz_b
    return gx_b, gb_b, gnw_b, s1_b, s2_b


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('with_blur', [False, True], ids=['plain', 'blur'])
@pytest.mark.parametrize('hw', TAIL_SHAPES, ids=[f'{h}x{w}' for h, w in TAIL_SHAPES])
def test_layer_tail_as_one_node(hw, with_blur, regime):
    """``ops.layer_tail``: the output and every gradient (x, bias, noise weight, style) against float64, from the activated tensor
    the node keeps - read through ``ops.layer_tail_deferred``, whose materialised output must be the node's, bit for bit.  Large
    planes: bias_act_stats / blur_fused<BF_FWD, statistics> forward, instnorm_bwd_apply_act_kernel (36x228: two chunks, the second
    ragged) or instnorm_bwd_act_blur_kernel<4 / 2> backward (one chunk per plane at every size here: a second one needs more than
    1024 four-column strips in a plane), within ``layer_tail_bwd_bounds`` (fp64 element formula, one
    rounding); 16x16 and 5x7 compose the separate kernels (``_composed_tail_bounds``).  Two runs: equal bits.
    Measured: out 1.00, gx 0.99, gb 0.66, gnw 0.35, dstyle 1.00."""
    from gan_lab_amd import ops
    h, w = hw
    n, c = 2, 3
    x, b, nz, nw, style, gout = ref.tail_operands(ref.tail_seed(h, w), n, c, h, w, regime)
    what = f'layer_tail {h}x{w} blur={with_blur} {regime}'
    fused = h * w >= ops.STATS_MIN_PLANE and (h * w) % 4 == 0 and (not with_blur or (h % 2 == 0 and w % 4 == 0))
    leaves = [_g(t).requires_grad_(True) for t in (x, b, nw, style)]
    xg, bg, nwg, sg = leaves
    t = 256 if h * w >= 1024 else 64
    fwd = ('instnorm_style_fwd_kernel<4>' if (h * w) % 4 == 0 else 'instnorm_style_fwd_kernel<1>')

    def run():
        with _launched(what, fwd, *(_tail_forward_symbols(hw, with_blur, True) if fused else [f'instnorm_stats_kernel<{t}>'])):
            out = ops.layer_tail(xg, bg, _g(nz), nwg, sg, BIAS_SCALE, 'lrelu', SLOPE, with_blur, EPS)
        if fused:
            want = [f'instnorm_bwd_reduce_kernel<{t}>', 'channel_sum_stage2(',
                    f'instnorm_bwd_act_blur_kernel<{4 if h % 4 == 0 else 2}>' if with_blur else 'instnorm_bwd_apply_act_kernel(']
        else:
            want = [f'instnorm_bwd_reduce_kernel<{t}>', f'instnorm_bwd_apply_kernel<{4 if (h * w) % 4 == 0 else 1}>']
        return [out.detach()] + [g.clone() for g in _backward(what, want, [out], [_g(gout)], leaves)]
    got, again = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(got, again)), what
    if fused:       # the same first kernel as the node's
        d = ops.layer_tail_deferred(xg, bg, _g(nz), nwg, sg, BIAS_SCALE, 'lrelu', SLOPE, with_blur, EPS)
        ya = _n(d.a)
        assert torch.equal(ops.materialize(d).detach(), got[0]), what
    else:           # the call the fallback makes
        ya = _n(ops.bias_act(xg, bg, _g(nz), nwg, BIAS_SCALE, 'lrelu', SLOPE, with_blur))
    _check(what + ' out', got[0], ref.instnorm_style(ya, style), ref.instnorm_style_bound(ya, style))
    gx, gb, gnw, dstyle, _ = ref.layer_tail_bwd(gout, ya, style, nz, SLOPE, BIAS_SCALE, with_blur=with_blur)
    if fused:
        gx_b, gb_b, gnw_b, s1_b, s2_b = ref.layer_tail_bwd_bounds(gout, ya, style, nz, SLOPE, BIAS_SCALE, with_blur=with_blur)
    else:
        gx_b, gb_b, gnw_b, s1_b, s2_b = _composed_tail_bounds(gout, ya, style, nz, with_blur)
    _check(what + ' gx', got[1], gx, gx_b)
    _check(what + ' gb', got[2], gb, gb_b)
    _check(what + ' gnw', got[3], gnw, gnw_b)
    _check(what + ' dstyle', got[4], dstyle, np.concatenate([s2_b.reshape(n, c), s1_b.reshape(n, c)], axis=1))


def test_blur_bias_act_without_statistics_in_two_chunks():
    """36x228 with N = 2: 1026 four-column strips, so the statistics-free blur_fused_kernel<BF_FWD, 4> runs two chunks; 512x8:
    rows 8; 6x172: rows 2.  Measured: 0.38."""
    from gan_lab_amd import ops
    for h, w in ((36, 228), (512, 8), (6, 172)):
        x, b, nz, nw, _, _ = ref.tail_operands(h + w, 2, 3, h, w)
        with _launched(f'blur_bias_act {h}x{w}', f'blur_fused_kernel<0,{_rows(h, 512)},false,false>'):
            y = ops.bias_act(_g(x), _g(b), _g(nz), _g(nw), BIAS_SCALE, 'lrelu', SLOPE, True)
        yr, z, mag = ref.bias_act(ref.blur(x), b, nz, nw, BIAS_SCALE, SLOPE)
        _check(f'blur_bias_act {h}x{w}', y, yr, ref.bias_act_bound(z, mag, SLOPE, pre=ref.blur_bound(x)))


# ---- blur fused with the activation backward, float masks and sign bits -----------------------------------------------------------
FUSED_BWD_CASES = [((6, 8), False), ((12, 16), False), ((256, 8), False), ((36, 228), False), ((6, 32), True), ((12, 32), True),
                   ((256, 32), True)]


@pytest.mark.parametrize('hw,bits', FUSED_BWD_CASES, ids=[f'{h}x{w}{"-bits" if b else ""}' for (h, w), b in FUSED_BWD_CASES])
def test_blur_then_activation_backward_and_its_adjoint(hw, bits):
    """The critic side: out = lrelu'(y) blur(g) with the bias gradient (blur_fused_kernel<BF_A>: rows 2 / 4, and 8 from H = 256)
    and its adjoint out = blur(lrelu'(y) g) with bias and noise-weight gradients (BF_AT: rows 2 / 4 only), with the activation
    as a float tensor and as sign bits (taken from ``k_blur_bits``: exact, checked above).  y holds zeros and -0.0.
    Bounds: ``blur_act_bwd_bounds`` / ``act_bwd_blur_bounds``.  Two runs: equal bits.
    Measured: BF_A out 0.52, gb 0.04; BF_AT out 0.61, gb 0.13, gnw 0.12 (the sums: worst case of every addend's roundings against
    their random walk; a mask word out of place misses the gb bound by 1e3, test_tail_host.py)."""
    from gan_lab_amd import ops
    h, w = hw
    rng = np.random.RandomState(h + w)
    g, nz = ref.f32(rng.standard_normal((2, 3, h, w))), ref.f32(rng.standard_normal((2, 1, h, w)))
    y = _with_zeros(ref.f32(rng.standard_normal((2, 3, h, w))))
    mask = y > 0
    yg = ops.k_blur_bits(_g(y))[1] if bits else _g(y)
    if bits:
        assert np.array_equal(ref.mask_from_bits(yg.cpu().numpy(), y.shape), mask)
    tag = 'true' if bits else 'false'
    what = f'fused backward {h}x{w} bits={bits}'

    def run_a():
        with _launched(what, f'blur_fused_kernel<1,{_rows(h, 256)},false,{tag}>', 'channel_sum_stage2('):
            return ops.k_blur_act_bwd(_g(g), yg, SLOPE, BIAS_SCALE, True)

    def run_at():
        with _launched(what, f'blur_fused_kernel<2,{_rows(h, 1 << 30)},false,{tag}>', 'channel_sum_stage2('):
            return ops.k_act_bwd_blur(_g(g), yg, _g(nz), SLOPE, BIAS_SCALE, True, True)
    for run, wants, bounds, names in (
            (run_a, ref.blur_act_bwd(g, mask, SLOPE, BIAS_SCALE), ref.blur_act_bwd_bounds(g, mask, SLOPE, BIAS_SCALE), ('out', 'gb')),
            (run_at, ref.act_bwd_blur(g, mask, nz, SLOPE, BIAS_SCALE), ref.act_bwd_blur_bounds(g, mask, nz, SLOPE, BIAS_SCALE),
             ('out', 'gb', 'gnw'))):
        got, again = run(), run()
        assert all(torch.equal(p, q) for p, q in zip(got, again)), what
        for nm, gv, wv, bv in zip(names, got, wants, bounds):
            _check(f'{what} {run.__name__[4:]} {nm}', gv, wv, bv)


# ---- the toRGB-folded backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('c,hw,folded', [(16, (32, 32), True), (12, (32, 32), True), (16, (16, 32), False)],
                         ids=['16ch-32x32', '12ch-32x32', '16ch-16x32'])
def test_torgb_folded_backward(c, hw, folded, regime):
    """``layer_tail_deferred`` -> ``torgb_mod`` with 3 image channels: where the fold applies (HW >= 1024; the compile-time form at
    C = 16, the run-time form at C = 12) the tail's backward recomputes gy = scale W^T grgb in fp32 inside its two passes
    (``torgb_input_grad``: each product's own count of roundings, 4 / 4 / 3, handed to ``layer_tail_bwd_bounds`` as ``g_err``); at HW = 512 the
    1x1 input gradient is written by the conv kernel (the same bound) and the plain kernels run.  The reference is the 1x1 conv's
    input gradient restated in float64, then the plain tail formulas on the kernel's own activated tensor.
    Measured (largest / smallest over cases and regimes): gx 0.91 / 0.32, gb 0.49 / 0.002, gnw 0.32 / 0.004, dstyle 0.93 / 0.016 -
    the large ones on the near-constant planes, where the stored mean's rounding fills the bound; the small ones at unit normal,
    where the sums carry the recomputation's worst case once per element (what they still reject: test_tail_host.py)."""
    from gan_lab_amd import _lib, ops
    h, w = hw
    n = 2
    x, b, nz, nw, style, _ = ref.tail_operands(c + h, n, c, h, w, regime)
    _, z, mag = ref.bias_act(x, b, nz, nw, BIAS_SCALE, SLOPE)
    assert ref.near_kink_share(z, mag, SLOPE) < 1e-3
    rng = np.random.RandomState(c)
    wrgb, brgb, grgb = ref.f32(rng.standard_normal((3, c)) * 0.5), ref.f32(rng.standard_normal(3)), ref.f32(rng.standard_normal((n, 3, h, w)))
    scale = float(np.float32(1.0 / np.sqrt(c)))
    assert bool(_lib.lib().ganlab_instnorm_bwd_rgb_supported(n, c, 3, h * w)) == folded
    leaves = [_g(t).requires_grad_(True) for t in (x, b, nw, style)]
    xg, bg, nwg, sg = leaves
    what = f'torgb fold C={c} {h}x{w} {regime}'

    def run():
        d = ops.layer_tail_deferred(xg, bg, _g(nz), nwg, sg, BIAS_SCALE, 'lrelu', SLOPE, False, EPS)
        assert ops.torgb_mod_ok(d, _g(wrgb.reshape(3, c, 1, 1)))
        rgb = ops.torgb_mod(d, _g(wrgb.reshape(3, c, 1, 1)), _g(brgb), scale, 1.0)
        tag = 'true' if c == 16 else 'false'
        want = [f'instnorm_bwd_reduce_rgb_kernel<{tag}>', 'instnorm_bwd_reduce_rgb_finish_kernel(',
                f'instnorm_bwd_apply_act_rgb_kernel<{tag}>', 'channel_sum_stage2('] if folded else \
            ['instnorm_bwd_reduce_kernel<64>', 'instnorm_bwd_apply_act_kernel(', 'channel_sum_stage2(']
        return [d.a.detach()] + [g.clone() for g in _backward(what, want, [rgb], [_g(grgb)], leaves)]
    got, again = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(got, again)), what
    ya = _n(got[0])
    gy, g_err = ref.torgb_input_grad(grgb, wrgb, scale)
    gx, gb, gnw, dstyle, _ = ref.layer_tail_bwd(gy, ya, style, nz, SLOPE, BIAS_SCALE)
    gx_b, gb_b, gnw_b, s1_b, s2_b = ref.layer_tail_bwd_bounds(gy, ya, style, nz, SLOPE, BIAS_SCALE, g_err=g_err)
    _check(what + ' gx', got[1], gx, gx_b)
    _check(what + ' gb', got[2], gb, gb_b)
    _check(what + ' gnw', got[3], gnw, gnw_b)
    _check(what + ' dstyle', got[4], dstyle, np.concatenate([s2_b.reshape(n, c), s1_b.reshape(n, c)], axis=1))


# ---- offset views in front of the kernels that only have float4 forms ---------------------------------------------------------------
@pytest.mark.parametrize('with_blur', [False, True], ids=['plain', 'blur'])
def test_offset_views_through_the_float4_only_kernels(with_blur):
    """x, the noise and the cotangent as contiguous views 4 bytes past a 16-byte boundary, at 32x32 where every fused form
    applies: bias_act with statistics, the layer tail forward and backward, the blur-fused backward passes and the blur with sign
    bits have no scalar form, so the Python side hands them aligned copies - the same kernels run and give the bits of the aligned
    run (whose values the tests above hold to float64)."""
    from gan_lab_amd import ops
    n, c, h, w = 2, 3, 32, 32
    x, b, nz, nw, style, gout = ref.tail_operands(ref.tail_seed(h, w), n, c, h, w)
    stats_kernel = 'blur_fused_kernel<0,4,true,false>' if with_blur else 'bias_act_stats_kernel('
    bwd_kernel = 'instnorm_bwd_act_blur_kernel<4>' if with_blur else 'instnorm_bwd_apply_act_kernel('

    def tail(offset):
        leaves = [_g(x, offset).requires_grad_(True)] + [_g(t).requires_grad_(True) for t in (b, nw, style)]
        with _launched('offset tail', stats_kernel, 'instnorm_style_fwd_kernel<4>'):
            out = ops.layer_tail(leaves[0], leaves[1], _g(nz, offset), leaves[2], leaves[3], BIAS_SCALE, 'lrelu', SLOPE, with_blur, EPS)
        with _launched('offset bias_act', stats_kernel):
            y, stats = ops.bias_act(leaves[0], leaves[1], _g(nz, offset), leaves[2], BIAS_SCALE, 'lrelu', SLOPE, with_blur, stats_eps=EPS)
        grads = _backward('offset tail', ['instnorm_bwd_reduce_kernel<256>', bwd_kernel], [out], [_g(gout, offset)], leaves)
        return [out.detach(), y.detach(), stats[0], stats[1]] + [g.clone() for g in grads]
    assert all(torch.equal(p, q) for p, q in zip(tail(True), tail(False)))
    if with_blur:
        ya = _with_zeros(x)

        def fused(offset):
            with _launched('offset bits', 'blur3x3_vec_kernel<4,true>'):
                yb, bits = ops.k_blur_bits(_g(ya, offset))
            with _launched('offset BF_A', 'blur_fused_kernel<1,4,false,false>'):
                a = ops.k_blur_act_bwd(_g(gout, offset), _g(ya, offset), SLOPE, BIAS_SCALE, True)
            with _launched('offset BF_AT', 'blur_fused_kernel<2,4,false,false>'):
                at = ops.k_act_bwd_blur(_g(gout, offset), _g(ya, offset), _g(nz, offset), SLOPE, BIAS_SCALE, True, True)
            with _launched('offset BF_AT bits', 'blur_fused_kernel<2,4,false,true>'):
                atb = ops.k_act_bwd_blur(_g(gout, offset), bits, _g(nz, offset), SLOPE, BIAS_SCALE, True, True)
            return [yb, bits] + list(a) + list(at) + list(atb)
        assert all(torch.equal(p, q) for p, q in zip(fused(True), fused(False)))


# ---- the closing census ---------------------------------------------------------------------------------------------------------------
def test_every_listed_instantiation_was_launched():
    """A condition on this module as a whole: every kernel instantiation of the launchers' branch map was named by a launch
    assertion and did run.  It reads what the tests above recorded in this process, so run it with the whole module, in file order
    and in one process (``pytest -m gpu tests/test_gpu_tail.py``): alone, under ``-k`` or spread over workers it reports the
    instantiations whose tests it did not see."""
    missing = [k for k in REQUIRED if not any(k in s for s in SEEN)]
    assert not missing, missing
