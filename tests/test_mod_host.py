"""CPU tests of tests/mod_reference.py: each float64 restatement of the modulated toRGB / deferred-InstanceNorm kernels against
torch autograd in float64 (1e-12), each bound against the mistakes it exists for (a perturbed reference must miss the bound by
a wide factor), and each plan restatement at the edge its GPU case names.  No GPU, no gan_lab_amd import."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mod_reference as M
import tail_reference as tail

SCALE, BIAS_SCALE = float(np.float32(0.25)), float(np.float32(0.7))
WIDE = 100.0


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _worst(got, want, bound):
    err = np.abs(got - want)
    return float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())


def _chain(seed, n, cin, cout, h, w, with_style=True, with_bias=True):
    """The restated chain on a plane with mean 0.5 and unit spread, and the same thing by definition under autograd."""
    rng = np.random.RandomState(seed)
    a = tail.f32(0.5 + rng.standard_normal((n, cin, h, w)))
    style = tail.f32(0.5 * rng.standard_normal((n, 2 * cin))) if with_style else None
    wt, bias = tail.f32(rng.standard_normal((cout, cin))), (tail.f32(rng.standard_normal(cout)) if with_bias else None)
    gy = tail.f32(rng.standard_normal((n, cout, h, w)))
    b, mean, rstd = M.materialised(a, style)
    s, t = M.in_affine(mean, rstd, style)
    weff, beff = M.torgb_prep(wt, bias, s, t, SCALE, BIAS_SCALE)
    img = M.torgb_fwd(a.reshape(n, cin, h * w), weff, beff, cout).reshape(n, cout, h, w)
    out = M.torgb_cross(a.reshape(n, cin, h * w), gy.reshape(n, cout, h * w))
    gw, gb = M.torgb_wgrad(out, s, t, SCALE, BIAS_SCALE, cout)
    # the definition: F.conv2d of the materialised tensor, gradients by autograd
    wd = torch.from_numpy(wt).reshape(cout, cin, 1, 1).requires_grad_(True)
    bd = torch.from_numpy(bias if with_bias else np.zeros(cout)).requires_grad_(True)
    img_d = F.conv2d(torch.from_numpy(b), wd * SCALE) + (bd * BIAS_SCALE).view(1, -1, 1, 1)
    gw_d, gb_d = torch.autograd.grad(img_d, (wd, bd), torch.from_numpy(gy))
    return dict(img=img, gw=gw, gb=gb, out=out, weff=weff, beff=beff, s=s, t=t, b=b), \
        dict(img=img_d.detach().numpy(), gw=gw_d.numpy().reshape(cout, cin), gb=gb_d.numpy())


@pytest.mark.parametrize('n,cin,cout,hw,style,bias', [(1, 1, 1, (2, 2), True, True), (3, 5, 3, (6, 10), True, True),
                                                      (2, 16, 4, (8, 8), True, False), (2, 16, 3, (8, 8), False, True)],
                         ids=['1to1', '5to3', '16to4-nobias', '16to3-nostyle'])
def test_restatements_equal_autograd_in_float64(n, cin, cout, hw, style, bias):
    """in_affine -> prep -> forward is F.conv2d of the materialised tensor; the cross-sum algebra gives autograd's weight and
    bias gradients; padded lanes and unused cross slots are exactly zero.  (Unit-spread planes: on the near-constant regimes the
    deferred FORM cancels in float64 too - which is why the GPU tests take the materialised definition as their reference.)"""
    r, d = _chain(n * 7 + cin, n, cin, cout, hw[0], hw[1], style, bias)
    for k in ('img', 'gw', 'gb'):
        assert _rel(r[k], d[k]) <= 1e-12, k
    assert not r['weff'][:, :, cout:].any() and not r['beff'][:, cout:].any()
    cross = r['out'][:, :64].reshape(n, 16, 4)
    assert not cross[:, cin:].any() and not cross[:, :, cout:].any() and not r['out'][:, 64 + cout:].any()
    part = M.torgb_cross_partials(tail.f32(np.random.RandomState(1).standard_normal((n, cin, 8))),
                                  tail.f32(np.random.RandomState(2).standard_normal((n, cout, 8))))
    assert part.shape == (n, 1, 68)


def test_in_affine_without_style_is_the_plain_normalisation():
    mean, rstd = tail.f32(np.random.RandomState(0).standard_normal((2, 3))), tail.f32(np.random.RandomState(1).uniform(0.5, 2, (2, 3)))
    s, t = M.in_affine(mean, rstd, None)
    assert np.array_equal(s, rstd) and np.array_equal(t, -mean * rstd)
    assert np.array_equal(M.in_affine_s_bits(rstd, None).astype(np.float64), rstd)


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def test_plans_reach_the_edges_their_cases_name():
    p = M.fwd_plan(1, 4)
    assert (p['blocks'], p['trips'], p['last_trip_items']) == (1, 1, 1)
    p = M.fwd_plan(1, 1028)
    assert (p['blocks'], p['trips']) == (2, 1) and 1028 // 4 - 256 == 1
    p = M.fwd_plan(2, 4 * 128 * 256 + 20)
    assert p['capped'] and p['blocks'] == 128 and p['trips'] == 2 and p['last_trip_items'] == 5       # 129 blocks asked, 128 given
    assert p['launches'] == [('rm_torgb_fwd_kernel', 256)]
    assert M.fwd_plan(1, 4 * 129 * 256)['capped'] and M.fwd_plan(1, 4 * 129 * 256)['blocks'] == 128
    assert M.cross_plan(1, 4)['blocks'] == 1
    assert M.cross_plan(2, 4 * 4097)['launches'] == [('rm_torgb_cross_kernel', 4), ('rm_torgb_cross_finish_kernel', 2)]
    p = M.cross_plan(1, 4 * (2 * 4096 + 1))
    assert p['blocks'] == 3 and p['odd_tail']
    p = M.cross_plan(1, 4 * (64 * 4096 + 7))
    assert p['capped'] and p['blocks'] == 64 and p['trips'] == 17 and p['last_trip_items'] == 7
    assert M.cross_counts(4 * (64 * 4096 + 7)) == (3 + 17 + 8 + 33, 2 + 17 + 8 + 33)
    assert M.cross_workspace_bytes(3) == 3 * 64 * 68 * 4
    assert [M.in_affine_plan(1, k)['launches'][0][1] for k in (1, 255, 256, 257, 513)] == [1, 1, 1, 2, 3]
    assert M.in_affine_plan(1, 513)['last_block_items'] == 1
    assert M.prep_plan(3)['launches'] == [('rm_torgb_prep_kernel', 3)] and M.wgrad_plan()['launches'] == [('rm_torgb_wgrad_kernel', 1)]


# ---- the bounds reject the mistakes they exist for ------------------------------------------------------------------------------------
def test_forward_bound_rejects_a_dropped_second_trip():
    """Pixels past 128 * 256 * 4 left stale (zero): the bound there is a few u of values of order 1."""
    hw = 4 * 128 * 256 + 20
    x, w, b, s, t, _ = M.torgb_operands(3, 2, 5, 3, hw)
    weff, beff = M.torgb_prep(w, b, s, t, SCALE, BIAS_SCALE)
    y, bound = M.torgb_fwd(x, weff, beff, 3), M.torgb_fwd_bound(x, weff, beff, 3)
    assert _worst(y, y, bound) == 0.0
    bad = y.copy()
    bad[:, :, 128 * 256 * 4:] = 0.0
    assert _worst(bad, y, bound) > 1e4
    assert float(bound.max()) < 1e-5 and float(np.abs(y).mean()) > 0.1       # |y| of order 1: the bound does not degenerate


@pytest.mark.parametrize('hw4,drop', [(4097, 1), (2 * 4096 + 1, 2), (2 * 4096 + 1, 0)], ids=['second-of-2', 'odd-last-of-3', 'first-of-3'])
def test_cross_bound_rejects_a_block_left_out_of_the_finish(hw4, drop):
    """The odd last block of three holds ONE float4 item: four products of order 1 against a bound of gamma(16) sum |x gy| over
    8193 items - the tightest of the mistakes here."""
    x, _, _, _, _, gy = M.torgb_operands(hw4, 1, 16, 4, 4 * hw4)
    part = M.torgb_cross_partials(x, gy)
    out, bound = M.torgb_cross(x, gy), M.torgb_cross_bound(x, gy)
    assert np.abs(part.sum(axis=1) - out).max() <= 1e-9
    bad = np.delete(part, drop, axis=1).sum(axis=1)
    used = out != 0
    ratio = np.abs(bad - out)[used] / bound[used]
    # (the single-item block: every one of the 68 sums is off; most by much more than the bound, the median says so)
    assert np.median(ratio) > (WIDE if hw4 == 4097 or drop == 0 else 10.0), float(np.median(ratio))
    assert ratio.max() > WIDE


def test_prep_bounds_reject_scale_on_the_bias_and_swapped_indices():
    x, w, b, s, t, _ = M.torgb_operands(11, 3, 5, 3, 8)
    weff, beff = M.torgb_prep(w, b, s, t, SCALE, BIAS_SCALE)
    weff_b, beff_b = M.torgb_prep_bounds(w, b, s, t, SCALE, BIAS_SCALE)
    scaled_bias = SCALE * (np.einsum('oc,nc->no', w, t) + b[None, :] * BIAS_SCALE)
    assert _worst(scaled_bias, beff[:, :3], beff_b[:, :3]) > 1e4
    swapped = np.zeros_like(weff)
    wflat = w.reshape(-1)
    for ci in range(5):
        for co in range(3):
            swapped[:, ci, co] = SCALE * wflat[ci * 3 + co] * s[:, ci]      # w read as (Cin, Cout)
    assert _worst(swapped, weff, weff_b) > 1e4
    assert float((weff_b[:, :, :3] / np.abs(weff[:, :, :3])).max()) < 3 * tail.U        # two roundings, nothing more


def test_in_affine_bound_rejects_t_without_the_style_scale():
    rng = np.random.RandomState(5)
    mean, rstd = tail.f32(0.5 + rng.standard_normal((2, 7))), tail.f32(rng.uniform(0.5, 2.0, (2, 7)))
    style = tail.f32(0.5 * rng.standard_normal((2, 14)))
    s, t = M.in_affine(mean, rstd, style)
    s32 = M.in_affine_s_bits(rstd, style).astype(np.float64)
    assert np.abs(s32 - s).max() <= 2.1 * tail.U * np.abs(s).max()
    bound = M.in_affine_t_bound(mean, s32, style)
    _, yb = M._style(style, 2, 7)
    t_own = yb - mean * s32                                  # what the kernel is held to: t from ITS s
    assert _worst(tail.f32(t_own), t_own, bound) <= 1.0
    assert _worst(yb - mean * rstd, t_own, bound) > 1e4
    ys_not_plus_one = rstd * (M._style(style, 2, 7)[0] - 1.0)
    assert not np.array_equal(tail.f32(ys_not_plus_one), s32)         # (s is compared bit for bit)


def test_wgrad_bound_rejects_the_missing_shift_term():
    x, w, b, s, t, gy = M.torgb_operands(13, 3, 5, 3, 64)
    out = M.torgb_cross(x, gy)
    gw, gb = M.torgb_wgrad(out, s, t, SCALE, BIAS_SCALE, 3)
    gw_b, gb_b = M.torgb_wgrad_bounds(out, s, t, SCALE, BIAS_SCALE, 3)
    cross = out[:, :64].reshape(3, 16, 4)[:, :5, :3]
    assert _worst(SCALE * np.einsum('nc,nco->oc', s, cross), gw, gw_b) > 1e4
    assert _worst(tail.f32(gw), gw, gw_b) <= 1.0 and _worst(tail.f32(gb), gb, gb_b) <= 1.0


# ---- the regime operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', M.REGIMES)
def test_regime_operands_keep_the_reference_finite_and_of_order_one(regime):
    """|b| of order 1 in every regime, so no bound degenerates; the deferred form's own terms |a s| and |t| grow to
    |mean| rstd |ys + 1| on the near-constant planes - about 3e2 (near3) and 3e3 (near1) - and the deferred bound with them,
    while the materialised form's bound stays at a few u: the ratio the GPU tests report is bounded by this one."""
    a, style = M.regime_activation(7, (2, 16, 32, 32), regime)
    b, mean, rstd = M.materialised(a, style)
    assert np.isfinite(b).all() and 0.3 < np.sqrt((b ** 2).mean()) < 3.0
    d = M.deferred_bounds(a, style)
    mat = tail.instnorm_style_bound(a, style)
    assert np.isfinite(d['eb']).all() and (d['eb'] > 0).all()
    size = float(np.abs(d['t']).max())
    lo, hi = {'normal': (0.0, 10.0), 'near3': (50.0, 3e3), 'near1': (500.0, 3e4)}[regime]
    assert lo <= size <= hi, size
    # "a few u times (|a s| + |t|)": by count 3 + 2 on |a s| and 3 + 1 + 2 + 1 on |t|, each with the statistics' fp64 share
    # (|mean s| stands beside |t|: where yb happens to cancel mean s, t is small but was still formed from mean s)
    few = float((d['eb'] / (tail.U * (np.abs(a * d['s']) + np.abs(mean[:, :, None, None] * d['s']) + np.abs(d['t'])))).max())
    assert few < 12.0, few
    print(f'mod host | {regime}: max |t| {size:.3g}, deferred bound / materialised bound (rms) '
          f'{np.sqrt((d["eb"] ** 2).mean()) / np.sqrt((mat ** 2).mean()):.3g}')


@pytest.mark.parametrize('regime', M.REGIMES)
def test_deferred_image_bound_holds_for_a_simulated_fp32_chain_and_rejects_a_wrong_shift(regime):
    """The documented computation run in float32 on the CPU (numpy float32 arithmetic, statistics rounded to fp32) stays inside
    ``torgb_deferred_bounds`` of the materialised float64 image; the same chain with t built without (ys + 1) does not."""
    n, c, h, w = 2, 12, 16, 16
    a, style = M.regime_activation(3, (n, c, h, w), regime)
    rng = np.random.RandomState(4)
    wt, bias = tail.f32(0.5 * rng.standard_normal((3, c))), tail.f32(rng.standard_normal(3))
    b, mean, rstd = M.materialised(a, style)
    want = tail.torgb(b, wt, bias, SCALE, BIAS_SCALE)
    bound = M.torgb_deferred_bounds(a, style, wt, bias, SCALE, BIAS_SCALE)
    f = np.float32
    m32, r32 = mean.astype(f), rstd.astype(f)
    ys1 = (style.reshape(n, 2, c)[:, 0].astype(f) + f(1))
    s32 = r32 * ys1
    for wrong in (False, True):
        t32 = style.reshape(n, 2, c)[:, 1].astype(f) - m32 * (r32 if wrong else s32)
        weff = (f(SCALE) * wt.astype(f))[None, :, :] * s32[:, None, :]                  # (n, co, ci)
        beff = np.zeros((n, 3), dtype=f)
        for ci in range(c):
            beff = beff + wt.astype(f)[None, :, ci] * t32[:, ci:ci + 1]
        beff = beff * f(SCALE) + bias.astype(f)[None, :] * f(BIAS_SCALE)
        y = np.broadcast_to(beff[:, :, None, None], (n, 3, h, w)).astype(f)
        for ci in range(c):
            y = y + weff[:, :, ci, None, None] * a.astype(f)[:, None, ci]
        ratio = _worst(y.astype(np.float64), want, bound)
        print(f'mod host | simulated chain {regime} wrong={wrong}: worst error / bound {ratio:.3g}')
        assert (ratio > WIDE) if wrong else (ratio <= 1.0), ratio
