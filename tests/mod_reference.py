"""Float64 restatement of the modulated toRGB and deferred-InstanceNorm kernels of csrc/mod.hip (in_affine, toRGB prep, forward,
cross sums, weight / bias gradient), the plain-Python restatement of each launcher's plan, and the per-element error bounds the
GPU tests hold the kernels to.  Written from the semantics - b = (a - mean) rstd (ys + 1) + yb = a s + t
(stylegan/architectures.py:497-526), toRGB a 1x1 conv of b - in plain numpy; no kernel is ported.  Users:
tests/test_mod_host.py (the restatements against autograd in float64, every bound against the mistakes it must catch, every plan
at the edge its case names) and tests/test_gpu_mod.py (the kernels).

Conventions: those of tests/tail_reference.py.  Arrays are float64 whose values are float32 numbers; ``x`` / ``a`` is
(N, Cin, HW) or NCHW, ``s`` / ``t`` (N, Cin), ``style`` (N, 2 Cin) = [ys | yb], ``w`` (Cout, Cin), ``weff`` (N, Cin, 4),
``beff`` (N, 4), the cross sums ``out`` (N, 68) = 16 x 4 sums x[ci] . gy[co], then 4 sums of gy[co].

Bounds.  u = 2^-24, ``gamma(k)`` = ku / (1 - ku): k chained fp32 roundings (an FMA only removes some).  Every bound is a count
of roundings on the reference's own quantities, stated next to the formula it bounds; nothing is normalised by a maximum and
nothing measured enters a bound.  Every kernel is fed exact fp32 inputs; a later stage is given the earlier kernel's output."""
import numpy as np

import tail_reference as tail
from tail_reference import U, gamma, f32

SECOND_ORDER = 1.0 + 64 * U        # products of two first-order terms, dropped in the derivations below


def cdiv(a, b):
    return -(-a // b)


# ==== the launchers' plans ===========================================================================================================
FWD_CAP, CROSS_CAP, CROSS_ITEMS = 128, 64, 4096


def fwd_plan(n, hw):
    """ganlab_mod_torgb_fwd_f32: min(ceil(hw4 / 256), 128) blocks by N; a block's threads take float4 items blocks * 256 apart."""
    hw4 = hw // 4
    blocks = min(cdiv(hw4, 256), FWD_CAP)
    trips = cdiv(hw4, blocks * 256)
    return dict(launches=[('rm_torgb_fwd_kernel', blocks * n)], blocks=blocks, trips=trips, capped=cdiv(hw4, 256) > FWD_CAP,
                last_trip_items=hw4 - (trips - 1) * blocks * 256)


def cross_plan(n, hw):
    """ganlab_mod_torgb_cross_f32: clamp(ceil(hw4 / 4096), 1, 64) blocks by N, then N finish blocks that add the block partials in
    two interleaved chains (even blocks, odd blocks) and an odd last block on its own."""
    hw4 = hw // 4
    blocks = max(1, min(cdiv(hw4, CROSS_ITEMS), CROSS_CAP))
    trips = cdiv(hw4, blocks * 256)
    return dict(launches=[('rm_torgb_cross_kernel', blocks * n), ('rm_torgb_cross_finish_kernel', n)], blocks=blocks, trips=trips,
                capped=cdiv(hw4, CROSS_ITEMS) > CROSS_CAP, odd_tail=blocks % 2 == 1,
                last_trip_items=hw4 - (trips - 1) * blocks * 256)


def cross_workspace_bytes(n):
    return n * CROSS_CAP * 68 * 4


def prep_plan(n):
    return dict(launches=[('rm_torgb_prep_kernel', n)])


def wgrad_plan():
    return dict(launches=[('rm_torgb_wgrad_kernel', 1)])


def in_affine_plan(n, c):
    return dict(launches=[('in_affine_kernel', cdiv(n * c, 256))], last_block_items=n * c - (cdiv(n * c, 256) - 1) * 256)


# ==== in_affine ======================================================================================================================
def _style(style, n, c):
    if style is None:
        return np.ones((n, c)), np.zeros((n, c))
    st = np.asarray(style, dtype=np.float64).reshape(n, 2, c)
    return st[:, 0] + 1.0, st[:, 1]


def in_affine(mean, rstd, style):
    """s = rstd (ys + 1), t = yb - mean s per (n, c); style None: ys + 1 = 1, yb = 0."""
    n, c = mean.shape
    ys1, yb = _style(style, n, c)
    s = rstd * ys1
    return s, yb - mean * s


def in_affine_s_bits(rstd, style):
    """fl(rstd fl(ys + 1)) in float32 arithmetic: what ``s`` must be, bit for bit (two roundings in a fixed order; without a
    style the product with 1 is exact)."""
    n, c = rstd.shape
    r = rstd.astype(np.float32)
    if style is None:
        return r
    ys = np.asarray(style, dtype=np.float64).reshape(n, 2, c)[:, 0].astype(np.float32)
    return r * (ys + np.float32(1.0))


def in_affine_t_bound(mean, s_kernel, style):
    """t from the kernel's own fp32 s: fl(yb - fl(mean s)) or one fused rounding - u |mean s| for the product, u |t| (at the
    rounded product: + u^2 |mean s|) for the difference."""
    n, c = mean.shape
    _, yb = _style(style, n, c)
    ms = np.abs(mean * s_kernel)
    return U * ms + U * (np.abs(yb - mean * s_kernel) + U * ms)


# ==== toRGB: prep, forward ===========================================================================================================
def torgb_prep(w, bias, s, t, scale, bias_scale):
    """weff[n][ci][co] = scale w[co][ci] s[n, ci], beff[n][co] = bias[co] bias_scale + scale sum_ci w[co][ci] t[n, ci]; lanes
    co >= Cout are zero."""
    cout, cin = w.shape
    n = s.shape[0]
    weff, beff = np.zeros((n, cin, 4)), np.zeros((n, 4))
    weff[:, :, :cout] = scale * np.einsum('oc,nc->nco', w, s)
    beff[:, :cout] = scale * np.einsum('oc,nc->no', w, t) + (0.0 if bias is None else np.asarray(bias)[None, :] * bias_scale)
    return weff, beff


def torgb_prep_bounds(w, bias, s, t, scale, bias_scale):
    """weff: (scale w) s, two products.  beff: the Cin-term chain of w t from 0 (gamma(Cin)), times scale, bias bias_scale, the
    sum: gamma(Cin + 2) on |scale| sum |w t| and gamma(2) on |bias bias_scale|."""
    cout, cin = w.shape
    n = s.shape[0]
    weff_b, beff_b = np.zeros((n, cin, 4)), np.zeros((n, 4))
    weff_b[:, :, :cout] = gamma(2) * np.abs(scale) * np.einsum('oc,nc->nco', np.abs(w), np.abs(s))
    beff_b[:, :cout] = gamma(cin + 2) * np.abs(scale) * np.einsum('oc,nc->no', np.abs(w), np.abs(t)) + \
        (0.0 if bias is None else gamma(2) * np.abs(np.asarray(bias)[None, :] * bias_scale))
    return weff_b, beff_b


def torgb_fwd(x, weff, beff, cout):
    """y[n, co, px] = sum_ci weff[n][ci][co] x[n, ci, px] + beff[n][co]; x: (N, Cin, HW)."""
    return np.einsum('nco,ncp->nop', weff[:, :, :cout], x) + beff[:, :cout, None]


def torgb_fwd_bound(x, weff, beff, cout):
    """The accumulator starts at beff and takes Cin products in order: (Cin + 2) u (sum_ci |weff x| + |beff|)."""
    cin = x.shape[1]
    return gamma(cin + 2) * (np.einsum('nco,ncp->nop', np.abs(weff[:, :, :cout]), np.abs(x)) + np.abs(beff[:, :cout, None]))


# ==== toRGB: cross sums, weight / bias gradient ======================================================================================
def _cross_terms(x, gy):
    n, cin = x.shape[:2]
    cout = gy.shape[1]
    xp, gp = np.zeros((n, 16) + x.shape[2:]), np.zeros((n, 4) + gy.shape[2:])
    xp[:, :cin], gp[:, :cout] = x, gy
    return xp, gp


def torgb_cross(x, gy):
    """out[n][ci * 4 + co] = sum_px x[n, ci, px] gy[n, co, px] (ci < 16, co < 4; unused slots zero), out[n][64 + co] =
    sum_px gy[n, co, px]."""
    xp, gp = _cross_terms(x, gy)
    return np.concatenate([np.einsum('ncp,nop->nco', xp, gp).reshape(x.shape[0], 64), gp.sum(axis=2)], axis=1)


def torgb_cross_partials(x, gy):
    """The same sums per block of ``cross_plan``: (N, blocks, 68); float4 item q goes to block (q // 256) % blocks."""
    n, hw = x.shape[0], x.shape[2]
    blocks = cross_plan(n, hw)['blocks']
    owner = (np.arange(hw // 4) // 256) % blocks
    part = np.zeros((n, blocks, 68))
    for b in range(blocks):
        px = np.repeat(owner == b, 4)
        part[:, b] = torgb_cross(x[:, :, px], gy[:, :, px])
    return part


def cross_counts(hw):
    """Roundings a term of a cross sum passes: the float4's four products and two levels of sums (3; a gradient sum: 2), the
    thread's accumulator once per trip (at most ceil(hw4 / (blocks 256)) sequential terms), the wave tree (6), four waves (2), the
    pairwise finish over blocks (ceil(blocks / 2) sequential terms, then the two chains)."""
    p = cross_plan(1, hw)
    rest = p['trips'] + 6 + 2 + cdiv(p['blocks'], 2) + 1
    return 3 + rest, 2 + rest


def torgb_cross_bound(x, gy):
    xp, gp = _cross_terms(np.abs(x), np.abs(gy))
    kc, kg = cross_counts(x.shape[2])
    return np.concatenate([gamma(kc) * np.einsum('ncp,nop->nco', xp, gp).reshape(x.shape[0], 64), gamma(kg) * gp.sum(axis=2)], axis=1)


def torgb_wgrad(out, s, t, scale, bias_scale, cout):
    """gw[co][ci] = scale sum_n (s[n, ci] cross[n][ci][co] + t[n, ci] gsum[n][co]), gb[co] = bias_scale sum_n gsum[n][co]."""
    n, cin = s.shape
    cross, gsum = out[:, :64].reshape(n, 16, 4)[:, :cin, :cout], out[:, 64:64 + cout]
    gw = scale * (np.einsum('nc,nco->oc', s, cross) + np.einsum('nc,no->oc', t, gsum))
    return gw, bias_scale * gsum.sum(axis=0)


def torgb_wgrad_bounds(out, s, t, scale, bias_scale, cout):
    """Per image two products and their sum, the N-term chain, the scale: gamma(N + 3) on |scale| sum_n (|s cross| + |t gsum|);
    gb: the chain and the scale, gamma(N + 1) on |bias_scale| sum_n |gsum|."""
    n, cin = s.shape
    cross, gsum = np.abs(out[:, :64].reshape(n, 16, 4)[:, :cin, :cout]), np.abs(out[:, 64:64 + cout])
    gw_b = gamma(n + 3) * abs(scale) * (np.einsum('nc,nco->oc', np.abs(s), cross) + np.einsum('nc,no->oc', np.abs(t), gsum))
    return gw_b, gamma(n + 1) * abs(bias_scale) * gsum.sum(axis=0)


# ==== the deferred chain against the materialised definition ========================================================================
def materialised(a, style, eps=tail.EPS):
    """b = (a - mean) rstd (ys + 1) + yb from the exact statistics of the fp32 ``a`` (NCHW): the definition every deferred
    consumer is compared with.  Returns (b, mean, rstd) with (N, C) statistics."""
    n, c = a.shape[:2]
    mean, _, rstd = tail.instnorm_stats(a, eps)
    return tail.instnorm_style(a, style, eps), mean.reshape(n, c), rstd.reshape(n, c)


def deferred_bounds(a, style, eps=tail.EPS):
    """What the documented computation b^ = fl(a s^ + t^) allows per element, with s^ = fl(rstd^ fl(ys + 1)),
    t^ = fl(yb - fl(mean^ s^)) from the fp32 statistics (mean^, rstd^) the statistics kernels return - their errors
    e_m = |mean^ - mean|, e_r = |rstd^ - rstd| / rstd from ``tail_reference.stats_bounds``:
      ds = e_r + gamma(2)                           relative error of s^ (rstd^, ys + 1, the product)
      dt = |mean s| ds + |s| e_m + u (|mean s| + |t|)   error of t^ (s^ and mean^ inside it, its product, its difference)
      eb = |a s| ds + dt + u (|a s| + |b|)          error of b^ (s^, t^, the product and the sum - or one fma)
    a s ds and mean s ds are added, not cancelled: (a - mean) s ds is what an exact evaluation of the deferred form would leave,
    but fl(a s^) + t^ is formed from two numbers of size |t| each rounded on its own.  On a near-constant plane |a s| and |t| are
    about |mean| rstd |ys + 1|, so eb is a few u of THAT - not of |b|: the price of the deferred form, stated, not hidden.
    Returns dict(ds, dt, s, t: (N, C, 1, 1) per plane; eb, b: per element)."""
    n, c = a.shape[:2]
    mean, _, rstd = tail.instnorm_stats(a, eps)
    mean_b, rstd_b = tail.stats_bounds(a, eps)
    ys1, yb = tail._style_parts(style, n, c)
    s = rstd * ys1
    t = yb - mean * s
    b = a * s + t
    ds = rstd_b / rstd + gamma(2)
    dt = (np.abs(mean * s) * ds + np.abs(s) * mean_b + U * (np.abs(mean * s) + np.abs(t))) * SECOND_ORDER
    eb = (np.abs(a * s) * ds + dt + U * (np.abs(a * s) + np.abs(b))) * SECOND_ORDER
    return dict(ds=ds, dt=dt, eb=eb, s=s, t=t, b=b)


def torgb_deferred_bounds(a, style, w, bias, scale, bias_scale, eps=tail.EPS):
    """The image of ``ops.torgb_mod`` on a deferred tensor against scale W b + bias bias_scale of the materialised b:
      sum_ci |scale w| (|a s| (ds + gamma(2)) + dt)     s^ inside weff (and weff's two products), t^ inside beff
      gamma(Cin + 2) |scale| sum_ci |w t| + gamma(2) |bias bias_scale|      beff's own chain (``torgb_prep_bounds``)
      gamma(Cin + 2) (sum_ci |weff a| + |beff|)         the forward's chain (``torgb_fwd_bound``)."""
    d = deferred_bounds(a, style, eps)
    cout, cin = w.shape
    aw = np.abs(scale * w)
    as_ = np.abs(a * d['s'])
    beff = scale * np.einsum('oc,ncij->noij', w, d['t']) + (0.0 if bias is None else tail._per_channel(bias) * bias_scale)
    wt = np.einsum('oc,ncij->noij', aw, np.abs(d['t']))
    bb = 0.0 if bias is None else np.abs(tail._per_channel(bias) * bias_scale)
    return (np.einsum('oc,nchw->nohw', aw, as_ * (d['ds'] + gamma(2)) + d['dt']) + gamma(cin + 2) * wt + gamma(2) * bb +
            gamma(cin + 2) * (np.einsum('oc,nchw->nohw', aw, as_) + np.abs(beff))) * SECOND_ORDER


def torgb_deferred_grad_bounds(a, style, gy, scale, bias_scale, eps=tail.EPS):
    """gw = scale sum_{n, px} gy b and gb = bias_scale sum_{n, px} gy of the materialised b, as the kernels form them from the
    cross sums: s^ cross^ + t^ gsum^ per image.  cross^ and gsum^ carry ``torgb_cross_bound``, s^ and t^ carry ds and dt, the fold
    carries ``torgb_wgrad_bounds``."""
    n, c, h, wd = a.shape
    d = deferred_bounds(a, style, eps)
    s, t, ds, dt = (d[k].reshape(n, c) for k in ('s', 't', 'ds', 'dt'))
    x3, g3 = a.reshape(n, c, h * wd), gy.reshape(n, gy.shape[1], h * wd)
    cout = gy.shape[1]
    out, out_b = torgb_cross(x3, g3), torgb_cross_bound(x3, g3)
    cross, gsum = np.abs(out[:, :64].reshape(n, 16, 4)[:, :c, :cout]), np.abs(out[:, 64:64 + cout])
    cross_b, gsum_b = out_b[:, :64].reshape(n, 16, 4)[:, :c, :cout], out_b[:, 64:64 + cout]
    fold_w, fold_b = torgb_wgrad_bounds(out, s, t, scale, bias_scale, cout)
    gw_b = abs(scale) * (np.einsum('nc,nco->oc', np.abs(s) * ds, cross) + np.einsum('nc,nco->oc', np.abs(s), cross_b) +
                         np.einsum('nc,no->oc', dt, gsum) + np.einsum('nc,no->oc', np.abs(t), gsum_b)) + fold_w
    return gw_b * SECOND_ORDER, (abs(bias_scale) * gsum_b.sum(axis=0) + fold_b) * SECOND_ORDER


def conv_terms(kind, ks, cin, n, hw_out):
    """Number of terms a consumer adds into one output: a forward output ks^2 Cin products, a weight-gradient entry N H W.  A sum
    of k terms in ANY order is within gamma(k - 1) of sum |terms|; the packed weight's scale and the product add two."""
    return (ks * ks * cin if kind == 'fwd' else n * hw_out[0] * hw_out[1]) + 2


# ==== operands =======================================================================================================================
REGIMES = tail.REGIMES


def regime_activation(seed, shape, regime):
    """An activated tensor ``a`` (NCHW, exact fp32) as the layer tail leaves it: ``tail_reference.regime_plane`` - unit normal, or
    near-constant one-signed planes (what LeakyReLU outputs of a biased layer look like) - and a style (N, 2C)."""
    rng = np.random.RandomState(seed)
    a, _ = tail.regime_plane(rng, shape, regime)
    return a, f32(0.5 * rng.standard_normal((shape[0], 2 * shape[1])))


def torgb_operands(seed, n, cin, cout, hw, bias=True):
    """(x (N, Cin, HW), w (Cout, Cin), bias, s, t (N, Cin), gy (N, Cout, HW)) of the kernel-by-name cases: s and t as in_affine
    leaves them on planes with mean about 0.5 and unit spread (s about 1 +- 0.5, t of order 1), so |b| stays of order 1."""
    rng = np.random.RandomState(seed)
    x = f32(0.5 + rng.standard_normal((n, cin, hw)))
    w = f32(0.5 * rng.standard_normal((cout, cin)))
    b = f32(rng.standard_normal(cout)) if bias else None
    s = f32(1.0 + 0.5 * rng.uniform(-1, 1, (n, cin)))
    t = f32(rng.standard_normal((n, cin)))
    gy = f32(rng.standard_normal((n, cout, hw)))
    return x, w, b, s, t, gy
