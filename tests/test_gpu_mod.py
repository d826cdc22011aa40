"""GPU tests of the modulated toRGB and deferred-InstanceNorm kernels of csrc/mod.hip against the float64 restatement of
tests/mod_reference.py.

Part 1 - the kernels by name, through the C entry points (``_lib.lib()``), outputs inside guarded buffers: every case asserts the
launched symbols, the workgroup count of every launch against the restated plan, and the values against float64 within a
per-element count of roundings (derived in mod_reference.py next to each formula; nothing is normalised by a maximum).  A later
stage is fed the earlier kernel's own output.  One inf / NaN stays where linear algebra puts it; the entry points refuse bad
arguments without a launch.
Part 2 - the deferred chain against the MATERIALISED definition in float64, (s, t) from ``in_affine`` on statistics the library
computed itself, under each of ``tail_reference.REGIMES``: ``ops.torgb_mod`` on a ``Deferred`` (image, weight and bias gradient,
the gradient handed to the tail - unfolded and folded) and one run per affine-on-load row of tests/exact_forms.py.  The bound is
what the documented computation a s + t allows (``mod_reference.deferred_bounds``).  Each regime also prints the rms error of
the deferred path over that of the materialised GPU path (``layer_tail`` then ``conv2d``): reported, not asserted.
Every check prints ``worst error / bound``.  ``test_every_mod_kernel_is_accounted_for`` closes the module over ``REQUIRED``.
tests/test_mod_host.py shows on the CPU that each bound rejects the mistakes it is meant to catch.
Measured worst error / bound: DESIGN.md section 4.25."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import exact_forms as E
import mod_reference as M
import tail_reference as ref
import x3_forms as X

pytestmark = pytest.mark.gpu

SCALE, BIAS_SCALE = float(np.float32(0.25)), float(np.float32(0.7))
EPS, SLOPE = ref.EPS, ref.SLOPE
GUARD, SENTINEL = 64, -7.25
EINVAL, EWORKSPACE = -1, -2
SEEN = set()
REQUIRED = ['rm_torgb_prep_kernel', 'rm_torgb_fwd_kernel', 'rm_torgb_cross_kernel', 'rm_torgb_cross_finish_kernel',
            'rm_torgb_wgrad_kernel', 'in_affine_kernel']


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def _L():
    from gan_lab_amd import _lib
    return _lib.lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().cuda() if a is not None else None


def _n(t):
    return t.detach().double().cpu().numpy()


class Guarded(object):
    """``numel`` floats between two runs of sentinel floats (``behind``: at least that many after the payload)."""

    def __init__(self, numel, behind=GUARD, fill=SENTINEL):
        self.numel, self.behind = numel, max(GUARD, (behind + 3) // 4 * 4)
        self.buf = torch.full((GUARD + numel + self.behind,), SENTINEL, dtype=torch.float32, device='cuda')
        self.view = self.buf[GUARD:GUARD + numel]
        self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.numel:] == SENTINEL).all())


def _norm(launches):
    out = [(E.norm(k or ''), n) for k, n in launches]
    SEEN.update(k for k, _ in out)
    return out


class _launched(object):
    """The launches of the block are exactly ``plan``: [(symbol, workgroups)] in order."""

    def __init__(self, what, plan):
        self.what, self.plan = what, plan

    def __enter__(self):
        from gan_lab_amd import _lib
        self.c0 = _lib.launch_count()
        return self

    def __exit__(self, et, ev, tb):
        from gan_lab_amd import _lib
        if et is None:
            torch.cuda.synchronize()
            self.got = _norm(_lib.launches_since(self.c0))
            print(f'mod | {self.what}: launched {self.got}')
            assert len(self.got) == len(self.plan), (self.what, self.got, self.plan)
            for (k, n), (sym, grid) in zip(self.got, self.plan):
                assert sym in k and n == grid, (self.what, self.got, self.plan)
        return False


def _unlaunched(what, rc, want, c0):
    from gan_lab_amd import _lib
    assert rc == want and _lib.launch_count() == c0, (what, rc, want, _lib.launch_count() - c0)


def _check(what, got, want, tol, finite=True):
    got = _n(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    got = got.reshape(want.shape)
    if finite:
        assert np.isfinite(got).all(), what
    err, tol = np.abs(got - want), np.broadcast_to(np.asarray(tol, dtype=np.float64), want.shape)
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    print(f'mod | {what}: max error {err.max():.3e}, worst error / bound {ratio.max():.3f}')
    assert (err <= tol).all(), (what, float(err.max()), float(ratio.max()))
    return float(ratio.max())


def _rms(got, want):
    return float(np.sqrt(((_n(got).reshape(want.shape) - want) ** 2).mean()))


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def k_in_affine(mean, rstd, style, s, t, n, c):
    return _L().ganlab_in_affine_f32(_p(mean), _p(rstd), _p(style), _p(s), _p(t), n, c, _st())


def k_prep(w, bias, s, t, weff, beff, n, cin, cout):
    return _L().ganlab_mod_torgb_prep_f32(_p(w), _p(bias), _p(s), _p(t), _p(weff), _p(beff), n, cin, cout, SCALE, BIAS_SCALE, _st())


def k_fwd(x, weff, beff, y, n, cin, cout, hw):
    return _L().ganlab_mod_torgb_fwd_f32(_p(x), _p(weff), _p(beff), _p(y), n, cin, cout, hw, _st())


def k_cross(x, gy, out, n, cin, cout, hw, ws, ws_bytes=None):
    return _L().ganlab_mod_torgb_cross_f32(_p(x), _p(gy), _p(out), n, cin, cout, hw, _p(ws),
                                           ws.numel() * 4 if ws_bytes is None else ws_bytes, _st())


def k_wgrad(cross, s, t, gw, gb, n, cin, cout):
    return _L().ganlab_mod_torgb_wgrad_f32(_p(cross), _p(s), _p(t), _p(gw), _p(gb), n, cin, cout, SCALE, BIAS_SCALE, _st())


def _workspace(n):
    nbytes = int(_L().ganlab_mod_torgb_cross_workspace(n))
    assert nbytes == M.cross_workspace_bytes(n)
    return torch.empty(nbytes // 4, dtype=torch.float32, device='cuda')


# ==== part 1: the kernels by name ====================================================================================================
@pytest.mark.parametrize('nc', [1, 255, 256, 257, 513], ids=str)
@pytest.mark.parametrize('with_style', [True, False], ids=['style', 'nostyle'])
def test_in_affine_kernel(nc, with_style):
    """N C = 1 .. 513 as N = 1 and, where it divides, N = 3 (the style's row stride); the last block holds 1, 255, 256, 1, 1
    threads.  s bit-exact against fl(rstd fl(ys + 1)), t within its two roundings of yb - mean s from the kernel's own s.
    Measured: t 0.98 (two roundings, nearly used up)."""
    for n in ([1, 3] if nc % 3 == 0 else [1]):
        c = nc // n
        rng = np.random.RandomState(nc + n)
        mean, rstd = ref.f32(0.5 + rng.standard_normal((n, c))), ref.f32(rng.uniform(0.3, 3.0, (n, c)))
        style = ref.f32(0.5 * rng.standard_normal((n, 2 * c))) if with_style else None
        s, t = Guarded(n * c), Guarded(n * c)
        with _launched(f'in_affine N={n} C={c} style={with_style}', M.in_affine_plan(n, c)['launches']):
            assert k_in_affine(_g(mean), _g(rstd), _g(style), s.view, t.view, n, c) == 0
        assert s.intact() and t.intact()
        assert np.array_equal(s.view.cpu().numpy().reshape(n, c), M.in_affine_s_bits(rstd, style)), 's is not fl(rstd fl(ys + 1))'
        s_own = _n(s.view).reshape(n, c)
        _, yb = M._style(style, n, c)
        _check(f'in_affine N={n} C={c} style={with_style} t', t.view, yb - mean * s_own, M.in_affine_t_bound(mean, s_own, style))


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('n', [1, 3], ids=['N1', 'N3'])
def test_torgb_prep_kernel(n, with_bias):
    """Cin in {1, 5, 16} x Cout in {1, 3, 4}: weff within two roundings, beff within its Cin + 2; lanes co >= Cout exactly zero;
    rows ci >= Cin (the floats behind weff) untouched.  Measured: weff 0.48, beff 0.59."""
    for cin in (1, 5, 16):
        for cout in (1, 3, 4):
            _, w, b, s, t, _ = M.torgb_operands(100 * n + 10 * cin + cout, n, cin, cout, 4, bias=with_bias)
            weff, beff = Guarded(n * cin * 4, fill=3.5), Guarded(n * 4, fill=3.5)
            what = f'prep N={n} {cin}->{cout} bias={with_bias}'
            with _launched(what, M.prep_plan(n)['launches']):
                assert k_prep(_g(w), _g(b), _g(s), _g(t), weff.view, beff.view, n, cin, cout) == 0
            assert weff.intact() and beff.intact(), what
            we, be = _n(weff.view).reshape(n, cin, 4), _n(beff.view).reshape(n, 4)
            assert not we[:, :, cout:].any() and not be[:, cout:].any(), what + ': padded lanes'
            wr, br = M.torgb_prep(w, b, s, t, SCALE, BIAS_SCALE)
            wb, bb = M.torgb_prep_bounds(w, b, s, t, SCALE, BIAS_SCALE)
            _check(what + ' weff', we, wr, wb)
            _check(what + ' beff', be, br, bb)


FWD_HW = [(1, 4), (1, 1028), (2, 4 * 128 * 256 + 20)]


@pytest.mark.parametrize('cin,cout', [(1, 1), (5, 3), (16, 4), (16, 3)], ids=['1to1', '5to3', '16to4', '16to3'])
@pytest.mark.parametrize('n,hw', FWD_HW, ids=[f'N{n}-HW{hw}' for n, hw in FWD_HW])
def test_torgb_fwd_kernel(n, hw, cin, cout):
    """HW = 4: one thread; 1028: a second block with one item; 4 * 128 * 256 + 20 with N = 2: 129 blocks asked, 128 given, a second
    trip of 5 items.  (weff, beff) are ``rm_torgb_prep_kernel``'s own output.  The floats behind y - where planes co >= Cout of
    the last image would land - are untouched.  Bound: (Cin + 2) u (sum |weff x| + |beff|).  Measured: 0.49."""
    x, w, b, s, t, _ = M.torgb_operands(hw + 10 * cin + cout, n, cin, cout, hw)
    weff, beff = torch.empty(n * cin * 4, device='cuda'), torch.empty(n * 4, device='cuda')
    assert k_prep(_g(w), _g(b), _g(s), _g(t), weff, beff, n, cin, cout) == 0
    y = Guarded(n * cout * hw, behind=(4 - cout) * hw)
    plan = M.fwd_plan(n, hw)
    what = f'fwd N={n} HW={hw} {cin}->{cout}'
    with _launched(what, plan['launches']):
        assert k_fwd(_g(x), weff, beff, y.view, n, cin, cout, hw) == 0
    assert y.intact(), what + ': wrote outside y'
    we, be = _n(weff).reshape(n, cin, 4), _n(beff).reshape(n, 4)
    _check(what, y.view, M.torgb_fwd(x, we, be, cout), M.torgb_fwd_bound(x, we, be, cout))


CROSS_CASES = [(2, 16, 4, 1), (2, 16, 4, 4097), (2, 16, 4, 2 * 4096 + 1), (1, 16, 4, 64 * 4096 + 7), (2, 5, 3, 4097), (3, 1, 1, 2 * 4096 + 1),
               (2, 12, 4, 1), (2, 16, 2, 257)]


@pytest.mark.parametrize('n,cin,cout,hw4', CROSS_CASES, ids=[f'N{n}-{ci}to{co}-hw4_{q}' for n, ci, co, q in CROSS_CASES])
def test_torgb_cross_kernels(n, cin, cout, hw4):
    """hw4 = 1; 4097: two blocks; 2 * 4096 + 1: three blocks, the odd tail of the finish; 64 * 4096 + 7: 65 blocks asked, 64 given,
    17 trips, the last with 7 items.  Cin < 16 / Cout < 4: the unused slots of out are exactly zero.  Bound: ``cross_counts``
    roundings on sum |x gy| (at most 61 at the largest case).  Two runs: equal bits.  Measured: 0.11 (a worst case over
    tens of chained sums against their random walk; a block left out of the finish misses it by > 100, test_mod_host.py)."""
    hw = 4 * hw4
    x, _, _, _, _, gy = M.torgb_operands(hw4 + cin, n, cin, cout, hw)
    xg, gg, ws = _g(x), _g(gy), _workspace(n)
    plan = M.cross_plan(n, hw)
    what = f'cross N={n} {cin}->{cout} hw4={hw4}'
    out = Guarded(n * 68)
    with _launched(what, plan['launches']):
        assert k_cross(xg, gg, out.view, n, cin, cout, hw, ws) == 0
    again = Guarded(n * 68)
    assert k_cross(xg, gg, again.view, n, cin, cout, hw, ws) == 0
    assert out.intact() and torch.equal(out.view, again.view), what
    got = _n(out.view).reshape(n, 68)
    cross = got[:, :64].reshape(n, 16, 4)
    assert not cross[:, cin:].any() and not cross[:, :, cout:].any() and not got[:, 64 + cout:].any(), what + ': unused slots'
    _check(what, got, M.torgb_cross(x, gy), M.torgb_cross_bound(x, gy))


@pytest.mark.parametrize('which', ['gw', 'gb', 'both'])
@pytest.mark.parametrize('n', [1, 3, 8], ids=['N1', 'N3', 'N8'])
def test_torgb_wgrad_kernel(n, which):
    """From ``rm_torgb_cross_kernel``'s own sums (5 -> 3 channels, 64 pixels): gw within N + 3 roundings, gb within N + 1; an output
    passed as null is not written - the other one and every guard stay as they were.  Measured: gw 0.27, gb 0.29."""
    cin, cout, hw = 5, 3, 64
    x, _, _, s, t, gy = M.torgb_operands(n, n, cin, cout, hw)
    out = torch.empty(n * 68, device='cuda')
    assert k_cross(_g(x), _g(gy), out, n, cin, cout, hw, _workspace(n)) == 0
    gw, gb = Guarded(cout * cin, fill=3.5), Guarded(cout, fill=3.5)
    with _launched(f'wgrad N={n} {which}', M.wgrad_plan()['launches']):
        assert k_wgrad(out, _g(s), _g(t), gw.view if which != 'gb' else None, gb.view if which != 'gw' else None, n, cin, cout) == 0
    assert gw.intact() and gb.intact()
    own = _n(out).reshape(n, 68)
    gw_r, gb_r = M.torgb_wgrad(own, s, t, SCALE, BIAS_SCALE, cout)
    gw_b, gb_b = M.torgb_wgrad_bounds(own, s, t, SCALE, BIAS_SCALE, cout)
    if which != 'gb':
        _check(f'wgrad N={n} {which} gw', gw.view, gw_r, gw_b)
    else:
        assert bool((gw.view == 3.5).all()), 'a null gw was written'
    if which != 'gw':
        _check(f'wgrad N={n} {which} gb', gb.view, gb_r, gb_b)
    else:
        assert bool((gb.view == 3.5).all()), 'a null gb was written'


@pytest.mark.parametrize('value', [float('inf'), float('nan')], ids=['inf', 'nan'])
def test_non_finite_stays_where_linear_algebra_puts_it(value):
    """One inf / NaN in x[1, 2, pixel 1029] (the second block's first item at HW = 2052): the forward is non-finite in that pixel
    column of image 1 - every colour - and nowhere else; the cross sums in the four lanes of row (n = 1, ci = 2) and nowhere else, the gradient
    sums untouched.  Everything else keeps the bits of the clean run."""
    n, cin, cout, hw, px = 2, 5, 3, 2052, 1029
    x, w, b, s, t, gy = M.torgb_operands(77, n, cin, cout, hw)
    bad = x.copy()
    bad[1, 2, px] = value
    weff, beff = torch.empty(n * cin * 4, device='cuda'), torch.empty(n * 4, device='cuda')
    assert k_prep(_g(w), _g(b), _g(s), _g(t), weff, beff, n, cin, cout) == 0
    ws = _workspace(n)
    res = []
    for xv in (x, bad):
        y, out = Guarded(n * cout * hw, behind=hw), Guarded(n * 68)
        with _launched(f'non-finite {value} fwd', M.fwd_plan(n, hw)['launches']):
            assert k_fwd(_g(xv), weff, beff, y.view, n, cin, cout, hw) == 0
        with _launched(f'non-finite {value} cross', M.cross_plan(n, hw)['launches']):
            assert k_cross(_g(xv), _g(gy), out.view, n, cin, cout, hw, ws) == 0
        assert y.intact() and out.intact()
        res.append((y.view.cpu().numpy().reshape(n, cout, hw), out.view.cpu().numpy().reshape(n, 68)))
    (y0, o0), (y1, o1) = res
    with np.errstate(invalid='ignore'):
        want_y = ~np.isfinite(M.torgb_fwd(bad, _n(weff).reshape(n, cin, 4), _n(beff).reshape(n, 4), cout))
        want_o = ~np.isfinite(M.torgb_cross(bad, gy))
    col = np.zeros((n, cout, hw), dtype=bool)
    col[1, :, px] = True
    row = np.zeros((n, 68), dtype=bool)
    row[1, 2 * 4:2 * 4 + 4] = True         # (the padded lane co = 3 too: 0 * inf, in the restatement as in the kernel; nobody reads it)
    assert np.array_equal(want_y, col) and np.array_equal(want_o, row)
    assert np.isfinite(y0).all() and np.isfinite(o0).all()
    print(f'mod | non-finite {value}: forward non-finite at {int((~np.isfinite(y1)).sum())} (reference {int(col.sum())}), '
          f'cross sums at {int((~np.isfinite(o1)).sum())} (reference {int(row.sum())})')
    assert np.array_equal(~np.isfinite(y1), col) and np.array_equal(~np.isfinite(o1), row)
    assert np.array_equal(y1[~col], y0[~col]) and np.array_equal(o1[~row], o0[~row])


def test_entry_points_refuse_without_a_launch():
    """Cout = 5, Cin = 17 (the entry points whose kernels index 16 x 4 lanes: prep, cross, wgrad - the forward's loop over Cin is
    general and has no such limit), HW % 4 != 0, x / y / gy / weff four bytes off a 16-byte boundary, a cross workspace one byte
    short (EWORKSPACE), null pointers, N = 0: the error code, and ``launch_count`` unchanged."""
    from gan_lab_amd import _lib
    n, cin, cout, hw = 2, 5, 3, 64
    big = torch.zeros(4096, device='cuda')
    off = big[1:]
    assert off.data_ptr() % 16 == 4
    ws = _workspace(n)
    c0 = _lib.launch_count()
    ok_fwd = dict(x=big, weff=big, beff=big, y=big, n=n, cin=cin, cout=cout, hw=hw)
    for what, kw in [('Cout=5', dict(cout=5)), ('HW=66', dict(hw=66)), ('x off', dict(x=off)), ('y off', dict(y=off)),
                     ('weff off', dict(weff=off)), ('x null', dict(x=None)), ('weff null', dict(weff=None)), ('beff null', dict(beff=None)),
                     ('y null', dict(y=None)), ('N=0', dict(n=0)), ('Cin=0', dict(cin=0))]:
        _unlaunched('fwd ' + what, k_fwd(**dict(ok_fwd, **kw)), EINVAL, c0)
    ok_prep = dict(w=big, bias=big, s=big, t=big, weff=big, beff=big, n=n, cin=cin, cout=cout)
    for what, kw in [('Cout=5', dict(cout=5)), ('Cin=17', dict(cin=17)), ('N=0', dict(n=0))] + \
            [(k + ' null', {k: None}) for k in ('w', 's', 't', 'weff', 'beff')]:
        _unlaunched('prep ' + what, k_prep(**dict(ok_prep, **kw)), EINVAL, c0)
    ok_cross = dict(x=big, gy=big, out=big, n=n, cin=cin, cout=cout, hw=hw, ws=ws)
    for what, kw in [('Cout=5', dict(cout=5)), ('Cin=17', dict(cin=17)), ('HW=66', dict(hw=66)), ('x off', dict(x=off)),
                     ('gy off', dict(gy=off)), ('N=0', dict(n=0))] + [(k + ' null', {k: None}) for k in ('x', 'gy', 'out')]:
        _unlaunched('cross ' + what, k_cross(**dict(ok_cross, **kw)), EINVAL, c0)
    _unlaunched('cross workspace one byte short', k_cross(**dict(ok_cross, ws_bytes=M.cross_workspace_bytes(n) - 1)), EWORKSPACE, c0)
    _unlaunched('cross workspace null', _L().ganlab_mod_torgb_cross_f32(_p(big), _p(big), _p(big), n, cin, cout, hw, None,
                                                                        M.cross_workspace_bytes(n), _st()), EWORKSPACE, c0)
    ok_wg = dict(cross=big, s=big, t=big, gw=big, gb=big, n=n, cin=cin, cout=cout)
    for what, kw in [('Cout=5', dict(cout=5)), ('Cin=17', dict(cin=17)), ('N=0', dict(n=0))] + \
            [(k + ' null', {k: None}) for k in ('cross', 's', 't')]:
        _unlaunched('wgrad ' + what, k_wgrad(**dict(ok_wg, **kw)), EINVAL, c0)
    ok_aff = dict(mean=big, rstd=big, style=big, s=big, t=big, n=n, c=cin)
    for what, kw in [('N=0', dict(n=0)), ('C=0', dict(c=0))] + [(k + ' null', {k: None}) for k in ('mean', 'rstd', 's', 't')]:
        _unlaunched('in_affine ' + what, k_in_affine(**dict(ok_aff, **kw)), EINVAL, c0)
    torch.cuda.synchronize()
    assert not big.any()


# ==== part 2: the deferred chain against the materialised definition ================================================================
def _stats_and_affine(a_gpu, style_gpu):
    """(s, t) as the library makes them: ganlab_instnorm_stats_f32 on ``a``, then ganlab_in_affine_f32."""
    n, c, h, w = a_gpu.shape
    mean, rstd, s, t = (torch.empty(n, c, device='cuda') for _ in range(4))
    assert _L().ganlab_instnorm_stats_f32(_p(a_gpu), _p(mean), _p(rstd), n * c, h * w, EPS, _st()) == 0
    with _launched(f'in_affine {n}x{c}', M.in_affine_plan(n, c)['launches']):
        assert k_in_affine(mean, rstd, style_gpu, s, t, n, c) == 0
    return s, t


class _Tape(object):
    """Launches of a backward pass, read on autograd's device thread from tensor hooks - piecewise, since the library keeps the
    last 16 only."""

    def __init__(self):
        self.launches, self.c = [], None

    def start(self, _):
        from gan_lab_amd import _lib
        if self.c is None:
            self.c = _lib.launch_count()

    def read(self, _):
        from gan_lab_amd import _lib
        now = _lib.launch_count()
        assert now - self.c <= 16, 'more launches between two hooks than the library keeps'
        self.launches += _norm(_lib.launches_since(self.c))
        self.c = now


def _is_pw_dgrad(k):
    return 'FwdCfg<1,' in k or 'pw_few_to_many_kernel' in k or 'pw_many_to_few_kernel' in k


TORGB_CASES = [(16, (32, 32)), (12, (32, 32)), (16, (16, 64)), (12, (16, 64))]


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('c,hw', TORGB_CASES, ids=[f'{c}ch-{h}x{w}' for c, (h, w) in TORGB_CASES])
def test_torgb_mod_on_a_deferred_tail_against_the_materialised_definition(c, hw, regime, monkeypatch):
    """``layer_tail_deferred`` -> ``torgb_mod``, 3 colours, N = 2.  Reference: the float64 statistics of the kernel's own activated
    tensor, b materialised, then the 1x1 conv and its gradients.  Image: ``torgb_deferred_bounds``; weight and bias gradient:
    ``torgb_deferred_grad_bounds``; the gradient handed to the tail, d / d (a s + t): with GANLAB_TORGB_FOLD=0 the 1x1 input gradient
    itself (``tail_reference.torgb_input_grad``; the restated 1x1 plan must be among the launches), folded (H W = 1024) the
    tail's own input gradient (``layer_tail_bwd_bounds`` with ``g_err``), with instnorm_bwd_reduce_rgb_kernel and no 1x1 kernel
    among the launches.  Prints deferred / materialised rms error of the image per regime.
    Measured (largest over cases; normal / near3 / near1): image 0.20 / 0.07 / 0.08, gw 0.011 / 0.007 / 0.006, gb 0.010, d/db 0.66,
    tail input gradient 0.39 / 0.68 / 0.93 folded and unfolded alike; deferred / materialised rms error of the image 1.4 - 1.6 /
    3.4 - 12.2 / 2.4 - 8.9."""
    from gan_lab_amd import ops
    h, w = hw
    n = 2
    x, b, nz, nw, style, _ = ref.tail_operands(c + h, n, c, h, w, regime)
    rng = np.random.RandomState(c + w)
    wrgb, brgb = ref.f32(0.5 * rng.standard_normal((3, c))), ref.f32(rng.standard_normal(3))
    grgb = ref.f32(rng.standard_normal((n, 3, h, w)))
    scale = float(np.float32(1.0 / np.sqrt(c)))
    what = f'torgb_mod C={c} {h}x{w} {regime}'
    xg, bg, nwg, sg = (_g(v).requires_grad_(True) for v in (x, b, nw, style))
    wg, brg = _g(wrgb.reshape(3, c, 1, 1)).requires_grad_(True), _g(brgb).requires_grad_(True)

    def run(fold):
        if fold:
            monkeypatch.delenv('GANLAB_TORGB_FOLD', raising=False)
        else:
            monkeypatch.setenv('GANLAB_TORGB_FOLD', '0')
        d = ops.layer_tail_deferred(xg, bg, _g(nz), nwg, sg, BIAS_SCALE, 'lrelu', SLOPE, False, EPS)
        assert ops.torgb_mod_ok(d, wg)
        with _launched(what, M.prep_plan(n)['launches'] + M.fwd_plan(n, h * w)['launches']):
            rgb = ops.torgb_mod(d, wg, brg, scale, BIAS_SCALE)
        tape, got = _Tape(), {}
        handles = [rgb.register_hook(tape.start), d.a.register_hook(lambda g: (got.__setitem__('ga', g.clone()), tape.read(g))[1])]
        handles += [v.register_hook(tape.read) for v in (xg, wg, brg)]
        for v in (xg, bg, nwg, sg, wg, brg):
            v.grad = None
        torch.autograd.backward([rgb], [_g(grgb)])
        torch.cuda.synchronize()
        for hd in handles:
            hd.remove()
        print(f'mod | {what} fold={fold} backward: launched {tape.launches}')
        return d, rgb.detach(), got['ga'], xg.grad.clone(), wg.grad.clone(), brg.grad.clone(), tape.launches

    d, rgb, ga, gx_u, gw, gb, launches = run(False)
    ya = _n(d.a)
    bmat, _, _ = M.materialised(ya, style)
    want = ref.torgb(bmat, wrgb, brgb, scale, BIAS_SCALE)
    _check(what + ' image', rgb, want, M.torgb_deferred_bounds(ya, style, wrgb, brgb, scale, BIAS_SCALE))
    gw_b, gb_b = M.torgb_deferred_grad_bounds(ya, style, grgb, scale, BIAS_SCALE)
    _check(what + ' gw', gw, scale * np.einsum('nohw,nchw->oc', grgb, bmat), gw_b)
    _check(what + ' gb', gb, BIAS_SCALE * grgb.sum(axis=(0, 2, 3)), gb_b)
    for sym, grid in M.cross_plan(n, h * w)['launches'] + M.wgrad_plan()['launches']:
        assert any(sym in k and g == grid for k, g in launches), (what, sym, grid, launches)
    gy_ref, g_err = ref.torgb_input_grad(grgb, wrgb, scale)
    assert E.plan_found(E.run_conv_plan(n, 3, h, w, c, 1, 0), launches), (what, 'no 1x1 input gradient', launches)
    assert any(_is_pw_dgrad(k) for k, _ in launches) and not any('instnorm_bwd_reduce_rgb_kernel' in k for k, _ in launches)
    _check(what + ' d/d(a s + t), unfolded', ga, gy_ref, g_err)
    # folded through RgbGradLink: the tail's own input gradient carries it
    d2, rgb2, _, gx_f, gw2, gb2, launches = run(True)
    assert torch.equal(rgb2, rgb) and torch.equal(gw2, gw) and torch.equal(gb2, gb) and torch.equal(d2.a, d.a)
    assert any('instnorm_bwd_reduce_rgb_kernel' in k for k, _ in launches), (what, launches)
    assert not any(_is_pw_dgrad(k) for k, _ in launches), (what, 'a 1x1 input gradient ran although the fold applies', launches)
    gx, _, _, _, _ = ref.layer_tail_bwd(gy_ref, ya, style, nz, SLOPE, BIAS_SCALE)
    gx_b, _, _, _, _ = ref.layer_tail_bwd_bounds(gy_ref, ya, style, nz, SLOPE, BIAS_SCALE, g_err=g_err)
    _check(what + ' tail input gradient, folded', gx_f, gx, gx_b)
    _check(what + ' tail input gradient, unfolded', gx_u, gx, gx_b)
    # the materialised GPU path on the same operands: layer_tail, then conv2d
    with torch.no_grad():
        mat = ops.conv2d(ops.layer_tail(xg, bg, _g(nz), nwg, sg, BIAS_SCALE, 'lrelu', SLOPE, False, EPS), wg, brg, scale=scale, padding=0,
                         bias_scale=BIAS_SCALE)
    ed, em = _rms(rgb, want), _rms(mat, want)
    print(f'mod | {what} image: rms error deferred {ed:.3e}, materialised {em:.3e}, deferred / materialised {ed / max(em, 1e-300):.2f}')


AFF_ROWS = [k for k, r in E.ROWS.items() if r.aff and k != 'wgrad_roll_aff_wide']


def _carried(f, eb, b, T64):
    """The consumer's bound from the per-element bound ``eb`` of b: the row's own float64 form on (eb, |w|) resp. (eb, |gy|) -
    sum |w| eb, zero in the padding - plus the consumer's accumulation count on the same form of (|b|, |w|)."""
    up = 4 if f.kind == 'up' else 0                 # (the folded stride-2 kernels add weights before they multiply)
    tb, te = torch.from_numpy(np.abs(b)), torch.from_numpy(eb)
    if f.role == 'wgrad':
        k = M.conv_terms('wgrad', f.ks, f.ci, f.n, f.hw_out) + up
        g = T64.gy.abs()
        return (E.r_wgrad(f, te, g) + ref.gamma(k) * E.r_wgrad(f, tb, g)).numpy()
    k = M.conv_terms('fwd', f.ks, f.ci, f.n, f.hw_out) + up
    wa = T64.wt.abs()
    lin_b = E.r_lin(f, te, wa) + ref.gamma(k) * E.r_lin(f, tb, wa)
    if not f.tail:
        return lin_b.numpy()
    # the tail epilogue: (blur: 4 roundings,) + noise_w noise + bias bias_scale, LeakyReLU (Lipschitz 1; one product)
    lin = E.r_lin(f, tb, wa)
    if f.op == 'up_blur_tail':
        lin_b, lin = E.r_blur(lin_b) + ref.gamma(4) * E.r_blur(lin), E.r_blur(lin)
    mag = lin + (T64.nw.view(1, -1, 1, 1) * T64.nz).abs() + E._cb(T64.b, X.TAIL_BIAS_SCALE).abs()
    return (lin_b + ref.gamma(5) * mag).numpy()


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('name', AFF_ROWS)
def test_affine_on_load_row_with_statistics_derived_affine(name, regime):
    """The affine-on-load rows of tests/exact_forms.py - same shapes, same symbol and plan assertions - with ``a`` drawn per regime
    and (s, t) from the library's own statistics of it, against the row's float64 form on the MATERIALISED b.  Bound:
    ``deferred_bounds`` per element of b, carried through sum |w| (resp. sum |gy|), plus the consumer's accumulation count
    (``_carried``).  The tail rows are held on their activated output y; their statistics of y stay with
    tests/test_gpu_exact_kernels.py.  (wgrad_roll_aff_wide, 22 MB of x in three regimes, is left to that table.)
    Forward rows also print deferred / materialised (``instnorm_style`` then ``conv2d``) rms error.
    Measured (largest over rows): forward and tail rows 0.045 / 0.032 / 0.018 (normal / near3 / near1), weight gradients 0.008 (their
    count is the worst case of N H W chained roundings); deferred / materialised rms error 1.00 / 1.6 / 1.1 - 1.5."""
    from gan_lab_amd import ops
    f = E.ROWS[name]
    T = X.draw(f, 'randn')
    shp = f.operand_shapes()['x']
    a, style = M.regime_activation(len(name) + shp[1], shp, regime)
    ag, stg = _g(a), _g(style)
    s, t = _stats_and_affine(ag, stg)
    T = T._replace(x=torch.from_numpy(a).float(), s=s.cpu(), t=t.cpu())
    got, launches = E.run(ops, f, T)
    SEEN.update(k for k, _ in launches)
    print(f'mod | row {name} {regime}: launched {launches}')
    assert any(E.norm(f.symbol) in k for k, _ in launches), (name, f.symbol, launches)
    assert E.plan_found(f.plan, launches), (name, f.plan, launches)
    d = M.deferred_bounds(a, style)
    bmat, _, _ = M.materialised(a, style)
    T64 = X.to_f64(T)._replace(x=torch.from_numpy(bmat), s=torch.ones(shp[:2], dtype=torch.float64), t=torch.zeros(shp[:2], dtype=torch.float64))
    want = f.ref(f, T64)[0].detach().numpy()
    bound = _carried(f, np.broadcast_to(d['eb'], a.shape).copy(), bmat, T64)
    _check(f'row {name} {regime} {f.outs[0]}', got[0], want, bound)
    if f.op == 'fwd_aff':
        with torch.no_grad():
            prev = ops.set_x3(False)
            try:
                mat = ops.conv2d(ops.instnorm_style(ag, stg, EPS), T.wt.cuda(), None, scale=f.scale, padding=1, up=f.kind == 'up')
            finally:
                ops.set_x3(prev)
        ed, em = _rms(got[0], want), _rms(mat, want)
        print(f'mod | row {name} {regime}: rms error deferred {ed:.3e}, materialised {em:.3e}, deferred / materialised {ed / max(em, 1e-300):.2f}')


# ==== the closing census =============================================================================================================
def test_every_mod_kernel_is_accounted_for():
    """Every ``__global__`` kernel of csrc/mod.hip is either in this module's ``REQUIRED`` or the symbol of a row of
    tests/exact_forms.py (or a finish kernel in a row's plan), and every ``REQUIRED`` symbol was launched by the tests above - so
    run with the whole module, in file order, in one process."""
    import gan_lab_amd
    src = open(os.path.join(os.path.dirname(gan_lab_amd.__file__), 'csrc', 'mod.hip')).read()
    kernels = re.findall(r'__global__[^;{]*?void\s+(\w+)\s*\(', src)
    assert len(kernels) >= 8, kernels
    table = {re.sub(r'<.*', '', sym) for r in E.ROWS.values() for sym, _ in r.plan}
    orphan = [k for k in kernels if k not in REQUIRED and k not in table]
    assert not orphan, orphan
    assert all(k in kernels and k in E.NOT_CONV for k in REQUIRED)
    missing = [k for k in REQUIRED if not any(k in s for s in SEEN)]
    assert not missing, missing
