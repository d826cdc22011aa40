"""The power-spectrum regulariser on the GPU (csrc/spectrum.hip, gan_lab_amd/_ops/metrics.py, gan_lab_amd/spectrum_reg.py; DESIGN.md
4.9b) against the float64 restatement of its definition (tests/spectrum_reg_reference.py).

The accuracy bar.  The yardstick of a case is the error of the SAME restatement run entirely in float32 on the CPU (torch.fft on
complex64, fp32 bin sums and logarithms) against float64 on the same inputs.  For the loss (absolute error), for dx (largest
absolute error) and for the relative L2 error of dx, the GPU's error against float64 may be at most 2 x the yardstick's: both are
correctly ordered fp32 transforms, the kernels' bin sums are fp64, and the factor 2 covers a different butterfly order.  Every test
prints the GPU error next to its yardstick before it asserts.

The first run on an MI355X met the factor 2 for dx in all 24 cases (largest ratio 1.03 for the largest error, 0.93 for the relative
L2 error) and missed it for the loss in 6 of them.  The loss is ONE fp32 number: the GPU's error was 0.3e-9 .. 6.8e-8 over the cases
and the yardstick's 0.4e-9 .. 1.6e-7, each a fraction of an ulp up to a few ulps of L (1.5e-8 at L = 0.13), so the ratio of the two in
a single case is a matter of which way two roundings fell (39 where the yardstick's own error happened to be 3.7e-10, a fortieth
of an ulp).  As the issue provides for this outcome, both errors are recorded per shape in DESIGN.md 4.9b and the loss's bar in each
of the six shapes is its measured ratio x 1.5 (``LOSS_PARITY`` below); the other 18 shapes, and dx in all 24, keep the factor 2.

Shapes: R = 16 (even log2, the smallest size, 64 row pairs per workgroup, one column tile), R = 32 (odd log2: the trailing radix-2
stage; 17 columns are the first size with more than one 16-column tile), R = 64 (three tiles, the last with one live column); N = 1
and N = 3; both windows and both bands.  Inputs are smooth images plus white noise of std 0.1, so every bin is far above the 1e-30
floor (checked in float64 on the CPU side)."""
import functools

import numpy as np
import pytest
import torch

import spectrum_reg_reference as ref

pytestmark = pytest.mark.gpu

PARITY = 2.0
# (R, N, window, band): measured ratio x 1.5 where the first run exceeded 2 (the module docstring; DESIGN.md 4.9b has the table)
LOSS_PARITY = {
    (16, 1, 'hann', 'all'): 4.13,      # 2.75
    (16, 1, 'hann', 'hf'): 4.73,       # 3.16
    (16, 3, 'none', 'hf'): 4.40,       # 2.94
    (32, 1, 'hann', 'all'): 58.86,      # 39.24
    (32, 3, 'hann', 'hf'): 4.86,       # 3.24
    (64, 1, 'hann', 'hf'): 3.04,       # 2.03
}


@functools.lru_cache(maxsize=None)
def _case(n, res, window, band):
    """(x, T, L64, dx64, L32, dx32): computed once, shared, never modified."""
    x = ref.smooth_noisy(n, res, seed=100 + res + n)
    k = torch.arange(res // 2 + 1, dtype=torch.float64)
    t = ref.set_profile(ref.smooth_noisy(n, res, seed=200 + res + n), window) * (1. + 0.5 * torch.sin(k))
    s = ref.set_profile(x, window)
    assert float(s.min()) > 1e-8 and float(t.min()) > 1e-8         # far above the floor
    L64, d64 = ref.loss_and_grad(x, t, band, window)
    L32, d32 = ref.loss_and_grad(x, t, band, window, dtype=torch.float32)
    assert float(L64) > 1e-3 and float(d64.abs().max()) > 0.
    return x, t, L64, d64, L32, d32


def _hip(x, t, band, window, grad_out=None, **kw):
    from gan_lab_amd import ops
    xd = x.cuda().requires_grad_(True) if not x.is_cuda else x
    L = ops.spectrum_loss(xd, t if t.is_cuda else t.cuda(), band, window, **kw)
    assert L.shape == () and L.dtype == torch.float32 and L.is_cuda
    g, = torch.autograd.grad(L if grad_out is None else grad_out * L, xd)
    return L.detach(), g


def _errors(L, dx, L64, d64):
    dx = dx.double().cpu()
    return abs(float(L) - float(L64)), float((dx - d64).abs().max()), float((dx - d64).norm() / d64.norm())


@pytest.mark.parametrize('band', ref.BANDS)
@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('res', [16, 32, 64])
def test_loss_and_gradient_match_float64(res, n, window, band):
    x, t, L64, d64, L32, d32 = _case(n, res, window, band)
    L, dx = _hip(x, t, band, window)
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_contiguous()
    got, yard = _errors(L, dx, L64, d64), _errors(L32, d32, L64, d64)
    print(f'R={res} N={n} {window} {band}: L={float(L64):.6g} max|dx|={float(d64.abs().max()):.3e}  gpu err (L, dx max, dx rel L2) = '
          f'{got[0]:.3e} {got[1]:.3e} {got[2]:.3e}; fp32 cpu = {yard[0]:.3e} {yard[1]:.3e} {yard[2]:.3e}; ratios '
          + ' '.join(f'{g / max(y, 1e-300):.2f}' for g, y in zip(got, yard)))
    for what, g, y in zip(('loss', 'dx max', 'dx rel L2'), got, yard):
        bar = LOSS_PARITY.get((res, n, window, band), PARITY) if what == 'loss' else PARITY
        assert g <= bar * y, (what, res, n, window, band, g, y, bar)


def test_cotangent_scales_the_gradient():
    x, t, _, d64, _, d32 = _case(3, 32, 'hann', 'all')
    _, dx = _hip(x, t, 'all', 'hann', grad_out=-1.75)
    got = float((dx.double().cpu() + 1.75 * d64).norm() / (1.75 * d64).norm())
    yard = float((d32.double() - d64).norm() / d64.norm())
    print(f'cotangent -1.75: gpu rel L2 {got:.3e}; fp32 cpu {yard:.3e}')
    assert got <= PARITY * yard


@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('res,n', [(16, 3), (32, 3), (64, 1)])
def test_own_profile_gives_exact_zero(res, n, window):
    from gan_lab_amd import ops
    x = _case(n, res, window, 'all')[0].cuda()
    t = ops.spectrum_profile_mean(x, window)
    assert t.shape == (res // 2 + 1,) and t.dtype == torch.float64 and t.is_cuda
    want = ref.set_profile(x.cpu(), window)
    assert float(((t.cpu() - want).abs() / want).max()) < 1e-5
    for band in ref.BANDS:
        L, dx = _hip(x.clone().requires_grad_(True), t, band, window)
        assert float(L) == 0.0 and float(dx.abs().max()) == 0.0 and bool(torch.isfinite(dx).all())


@pytest.mark.parametrize('band', ref.BANDS)
def test_a_constant_offset_changes_nothing_without_a_window(band):
    """DC is outside every band, so with window='none' x + c has the loss and the gradient of x beyond fp32 rounding of the DC
    coefficient.  To see that rounding and nothing else, the images are multiples of 2^-12 below 2 in magnitude and c = 0.5: x + c is
    exact in fp32, so every implementation is handed the same shifted batch and float64 sees no change at all (asserted).  The bound
    is the issue's: the float32 CPU reference's own change on the same two batches, no factor.  Measured on an MI355X: the GPU's
    change of L and of dx is exactly 0 in both bands, and so is the reference's - the constant cancels exactly in the differences of
    the first butterflies and doubles exactly in their sums, so it reaches the DC coefficient alone in either factorisation.  With
    DC inside a band the change would be of the size of the loss.
    (An earlier form of this test shifted unquantised images by 0.37.  There x + c is rounded, float64 itself changes, and both
    implementations report that common change plus their own noise: GPU 0 / 1.49e-8 for L and 3.84e-9 / 6.05e-9 for dx in the two
    bands against 2.98e-8 / 0 and 4.19e-9 / 5.70e-9 of the reference - a coin flip against this bound for any implementation, which
    was a mistake of the test's design, not a property of the kernels.)"""
    x = (ref.smooth_noisy(3, 32, seed=41) * 4096.).round() / 4096.
    assert float(x.abs().max()) < 2.0
    y = x + 0.5
    assert torch.equal(y.double(), x.double() + 0.5)
    t = ref.set_profile(ref.smooth_noisy(3, 32, seed=42), 'none') * 1.5
    a64, b64 = ref.loss_and_grad(x, t, band, 'none'), ref.loss_and_grad(y, t, band, 'none')
    assert abs(float(a64[0]) - float(b64[0])) <= 1e-12 * float(a64[0]) and float((a64[1] - b64[1]).abs().max()) <= 1e-12 * float(
        a64[1].abs().max())
    a32, b32 = (ref.loss_and_grad(v, t, band, 'none', dtype=torch.float32) for v in (x, y))
    yard = abs(float(a32[0]) - float(b32[0])), float((a32[1] - b32[1]).abs().max())
    (La, da), (Lb, db) = _hip(x, t, band, 'none'), _hip(y, t, band, 'none')
    assert float(La) > 1e-3 and float(da.abs().max()) > 0.
    got = abs(float(La) - float(Lb)), float((da - db).abs().max())
    print(f'offset 0.5, {band}: gpu change (L, dx max) = {got[0]:.3e} {got[1]:.3e}; fp32 cpu = {yard[0]:.3e} {yard[1]:.3e}')
    assert got[0] <= yard[0] and got[1] <= yard[1]


def test_reproducible_target_untouched_and_first_order_only():
    from gan_lab_amd import ops
    x, t = _case(3, 32, 'hann', 'hf')[:2]
    td = t.cuda().requires_grad_(True)
    keep = td.detach().clone()
    runs = []
    for _ in range(2):
        xd = x.cuda().requires_grad_(True)
        L = ops.spectrum_loss(xd, td, 'hf', 'hann')
        L.backward()
        runs.append((L.detach().clone(), xd.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # bitwise
    assert td.grad is None and torch.equal(td.detach(), keep)
    xd = x.cuda().requires_grad_(True)
    g, = torch.autograd.grad(ops.spectrum_loss(xd, td, 'hf', 'hann'), xd, create_graph=True)
    assert torch.equal(g.detach(), runs[0][1])
    with pytest.raises(RuntimeError, match='first order only'):
        g.square().sum().backward()
    with pytest.raises(ValueError, match='target must hold'):
        ops.spectrum_loss(xd, td[:-1])
    with pytest.raises(ValueError, match='power of two'):
        ops.spectrum_loss(torch.zeros(1, 3, 8, 8, device='cuda'), torch.zeros(5, dtype=torch.float64, device='cuda'))


def test_batch_slices_and_chunks_are_the_whole_batch():
    """A slice along dim 0 is walked by its image stride, not copied; a batch larger than the scratch chunk is walked in chunks;
    anything else is made contiguous.  All are bitwise the contiguous, unchunked result (checked against float64 above)."""
    from gan_lab_amd import ops
    x, t = _case(3, 32, 'hann', 'all')[:2]
    L0, d0 = _hip(x, t, 'all', 'hann')
    both = torch.zeros(6, 3, 32, 32)
    both[0::2] = x
    both[1::2] = 7.0
    both = both.cuda().requires_grad_(True)
    view = both[0::2]
    assert not view.is_contiguous() and view.stride(0) == 2 * 3 * 32 * 32
    L = ops.spectrum_loss(view, t.cuda(), 'all', 'hann')
    g, = torch.autograd.grad(L, both)
    assert torch.equal(L, L0) and torch.equal(g[0::2], d0) and float(g[1::2].abs().max()) == 0.0
    for chunk in (1, 2):
        Lc, dc = _hip(x, t, 'all', 'hann', chunk=chunk)
        assert torch.equal(Lc, L0) and torch.equal(dc, d0)
    assert torch.equal(ops.spectrum_profile_mean(view.detach(), 'hann', chunk=2), ops.spectrum_profile_mean(x.cuda(), 'hann'))
    perm = x.permute(0, 1, 3, 2).contiguous().cuda().permute(0, 1, 3, 2).requires_grad_(True)      # column-major planes: copied
    assert not perm.is_contiguous()
    Lp = ops.spectrum_loss(perm, t.cuda(), 'all', 'hann')
    gp, = torch.autograd.grad(Lp, perm)
    assert torch.equal(Lp, L0) and torch.equal(gp, d0)


# ---- the learner ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def small_widths():
    from gan_lab_amd import progressive as P
    found = P.FMAP_BASE, P.FMAP_MAX
    P.FMAP_BASE, P.FMAP_MAX = 64, 16
    yield
    P.FMAP_BASE, P.FMAP_MAX = found


def _learner(res=16, strip=False, **kw):
    from gan_lab_amd import rng
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    torch.manual_seed(3)
    np.random.seed(3)
    rng.manual_seed(5)
    cfg = make_config('stylegan', dev='cuda', pin_memory=False, res_samples=res, res_dataset=res, init_res=res, batch_size=4,
                      len_latent=16, len_dlatent=16, mapping_num_fcs=2, cutoff_trunc_trick=None, nimg_transition=24,
                      num_iters_save_model=10 ** 9, log_every=0, loss='nonsaturating', gradient_penalty='r1', random_seed=3,
                      pct_mixing_reg=0., **kw)
    if strip:           # the config as it was before the fields existed
        for k in ('spectrum_reg', 'spectrum_reg_band', 'spectrum_reg_decay'):
            delattr(cfg, k)
    L = StyleGANLearner(cfg)
    L.beta = 0.999          # train() sets the EWMA generator's decay; the steps are driven by hand here
    return L


def _inputs(res=16):
    g = torch.Generator().manual_seed(9)
    real = ref.smooth_noisy(4, res, seed=77).cuda()
    return real, torch.randn(4, 16, generator=g).cuda(), torch.randn(4, 16, generator=g).cuda()


def _steps(L, res=16, cotangent=None):
    """d_step + g_step from fixed seeds -> (loss_d, loss_g, critic gradient arena, generator gradient arena, the fakes the
    regulariser saw)."""
    from gan_lab_amd import rng
    real, zd, zg = _inputs(res)
    rng.manual_seed(11)
    seen = []
    if L.spectrum_reg is not None:
        inner = L.spectrum_reg.loss

        def spy(fake):
            seen.append(fake.detach().clone())
            out = inner(fake)
            if cotangent is not None and out is not None:
                out.register_hook(lambda g: g * cotangent)
            return out
        L.spectrum_reg.loss = spy
    L.set_requires_grad_disc(True)
    ld = L.d_step(real, zb=zd)
    gd = L.arena_d.gflat.detach().clone()
    L.set_requires_grad_disc(False)
    lg = L.g_step(zb=zg)
    gg = L.arena_g.gflat.detach().clone()
    torch.cuda.synchronize()
    return ld.clone(), lg.clone(), gd, gg, seen


def test_learner_off_is_the_learner_before_the_fields(small_widths):
    a, b = _steps(_learner(strip=True)), _steps(_learner())
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)
    assert float(a[3].abs().max()) > 0 and float(a[2].abs().max()) > 0


def test_learner_term_linearity_and_critic_untouched(small_widths):
    """grad_g(w) = adversarial + w x the term's gradient: grad_g(2) - grad_g(0) = 2 (grad_g(1) - grad_g(0)) up to the fp32 rounding
    of the generator backward.  The measurement the tolerance was to be taken from - grad_g(1) once as it is and once with weight 2
    and the term's cotangent halved - is printed, but it is exactly zero (scaling by a power of two is exact in fp32), so the
    tolerance is set by reasoning instead: the three runs differ by the rounding of ``d_adv + w d_term`` at the image and of every
    sum behind it, each relative 2^-24 to its operands; with sums of up to 4 x 16 x 16 products per weight and some twenty layers a
    gradient entry carries at most about 1e-5 of the largest gradient of its run, and four runs enter: 4e-5 x the largest |grad_g|.
    The term's own contribution must stand at least a hundred times above that for the check to mean anything.
    Measured on an MI355X: max |d2 - 2 d1| = 4.30e-2 against the tolerance 2.91 (largest |grad_g| 7.27e4, so 5.9e-7 of it), with
    max |d2| = 7.35e4; weight 2 with the cotangent halved against weight 1: 0.0."""
    from gan_lab_amd import ops
    off = _steps(_learner())
    runs = {}
    for w in (1.0, 2.0):
        L = _learner(spectrum_reg=w, spectrum_reg_band='all')
        runs[w] = _steps(L)
        ld, lg, gd, gg, seen = runs[w]
        assert torch.equal(gd, off[2]) and torch.equal(ld, off[0])               # the critic step is the off run's, bitwise
        term = L.last_losses['spectrum_reg']
        assert term.is_cuda and term.shape == () and not term.requires_grad and len(seen) == 1
        assert torch.equal(term, ops.spectrum_loss(seen[0], L.spectrum_reg.target, 'all', 'hann'))
        assert torch.equal(lg, (off[1] + w * term)) or abs(float(lg) - float(off[1]) - w * float(term)) <= 1e-6 * abs(float(lg))
        assert float(term) > 0
    halved = _steps(_learner(spectrum_reg=2.0, spectrum_reg_band='all'), cotangent=0.5)
    floor = float((halved[3] - runs[1.0][3]).abs().max())
    d1, d2 = runs[1.0][3] - off[3], runs[2.0][3] - off[3]
    gmax = max(float(r[3].abs().max()) for r in (off, runs[1.0], runs[2.0]))
    err, tol = float((d2 - 2. * d1).abs().max()), 4e-5 * gmax
    print(f'linearity: max |d2 - 2 d1| = {err:.3e}; tolerance {tol:.3e}; max |d2| = {float(d2.abs().max()):.3e}; largest |grad_g| '
          f'{gmax:.3e}; weight 2 with the cotangent halved against weight 1: {floor:.3e}')
    assert float(d2.abs().max()) > 100. * tol
    assert err <= tol


def test_learner_target_follows_the_reals(small_widths):
    """After d_steps on real batches T is the float64 EMA of their reference profiles, to the parity bar: per bin, at most 2 x the
    error of the same EMA of float32 CPU profiles."""
    L = _learner(spectrum_reg=1.0, spectrum_reg_decay=0.5)
    assert not L.step_graph.eligible()                      # with the option on the learner steps eagerly
    assert _learner().step_graph.eligible()
    with pytest.raises(RuntimeError, match='set_target'):
        L.g_step(zb=_inputs()[1])
    reals = [ref.smooth_noisy(4, 16, seed=s) for s in (77, 78, 79)]
    for r in reals:
        L.d_step(r.cuda(), zb=_inputs()[1])
    t = L.spectrum_reg.target
    assert t.dtype == torch.float64 and t.is_cuda and t.shape == (9,)
    want = ref.ema([ref.set_profile(r, 'hann') for r in reals], 0.5)
    yard = ref.ema([ref.set_profile(r, 'hann', dtype=torch.float32).double() for r in reals], 0.5)
    err, bar = ((t.cpu() - want).abs() / want).max(), PARITY * ((yard - want).abs() / want).max()
    print(f'EMA target: gpu max rel err {float(err):.3e}; fp32 cpu {float(bar) / PARITY:.3e}')
    assert float(err) <= float(bar)
    L.spectrum_reg.set_target(reals[0].cuda())
    assert float(((L.spectrum_reg.target.cpu() - ref.set_profile(reals[0], 'hann')).abs() / want).max()) < 1e-5
    L.set_requires_grad_disc(False)
    assert torch.isfinite(L.g_step(zb=_inputs()[2]))
    L.spectrum_reg.reset()
    assert L.spectrum_reg.target is None


def test_learner_launches_nothing_at_8x8(small_widths):
    L = _learner(res=8, spectrum_reg=1.0)
    real, zd, zg = _inputs(8)
    L.d_step(real, zb=zd)
    assert L.spectrum_reg.target is None
    L.set_requires_grad_disc(False)
    L.g_step(zb=zg)
    assert L.last_losses['spectrum_reg'] is None
