"""The radial power-spectrum metric on the GPU (csrc/spectrum.hip, gan_lab_amd/spectrum.py) against the float64
numpy restatement of its definition (tests/spectrum_reference.py).

The accuracy bar.  The yardstick of a case is the error of the SAME restatement with the window product and the transform in fp32
(torch.fft.fft2 on a CPU complex64 tensor) against float64 on the same inputs; a per-bin relative error passes if
|gpu - f64| / f64 <= max(1e-6, 10 x the yardstick's largest per-bin relative error).  The factor 10 covers a different summation
order, fma contraction and a different FFT factorisation, nothing else.  On the CPU the yardstick was 1.0e-7 .. 4.3e-7 over the
sizes, kinds and windows below, so the floor of 1e-6 is the bar nearly everywhere.  Every test prints the GPU error next to its
yardstick before it asserts.

Measured on an MI355X (largest per-bin relative error of the GPU profile against float64 / the fp32 yardstick's, over the cases of
test_profiles_match_float64; DESIGN.md 4.9 has the table):
    R = 16    0.8e-7 .. 5.0e-7 / 1.0e-7 .. 5.0e-7        R = 32    1.2e-7 .. 4.6e-7 / 0.9e-7 .. 4.6e-7
    R = 64    1.5e-7 .. 1.0e-6 / 1.2e-7 .. 1.0e-6        R = 256   1.4e-7 .. 1.5e-6 / 1.2e-7 .. 1.5e-6
    R = 1024  1.6e-7 / 1.2e-7 (natural, hann, N = 2)
Every figure above 5e-7 is bin 0 (DC alone) of white noise with 37 images, where the 3 R^2 zero-mean samples nearly cancel and the GPU
and the yardstick agree to the printed digits; away from DC the GPU stays below 2.1e-7 and within 1.5 x the yardstick.  Tones:
peak bin within 1.0e-7 (relative to the peak), Nyquist tones exact.  Distances of two 16-image sets: 1.2e-8 .. 7e-8 relative.
"""
import functools
import math

import numpy as np
import pytest
import torch

import spectrum_reference as ref

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(device='cuda', dtype=dtype)        # (a copy: the shared cases are read-only)


def _bar(f32, f64, scale=None):
    """max(1e-6, 10 x the yardstick's largest error), errors relative per entry (or to ``scale``)."""
    f32, f64 = np.asarray(f32, dtype=np.float64), np.asarray(f64, dtype=np.float64)
    err = np.abs(f32 - f64) / (np.abs(f64) if scale is None else scale)
    return max(1e-6, 10. * float(err.max()))


@functools.lru_cache(maxsize=None)
def _case(kind, n, res, seed, window):
    """(images, float64 profiles, fp32 yardstick profiles): computed once, shared, never modified."""
    x = ref.sample(kind, n, res, seed)
    want, yard = ref.profiles(x, window), ref.profiles_fp32(x, window)
    for a in (x, want, yard):
        a.setflags(write=False)
    return x, want, yard


def _check_profiles(kind, n, res, window):
    from gan_lab_amd import spectrum
    x, want, yard = _case(kind, n, res, 2000 + res, window)
    # on the reference alone: the dynamic range of these inputs is at most 56 dB, so no bin is near zero
    assert want.min() > 0. and 10. * math.log10(want.max() / want.min()) <= 56.
    got = spectrum.profiles(_dev(x), window).cpu().numpy()
    assert got.shape == (n, res // 2 + 1) and got.dtype == np.float64
    err, bar = np.abs(got - want) / want, _bar(yard, want)
    print(f'{kind} {window} R={res} N={n}: gpu max rel err {err.max():.2e} (bin {int(err.max(axis=0).argmax())}); fp32 yardstick '
          f'{(np.abs(yard - want) / want).max():.2e}; bar {bar:.2e}')
    assert err.max() <= bar, (kind, window, res, n, float(err.max()), bar)


# N = 37: an odd count and, at 256^2, more workgroups than the chip holds at once (14208 row and 333 column workgroups).
# R = 16: a row shorter than a wavefront, every column in one tile; 32: an odd log2 (the radix-2 tail); 256: 9 column tiles, the
# last with one live column.
@pytest.mark.parametrize('n', [1, 3, 37])
@pytest.mark.parametrize('window', ['hann', 'none'])
@pytest.mark.parametrize('kind', ['noise', 'natural'])
@pytest.mark.parametrize('res', [16, 32, 64, 256])
def test_profiles_match_float64(res, kind, window, n):
    _check_profiles(kind, n, res, window)


def test_profiles_match_float64_at_1024():
    """The largest tile: one transform per row workgroup, 4 columns per column workgroup, 129 tiles per image."""
    _check_profiles('natural', 2, 1024, 'hann')


@pytest.mark.parametrize('res', [16, 64])
def test_tones_land_in_their_bin(res):
    """Window 'none', one channel a pure cosine.  The reference puts all power in one bin ((3, 4) -> bin 5; the corner tone in no
    kept bin, and at R = 16 neither (3, 8) nor (8, 3), whose radius 8.54 rounds to 9); errors are relative to the largest bin
    (a dropped tone: to the image's mean square), since the other bins are empty.  Columns / rows 0 and R/2 carry the half-spectrum weight 1, everything between them 2: these cases pin that."""
    from gan_lab_amd import spectrum
    h = res // 2
    tones = [(3, 4), (0, 5), (5, 0), (0, h), (h, 0), (3, h), (h, 3), (h, h)]
    x = np.stack([ref.tone(res, ku, kv, m % 3) for m, (ku, kv) in enumerate(tones)])
    want, yard = ref.profiles(x, 'none'), ref.profiles_fp32(x, 'none')
    got = spectrum.profiles(_dev(x), 'none').cpu().numpy()
    for m, (ku, kv) in enumerate(tones):
        msq = float((x[m].astype(np.float64) ** 2).mean())
        k = int(math.floor(math.hypot(ku, kv) + 0.5))
        assert (ku, kv) != (3, 4) or k == 5
        assert (ku, kv) != (h, h) or k > h
        # the samples are rounded to fp32: (2^-24)^2 ~ 4e-15 of the power is rounding noise spread over the other coefficients
        if k > h:                                  # a dropped corner ((R/2, R/2); at R = 16 also (3, 8) and (8, 3)): no kept bin
            assert want[m].max() <= 1e-12 * msq
            scale = msq
        else:
            assert int(want[m].argmax()) == k and want[m].sum() - want[m, k] <= 1e-12 * want[m, k]
            scale = float(want[m].max())
        err, bar = np.abs(got[m] - want[m]).max() / scale, _bar(yard[m], want[m], scale)
        print(f'R={res} tone {(ku, kv)}: peak {want[m].max():.6g} gpu {got[m].max():.6g} err/scale {err:.2e} bar {bar:.2e}')
        assert err <= bar, (res, ku, kv, err, bar)


@pytest.mark.parametrize('res', [16, 64])
def test_transposed_flipped_and_shifted_images_give_the_same_profile(res):
    """The profile is invariant under transposition (either window) and, without a window, under flips and circular shifts.
    The periodic Hann window is symmetric about i = 0, not about the image centre (a flip maps sample i to R-1-i, not to -i), so
    under 'hann' a flipped image is another windowed image: it is compared with the reference of the flipped image instead."""
    from gan_lab_amd import spectrum
    x, want, yard = _case('natural', 3, res, 2000 + res, 'hann')
    bar = _bar(yard, want)
    got = spectrum.profiles(_dev(x.transpose(0, 1, 3, 2)), 'hann').cpu().numpy()
    print(f'R={res} hann transposed against the unmoved image: {(np.abs(got - want) / want).max():.2e} bar {bar:.2e}')
    assert (np.abs(got - want) / want).max() <= bar
    variants = {'transposed': x.transpose(0, 1, 3, 2), 'flipped rows': x[:, :, ::-1], 'flipped columns': x[:, :, :, ::-1]}
    for name, v in variants.items():
        w = ref.profiles(np.ascontiguousarray(v), 'hann')
        got = spectrum.profiles(_dev(v), 'hann').cpu().numpy()
        err = (np.abs(got - w) / w).max()
        print(f'R={res} {name}: err {err:.2e} bar {bar:.2e}')
        assert err <= bar
    base = ref.profiles(x, 'none')
    bar = _bar(ref.profiles_fp32(x, 'none'), base)
    assert (np.abs(ref.profiles(np.ascontiguousarray(x.transpose(0, 1, 3, 2)), 'none') - base) / base).max() < 1e-12
    for name, v in dict(variants, shifted=np.roll(x, (5, res - 3), axis=(2, 3))).items():
        got = spectrum.profiles(_dev(v), 'none').cpu().numpy()
        err = (np.abs(got - base) / base).max()
        print(f'R={res} none {name}: err against the unmoved image {err:.2e} bar {bar:.2e}')
        assert err <= bar


def _evaluate(ps, x, batch):
    ps.reset()
    for i in range(0, len(x), batch):
        ps.feed(x[i:i + batch])
    return ps


@pytest.mark.parametrize('window', ['hann', 'none'])
def test_scaling_by_two_is_exactly_a_factor_four(window):
    from gan_lab_amd import spectrum
    x = _dev(_case('natural', 3, 64, 2064, 'hann')[0])
    a, b = spectrum.profiles(x, window), spectrum.profiles(x * 2, window)
    assert torch.equal(b, a * 4) and bool((a > 0).all())
    fake = _evaluate(spectrum.PowerSpectrum(64, 3, window), x * 2, 3)
    real = _evaluate(spectrum.PowerSpectrum(64, 3, window), x, 3)
    d = spectrum.distance(fake, real)
    want = 20. * math.log10(2.)
    print(f'{window}: distance(2x, x) = {d["spectrum"]!r} / {d["hf"]!r}, 20 log10 2 = {want!r}')
    assert abs(d['spectrum'] - want) <= 1e-12 and abs(d['hf'] - want) <= 1e-12 and d['images'] == 3


def test_results_are_bitwise_reproducible_and_independent_of_feeds_and_chunks(monkeypatch):
    from gan_lab_amd import ops, spectrum
    x = _dev(_case('natural', 37, 64, 2064, 'hann')[0])
    ps = spectrum.PowerSpectrum(64, 37)
    whole = _evaluate(ps, x, 37).profile()
    rows = ps.per_image().clone()
    assert torch.equal(rows, spectrum.profiles(x))
    assert _evaluate(ps, x, 37).profile() == whole and torch.equal(ps.per_image(), rows)       # twice in the same buffers
    assert _evaluate(spectrum.PowerSpectrum(64, 37), x, 37).profile() == whole                  # ... and in fresh ones
    for batch in (4, 1):
        assert _evaluate(ps, x, batch).profile() == whole and torch.equal(ps.per_image(), rows)
    d = spectrum.distance(ps, _evaluate(spectrum.PowerSpectrum(64, 37), x, 4))
    assert d['spectrum'] == 0.0 and d['hf'] == 0.0 and d['fake_db'] == d['real_db'] == whole['db']
    # a feed larger than the scratch is walked in chunks: 5 images per chunk here, 37 = 7 x 5 + 2
    per_image = ops.spectrum_scratch_bytes(2, 64) - ops.spectrum_scratch_bytes(1, 64)
    monkeypatch.setattr(spectrum, '_SCRATCH_BYTES', 5 * per_image)
    small = spectrum.PowerSpectrum(64, 37)
    assert small._chunk == 5 and _evaluate(small, x, 37).profile() == whole and torch.equal(small.per_image(), rows)
    # a non-contiguous feed is copied, not misread; an empty feed is accepted
    y = torch.cat([x, x], dim=1)[:, :3]
    assert not y.is_contiguous()
    ps.reset()
    ps.feed(y[:0])
    ps.feed(y)
    assert ps.profile() == whole


@pytest.mark.parametrize('res', [32, 64, 256])
def test_end_to_end_matches_the_float64_reference(res):
    from gan_lab_amd import spectrum
    xf, xr = ref.sample('natural', 16, res, 10 + res), ref.sample('natural', 16, res, 20 + res)
    pf, pr = ref.profiles(xf), ref.profiles(xr)
    want, yard = ref.distance(pf, pr), ref.distance(ref.profiles_fp32(xf), ref.profiles_fp32(xr))
    fake = _evaluate(spectrum.PowerSpectrum(res, 16), _dev(xf), 4)
    real = _evaluate(spectrum.PowerSpectrum(res, 16), _dev(xr), 16)
    got = spectrum.distance(fake, real)
    assert got['images'] == 16 and len(got['fake_db']) == len(got['real_db']) == res // 2 + 1
    for key in ('spectrum', 'hf'):
        err, bar = abs(got[key] - want[key]) / want[key], _bar(yard[key], want[key])
        print(f'R={res} {key}: gpu {got[key]:.12g} reference {want[key]:.12g} rel err {err:.2e} (fp32 yardstick '
              f'{abs(yard[key] - want[key]) / want[key]:.2e}) bar {bar:.2e}')
        assert want[key] > 0.05 and err <= bar
    prof = fake.profile()
    s, db = ref.decibels(pf)
    assert (np.abs(np.array(prof['power']) - s) / s).max() <= _bar(ref.decibels(ref.profiles_fp32(xf))[0], s)
    # d(10 log10 S) = 10 / ln 10 x dS / S
    assert np.abs(np.array(prof['db']) - db).max() <= 10. / math.log(10.) * _bar(ref.decibels(ref.profiles_fp32(xf))[0], s) + 1e-12
    assert prof['db'] == got['fake_db']


def test_an_all_zero_set_reads_minus_300_db():
    from gan_lab_amd import spectrum
    z = torch.zeros(2, 3, 32, 32, device='cuda')
    ps = _evaluate(spectrum.PowerSpectrum(32, 2), z, 2)
    out = ps.profile()
    assert out['power'] == [0.0] * 17 and out['db'] == [-300.0] * 17
    d = spectrum.distance(ps, _evaluate(spectrum.PowerSpectrum(32, 2), z, 1))
    assert d['spectrum'] == 0.0 and d['hf'] == 0.0


def test_argument_checks_on_the_device():
    from gan_lab_amd import ops, spectrum
    from gan_lab_amd._lib import GanlabLibraryError
    x = torch.zeros(4, 3, 32, 32, device='cuda')
    ws, scratch = ops.spectrum_workspace(4, 32, 'cuda'), ops.spectrum_scratch(4, 32, 'cuda')
    with pytest.raises(ValueError):
        ops.spectrum_feed(x, 64, 'hann', scratch, ws, 0, 4)                     # images are not 64 x 64
    with pytest.raises(ValueError):
        ops.spectrum_feed(x, 32, 'hamming', scratch, ws, 0, 4)
    with pytest.raises(GanlabLibraryError, match='EINVAL'):
        ops.spectrum_feed(x, 32, 'hann', scratch, ws, 1, 4)                     # images 1 .. 4 of an evaluation of 4
    with pytest.raises(GanlabLibraryError, match='EWORKSPACE'):
        ops.spectrum_feed(x, 32, 'hann', scratch[:64], ws, 0, 4)
    with pytest.raises(GanlabLibraryError, match='EWORKSPACE'):
        ops.spectrum_feed(x, 32, 'hann', scratch, ws.view(-1)[:17], 0, 4)
    big = torch.zeros(1, 3, 2048, 2048, device='cuda')
    with pytest.raises(GanlabLibraryError, match='EUNSUPPORTED'):
        ops.spectrum_feed(big, 2048, 'hann', scratch, ws, 0, 1)
    with pytest.raises(ValueError, match='power of two'):
        spectrum.profiles(torch.zeros(2, 3, 8, 8, device='cuda'))
    with pytest.raises(ValueError, match='share'):
        spectrum.distance(spectrum.PowerSpectrum(32, 2), spectrum.PowerSpectrum(32, 4))
    with pytest.raises(ValueError, match='2 images were declared, 0 were fed'):
        spectrum.PowerSpectrum(32, 2).profile()


# ---- learner -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def _widths():
    from gan_lab_amd import progressive as P
    P.FMAP_BASE, P.FMAP_MAX = 64, 16
    yield
    P.FMAP_BASE, P.FMAP_MAX = 8192, 512


class _ZLoader(object):
    def __init__(self, batches):
        self.batches, self.dataset = batches, list(range(sum(len(b[0]) for b in batches)))
        self.batch_sampler = type('S', (), {'batch_size': len(batches[0][0])})()

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _run_learner(kind, gen_metrics, init_res, res):
    """One training iteration with validation at iteration 0: 8 validation latents and 8 reals in batches of 4.  Returns the
    learner and one record per compute_metrics call: resolution, last_metrics, lines, the process stream's offset before and
    after, and the generator forwards (snapshot and time-averaged) the call ran."""
    from gan_lab_amd import rng
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    torch.manual_seed(7)
    np.random.seed(7)
    L = make_learner(kind, res, init_res=init_res, batch=4, loss='nonsaturating', gradient_penalty='r1', num_iters_valid=2,
                     gen_metrics=gen_metrics, disc_metrics=[], random_seed=4, swd_nhoods=16, swd_dir_repeats=2,
                     swd_dirs_per_repeat=32)
    gen = torch.Generator().manual_seed(9)
    z_dl = _ZLoader([(torch.randn(4, 16, generator=gen),) for _ in range(2)])
    x_dl = SyntheticImageLoader(8, 4, init_res, seed=1)
    seen, forwards = [], []
    gen_class = type(L.gen_model)
    hook = torch.nn.modules.module.register_module_forward_hook(
        lambda mod, args, out: forwards.append(mod) if isinstance(mod, gen_class) else None)
    orig = L.compute_metrics

    def spy(*a, **kw):
        before, n0 = rng._STATE['offset'], len(forwards)
        lines = orig(*a, **kw)
        seen.append(dict(res=int(L.gen_model.curr_res), metrics=dict(L.last_metrics['generator']), lines=lines,
                         offsets=(before, rng._STATE['offset']), forwards=len(forwards) - n0))
        return lines
    L.compute_metrics = spy
    try:
        L.train(SyntheticImageLoader(4096, 4, init_res), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=1)
    finally:
        hook.remove()
    return L, seen


def test_learner_reports_the_spectrum_lines_with_one_extra_forward(_widths, capsys):
    L, seen = _run_learner('stylegan', ['generator loss', 'swd', 'msssim', 'spectrum'], 16, 16)
    out = capsys.readouterr().out
    (rec,) = seen
    names = [ln.split(':')[0].strip() for ln in rec['lines']]
    assert names == ['generator loss', 'swd 16x16', 'swd mean', 'msssim fake', 'msssim real', 'spectrum', 'spectrum hf']
    assert out.count('spectrum:') == 1 and out.count('spectrum hf:') == 1
    d = rec['metrics']['spectrum']
    assert d == L.last_metrics['generator']['spectrum']
    assert d['images'] == 8 and len(d['fake_db']) == len(d['real_db']) == 9
    assert all(math.isfinite(v) for v in d['fake_db'] + d['real_db'] + [d['spectrum'], d['hf']])
    assert d['spectrum'] > 0. and d['hf'] > 0.
    for line, key in ((rec['lines'][5], 'spectrum'), (rec['lines'][6], 'hf')):
        assert abs(float(line.split(':')[1]) - d[key]) <= 1e-3 * d[key]
    # the three metrics shared ONE forward of the time-averaged generator per batch: 2 batches x (snapshot + time-averaged) = 4,
    # not 2 x (1 + 3)
    assert L.config.use_ewma_gen and rec['forwards'] == 4
    assert L.gen_model.training and L.disc_model.training
    # alone, the metric gives the same numbers (it scores the same images) ...
    L1, seen1 = _run_learner('stylegan', ['generator loss', 'spectrum'], 16, 16)
    assert seen1[0]['metrics']['spectrum'] == d and seen1[0]['forwards'] == 4
    assert [ln.split(':')[0].strip() for ln in seen1[0]['lines']] == ['generator loss', 'spectrum', 'spectrum hf']
    # ... and training does not notice it
    L0, seen0 = _run_learner('stylegan', ['generator loss'], 16, 16)
    assert 'spectrum' not in seen0[0]['metrics'] and seen0[0]['forwards'] == 2
    # the process stream stands where it stands without the metrics (the snapshot generator's own noise draws advance it in
    # both runs; the time-averaged generator's extra forward gives its draws back)
    assert rec['offsets'] == seen0[0]['offsets'] == seen1[0]['offsets'] and rec['offsets'][1] > rec['offsets'][0]
    assert seen0[0]['metrics']['generator loss'] == rec['metrics']['generator loss']
    assert torch.equal(L0.arena_g.flat, L.arena_g.flat) and torch.equal(L0.arena_d.flat, L.arena_d.flat)


def test_below_sixteen_the_line_is_nan_and_nothing_raises(_widths):
    L, seen = _run_learner('progan', ['generator loss', 'spectrum'], 8, 32)
    (rec,) = seen
    d = rec['metrics']['spectrum']
    assert rec['res'] == 8 and math.isnan(d['spectrum']) and math.isnan(d['hf']) and d['images'] == 0
    assert len(rec['lines']) == 2 and 'nan' in rec['lines'][1] and '16x16' in rec['lines'][1] and '8x8' in rec['lines'][1]


def test_compute_metrics_checks_on_the_device(_widths):
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    L = make_learner('progan', 16, init_res=16, batch=4, gen_metrics=['spectrum'], use_ewma_gen=False)
    z_dl = _ZLoader([(torch.randn(4, 16),) for _ in range(2)])
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['spectrum'], 'Discriminator', z_dl, SyntheticImageLoader(8, 4, 16))
    with pytest.raises(ValueError, match='valid_dl'):
        L.compute_metrics(['spectrum'], 'Generator', z_dl)
    lines = L.compute_metrics(['spectrum'], 'Generator', z_dl, SyntheticImageLoader(8, 4, 16))
    assert [ln.split(':')[0].strip() for ln in lines] == ['spectrum', 'spectrum hf']
    assert L.last_metrics['generator']['spectrum']['images'] == 8
    first = L._metric_evals['spectrum']
    L.compute_metrics(['spectrum'], 'Generator', z_dl, SyntheticImageLoader(8, 4, 16))
    assert L._metric_evals['spectrum'] is first                                 # cached per (res, n)
    with pytest.raises(ValueError, match='whole batch'):
        L.compute_metrics(['spectrum'], 'Generator', _ZLoader([(torch.randn(2, 16),)]), SyntheticImageLoader(8, 4, 16))
