"""The MS-SSIM metric on the GPU (csrc/msssim.hip, gan_lab_amd/msssim.py) against the float64 numpy restatement
of its definition (tests/msssim_reference.py).

The accuracy bar.  The yardstick of a case is the error of the SAME restatement run in fp32 numpy against float64 on the same
inputs; a GPU number passes if |gpu - f64| <= max(1e-6, 10 x that fp32 error).  The factor 10 covers a different summation order
and fma contraction, nothing else.  On the CPU the fp32 run's largest error over the (P, 5, 2) table was 5e-9 .. 1.2e-7 over all
twelve (resolution, kind) cases below and at most 4.4e-8 in a pair's final value, so the floor of 1e-6 is the bar nearly
everywhere.  Every test prints the GPU error next to its yardstick before it asserts.  No GPU figure is recorded yet: these tests have not
run on an MI355X, and DESIGN.md 4.8 says the same.

The pooled next level is compared bit for bit with the fp32 restatement (same order of the four additions) and to 1e-6 max |x|
with float64.  End to end only 'near' pairs are used (every CS_i mean above 0.99): a CS_i near the clamp makes the weighted power
ill-conditioned (d/dx x^0.0448 at x = 1e-4 is ~300), which is the definition's property, not the kernel's; the clamp itself has a
test of its own."""
import math

import numpy as np
import pytest
import torch

import msssim_reference as ref

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device='cuda', dtype=dtype)


def _bar(f32, f64):
    return max(1e-6, 10. * float(np.abs(np.asarray(f32) - np.asarray(f64)).max()))


# P = 2: fewer workgroups than the GPU has compute units at every level; P = 37: more than it can hold at once at 256^2 (2368 tiles
# of level 0 alone) and an odd count.  Output sides 6, 22, 54, 246 and 1: none is a multiple of the 32 x 32 tile.
@pytest.mark.parametrize('pairs', [2, 37])
@pytest.mark.parametrize('kind', ['noise', 'smooth', 'near'])
@pytest.mark.parametrize('res', [16, 32, 64, 256])
def test_level_table_matches_float64(res, kind, pairs):
    """Resolutions 16 .. 256 put windows of 11, 8, 4, 2 and 1 taps through the level kernel (16: sides 16, 8, 4, 2, 1)."""
    from gan_lab_amd import msssim
    a, b = ref.sample_pairs(kind, pairs, res, seed=1000 + res)
    values, table = msssim.pairs(_dev(a), _dev(b))
    want, yard = ref.table(a, b), ref.table(a, b, dtype=np.float32)
    got = table.cpu().numpy()
    assert got.shape == (pairs, 5, 2) and got.dtype == np.float64
    err, bar = np.abs(got - want).max(axis=(0, 2)), _bar(yard, want)
    print(f'{kind} {res} P={pairs}: per-level max err {" ".join("%.2e" % e for e in err)}; fp32 numpy '
          f'{np.abs(yard - want).max():.2e}; bar {bar:.2e}')
    assert err.max() <= bar, (res, kind, pairs, err, bar)
    # the weighted product of the table the kernel itself wrote: five fp64 powers, each within a few ulp of numpy's
    assert np.abs(values.cpu().numpy() - ref.combine(got)).max() <= 1e-13


@pytest.mark.parametrize('res', [16, 32, 64, 256])
def test_pooled_levels_are_the_stated_two_by_two_mean(res):
    from gan_lab_amd import msssim
    a, b = ref.sample_pairs('smooth', 5, res, seed=res)
    _, _, levels = msssim.pairs(_dev(a), _dev(b), return_levels=True)
    assert len(levels) == 4
    for src, k in ((a, 0), (b, 1)):
        w32, w64 = ref.pyramid(src)[1:], ref.pyramid(src.astype(np.float64))[1:]
        for i, (lv, x32, x64) in enumerate(zip(levels, w32, w64)):
            got = lv[k].cpu().numpy()
            assert got.shape == x32.shape == (5, 3, res >> (i + 1), res >> (i + 1))
            err = float(np.abs(got - x64).max())
            print(f'{res} image {"ab"[k]} level {i + 1}: max err vs float64 {err:.2e}, bit-equal to fp32 {np.array_equal(got, x32)}')
            assert err <= 1e-6 * float(np.abs(src).max())
            assert np.array_equal(got, x32)


def _evaluate(ms, x, batch):
    ms.reset()
    for i in range(0, len(x), batch):
        ms.feed(x[i:i + batch])
    return ms.result()


@pytest.mark.parametrize('res', [32, 64, 256])
def test_end_to_end_matches_the_float64_reference(res):
    from gan_lab_amd import msssim
    a, b = ref.sample_pairs('near', 8, res, seed=res + 1)
    x = np.empty((16, 3, res, res), dtype=np.float32)
    x[0::2], x[1::2] = a, b
    raw = ref.raw_table(a, b)
    assert raw[:, :, 0].min() >= 0.05                   # on the reference alone: no pair sits at (or near) the clamp
    want, yard = ref.of_set(x), ref.of_set(x, dtype=np.float32)
    ms = msssim.MultiScaleSSIM(res, 16)
    got = _evaluate(ms, _dev(x), 4)
    per_pair = ms.per_pair()[0].cpu().numpy()
    w_pairs, y_pairs = ref.per_pair(a, b), ref.per_pair(a, b, dtype=np.float32)
    print(f'{res}: mean hip {got["msssim"]:.12g} reference {want["msssim"]:.12g} err {abs(got["msssim"] - want["msssim"]):.2e} '
          f'(fp32 numpy {abs(yard["msssim"] - want["msssim"]):.2e}); per pair max err {np.abs(per_pair - w_pairs).max():.2e} '
          f'(fp32 numpy {np.abs(y_pairs - w_pairs).max():.2e})')
    assert got['pairs'] == 8
    assert np.abs(per_pair - w_pairs).max() <= _bar(y_pairs, w_pairs)
    assert abs(got['msssim'] - want['msssim']) <= _bar(yard['msssim'], want['msssim'])
    flat = lambda r: np.array(r['per_level'][0] + [r['per_level'][1]])       # noqa: E731
    assert np.abs(flat(got) - flat(want)).max() <= _bar(flat(yard), flat(want))
    # the same pairs through pairs(): separate a / b batches instead of an interleaved set, bitwise the same
    assert torch.equal(msssim.pairs(_dev(a), _dev(b))[0], ms.per_pair()[0])


def test_anticorrelated_pairs_are_clamped_to_exactly_zero():
    from gan_lab_amd import msssim
    rng = np.random.default_rng(11)
    a = rng.standard_normal((6, 3, 64, 64)).astype(np.float32)
    b = -a
    assert (ref.raw_table(a, b)[:, 0, 0] < -0.1).all()
    values, table = msssim.pairs(_dev(a), _dev(b))
    assert values.cpu().tolist() == [0.0] * 6 and table[:, 0, 0].cpu().tolist() == [0.0] * 6
    x = np.empty((12, 3, 64, 64), dtype=np.float32)
    x[0::2], x[1::2] = a, b
    out = _evaluate(msssim.MultiScaleSSIM(64, 12), _dev(x), 12)
    assert out['msssim'] == 0.0 and out['per_level'][0][0] == 0.0


def test_identical_images_and_data_range():
    from gan_lab_amd import msssim
    a, b = ref.sample_pairs('smooth', 3, 32, seed=2)
    values, table = msssim.pairs(_dev(a), _dev(a))
    assert values.cpu().tolist() == [1.0] * 3 and bool((table == 1.0).all())
    for data_range in (1.0, 7.5):
        got = msssim.pairs(_dev(a), _dev(b), data_range=data_range)[1].cpu().numpy()
        want = ref.table(a, b, data_range)
        assert np.abs(got - want).max() <= _bar(ref.table(a, b, data_range, dtype=np.float32), want)
    assert np.abs(ref.table(a, b, 1.0) - ref.table(a, b, 7.5)).max() > 1e-2        # the option does reach the kernel


def test_results_are_bitwise_reproducible_and_independent_of_the_feeds(monkeypatch):
    from gan_lab_amd import msssim
    a, b = ref.sample_pairs('smooth', 16, 64, seed=9)
    x = np.empty((32, 3, 64, 64), dtype=np.float32)
    x[0::2], x[1::2] = a, b
    x = _dev(x)
    ms = msssim.MultiScaleSSIM(64, 32)
    whole = _evaluate(ms, x, 32)
    values = ms.per_pair()[0].clone()
    assert _evaluate(ms, x, 32) == whole and torch.equal(ms.per_pair()[0], values)          # twice in the same buffers
    assert _evaluate(msssim.MultiScaleSSIM(64, 32), x, 32) == whole                          # ... and in fresh ones
    for batch in (2, 8):
        assert _evaluate(ms, x, batch) == whole and torch.equal(ms.per_pair()[0], values)
    assert 0.0 < whole['msssim'] < 1.0 and whole['pairs'] == 16
    # a feed larger than the scratch buffers is walked in chunks: 3 pairs per chunk here, 16 = 5 x 3 + 1
    monkeypatch.setattr(msssim, '_SCRATCH_BYTES', 3 * sum(2 * 3 * (64 >> i) ** 2 * 4 for i in range(1, 5)))
    small = msssim.MultiScaleSSIM(64, 32)
    assert small._chunk == 3 and _evaluate(small, x, 32) == whole and torch.equal(small.per_pair()[0], values)
    # a non-contiguous feed (every second image of a larger batch) is copied, not misread
    y = torch.cat([x, x], dim=1)[:, :3]
    assert not y.is_contiguous() and _evaluate(ms, y, 8) == whole


def test_argument_checks_on_the_device():
    from gan_lab_amd import msssim, ops
    x = torch.zeros(4, 3, 32, 32, device='cuda')
    ws = ops.msssim_workspace(2, 32, 'cuda')
    with pytest.raises(ValueError):
        ops.msssim_level(x[0::2], x[1::2], 0, 64, 4e-4, 3.6e-3, ws, 0, 2)           # images are not 64 x 64
    with pytest.raises(ValueError):
        ops.msssim_level(x[0::2], x[1:2], 0, 32, 4e-4, 3.6e-3, ws, 0, 2)            # 2 images against 1
    with pytest.raises(ValueError):
        ops.msssim_level(x[0::2].transpose(2, 3), x[1::2], 0, 32, 4e-4, 3.6e-3, ws, 0, 2)
    from gan_lab_amd._lib import GanlabLibraryError
    with pytest.raises(GanlabLibraryError, match='EINVAL'):
        ops.msssim_level(x[0::2], x[1::2], 0, 32, 4e-4, 3.6e-3, ws, 1, 2)           # pairs 1, 2 of an evaluation of 2
    with pytest.raises(GanlabLibraryError, match='EWORKSPACE'):
        ops.msssim_level(x[0::2], x[1::2], 0, 32, 4e-4, 3.6e-3, ws[:4], 0, 2)
    with pytest.raises(ValueError, match='power of two'):
        msssim.pairs(torch.zeros(2, 3, 8, 8, device='cuda'), torch.zeros(2, 3, 8, 8, device='cuda'))


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


def _run_learner(gen_metrics, iters=3, init_res=16, res=16):
    """A small StyleGAN; validation at iterations 0 and 1 of 3 (num_iters_valid = 2)."""
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    torch.manual_seed(7)              # weight initialisation and style mixing draw from the host generators
    np.random.seed(7)
    L = make_learner('stylegan', res, init_res=init_res, batch=4, loss='nonsaturating', gradient_penalty='r1', num_iters_valid=2,
                     gen_metrics=gen_metrics, disc_metrics=[], random_seed=4, swd_nhoods=16, swd_dir_repeats=2,
                     swd_dirs_per_repeat=32)
    gen = torch.Generator().manual_seed(9)
    z_dl = _ZLoader([(torch.randn(4, 16, generator=gen),) for _ in range(3)])
    x_dl = SyntheticImageLoader(8, 4, init_res, seed=1)       # 8 reals, 12 latents: 'msssim real' scores two whole batches
    seen = []
    orig = L.compute_metrics

    def spy(*a, **kw):
        lines = orig(*a, **kw)
        seen.append((int(L.gen_model.curr_res), dict(L.last_metrics['generator']), lines))
        return lines
    L.compute_metrics = spy
    L.train(SyntheticImageLoader(4096, 4, init_res), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=iters)
    return L, seen


def _state(L):
    out = [L.arena_g.flat, L.arena_d.flat, L.ewma.flat]
    for opt, model in ((L.opt_gen, L.gen_model), (L.opt_disc, L.disc_model)):
        mom = opt.export_moments(list(model.named_parameters()))
        assert mom['step'] > 0 and mom['exp_avg']
        out += [torch.tensor(float(mom['step']))] + [mom[k][n] for k in ('exp_avg', 'exp_avg_sq') for n in sorted(mom[k])]
    return out


def test_learner_reports_msssim_and_leaves_training_and_swd_untouched(_widths, capsys):
    L, seen = _run_learner(['generator loss', 'msssim'])
    out = capsys.readouterr().out
    assert [res for res, _, _ in seen] == [16, 16]
    for res, m, lines in seen:
        assert [ln.split(':')[0].strip() for ln in lines] == ['generator loss', 'msssim fake', 'msssim real']
        d = m['msssim']
        assert d['pairs'] == 6 and d['real']['pairs'] == 4 and len(d['per_level'][0]) == 4
        for v in (d['msssim'], d['real']['msssim'], d['per_level'][1], *d['per_level'][0]):
            assert math.isfinite(v) and 0.0 <= v <= 1.0
        assert abs(float(lines[1].split(':')[1]) - d['msssim']) <= 1e-3 * max(d['msssim'], 1e-3)
        assert abs(float(lines[2].split(':')[1]) - d['real']['msssim']) <= 1e-3 * max(d['real']['msssim'], 1e-3)
    assert out.count('msssim fake:') == 2 and out.count('msssim real:') == 2
    assert L.last_metrics['generator']['msssim']['pairs'] == 6 and L.gen_model.training and L.disc_model.training
    # the same run without the metric: the same weights and Adam state, bit for bit (nothing random is drawn, and the
    # time-averaged generator's extra forward gives the process stream back)
    L2, seen2 = _run_learner(['generator loss'])
    assert 'msssim' not in seen2[-1][1] and seen2[-1][1]['generator loss'] == seen[-1][1]['generator loss']
    s1, s2 = _state(L), _state(L2)
    assert len(s1) == len(s2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
    # with 'swd' also on: SWD's numbers are what they are without 'msssim', MS-SSIM's what they are without 'swd' (the two
    # share one forward of the time-averaged generator), and training is still untouched
    L3, seen3 = _run_learner(['generator loss', 'swd', 'msssim'])
    L4, seen4 = _run_learner(['generator loss', 'swd'])
    for (_, m3, lines3), (_, m4, _), (_, m1, _) in zip(seen3, seen4, seen):
        assert m3['swd'] == m4['swd'] and math.isfinite(m3['swd']['mean'])
        assert m3['msssim'] == m1['msssim']
        assert [ln.split(':')[0].strip() for ln in lines3] == ['generator loss', 'swd 16x16', 'swd mean', 'msssim fake',
                                                               'msssim real']
    assert all(torch.equal(a, b) for a, b in zip(_state(L3), s2))


def test_below_sixteen_the_line_is_nan_and_nothing_raises(_widths):
    L, seen = _run_learner(['generator loss', 'msssim'], iters=1, init_res=8, res=32)
    (res, m, lines), = seen
    assert res == 8 and math.isnan(m['msssim']['msssim']) and m['msssim']['pairs'] == 0
    assert len(lines) == 2 and 'nan' in lines[1] and '16x16' in lines[1] and '8x8' in lines[1]


def test_compute_metrics_checks_on_the_device(_widths):
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    L = make_learner('progan', 16, init_res=16, batch=4, gen_metrics=['msssim'], use_ewma_gen=False)
    z_dl = _ZLoader([(torch.randn(4, 16),) for _ in range(2)])
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['msssim'], 'Discriminator', z_dl, SyntheticImageLoader(8, 4, 16))
    lines = L.compute_metrics(['msssim'], 'Generator', z_dl)                                   # no reals: one line
    assert [ln.split(':')[0].strip() for ln in lines] == ['msssim fake']
    assert L.last_metrics['generator']['msssim']['pairs'] == 4 and 'real' not in L.last_metrics['generator']['msssim']
    lines = L.compute_metrics(['msssim'], 'Generator', z_dl, SyntheticImageLoader(8, 4, 16))
    assert [ln.split(':')[0].strip() for ln in lines] == ['msssim fake', 'msssim real']
    with pytest.raises(ValueError, match='whole batch'):
        L.compute_metrics(['msssim'], 'Generator', _ZLoader([(torch.randn(2, 16),)]))
    L3 = make_learner('progan', 16, init_res=16, batch=3, gen_metrics=['msssim'], use_ewma_gen=False, mbstd_group_size=-1)
    with pytest.raises(ValueError, match='batch_size'):
        L3.compute_metrics(['msssim'], 'Generator', _ZLoader([(torch.randn(3, 16),)]))
