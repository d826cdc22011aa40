"""The sliced Wasserstein metric on the GPU (csrc/swd.hip, gan_lab_amd/swd.py) against the float64 numpy
restatement of its definition (tests/swd_reference.py), always with the SAME patch centres and directions: the device's
draws are downloaded, or host-drawn ones uploaded.  Bounds: the pyramid is a 25-term convex combination in fp32 (1e-5 of
max |x|), the gather is a copy (bit-equal), the statistics are fp64 sums of fp32 values (1e-6 relative), a projection is a
148-term fp32 chain of unit-variance operands (1e-5 absolute), the sort is exact, and the whole chain stays within 1e-4
relative of float64 at ~2048 descriptors per set."""
import math

import numpy as np
import pytest
import torch

import swd_reference as ref

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device='cuda', dtype=dtype)


def _impulses(res):
    """One-hot planes: each corner and each edge midpoint (pins the mirror rule and both parities of ``up``), one per
    channel slot of a (k, 3, res, res) batch."""
    m, e = res // 2, res - 1
    spots = [(0, 0), (0, e), (e, 0), (e, e), (0, m), (e, m), (m, 0), (m, e), (0, m - 1), (e, m - 1), (m - 1, 0), (m - 1, e)]
    x = np.zeros((len(spots) // 3, 3, res, res), dtype=np.float32)
    for k, (i, j) in enumerate(spots):
        x[k // 3, k % 3, i, j] = 1.0
    return x


@pytest.mark.parametrize('res', [16, 32, 64, 256])
@pytest.mark.parametrize('kind', ['smooth+noise', 'impulses'])
def test_pyramid_matches_the_reference_at_every_level(res, kind):
    from gan_lab_amd import swd
    x = ref.sample_images(5, res, seed=res) if kind == 'smooth+noise' else _impulses(res)
    got = swd.laplacian_pyramid(_dev(x))
    want = ref.laplacian_pyramid(x.astype(np.float64))
    assert [tuple(g.shape) for g in got] == [w.shape for w in want] and got[-1].shape[-1] == 16
    bound = 1e-5 * float(np.abs(x).max())
    for g, w in zip(got, want):
        err = float(np.abs(g.double().cpu().numpy() - w).max())
        print(f'{kind} {res} level {w.shape[-1]}: max err {err:.3e} (bound {bound:.3e})')
        assert err <= bound, (kind, res, w.shape[-1], err)


@pytest.mark.parametrize('res', [16, 32])
def test_down_and_band_kernels_on_the_smallest_planes(res):
    """R = 16 has a one-level pyramid (no kernel runs), so the two stencils are also checked directly on small planes,
    with a leading shape that is not (N, 3)."""
    from gan_lab_amd import ops
    x = np.concatenate([ref.sample_images(2, res, seed=7).reshape(6, res, res), _impulses(res).reshape(-1, res, res)])
    g0 = _dev(x)
    g1 = ops.swd_down(g0)
    band = ops.swd_band(g0, g1)
    want1 = ref.down(x.astype(np.float64))
    bound = 1e-5 * float(np.abs(x).max())
    assert float(np.abs(g1.double().cpu().numpy() - want1).max()) <= bound
    want_band = x.astype(np.float64) - ref.up(g1.double().cpu().numpy())
    assert float(np.abs(band.double().cpu().numpy() - want_band).max()) <= bound
    for bad in (torch.zeros(2, 15, 16, device='cuda'), torch.zeros(2, 2, 2, device='cuda')):
        with pytest.raises(ValueError):
            ops.swd_down(bad)


def _positions_with_extremes(rng, n_img, n, s):
    pos = rng.integers(3, s - 3, size=(n_img, n, 2))
    pos[0, 0], pos[0, 1], pos[-1, -1], pos[-1, -2] = (3, 3), (s - 4, s - 4), (3, s - 4), (s - 4, 3)
    return pos.astype(np.int32)


@pytest.mark.parametrize('res', [16, 64])
def test_descriptors_are_a_bit_exact_gather_and_statistics_match_float64(res):
    from gan_lab_amd import swd
    rng = np.random.default_rng(res)
    x = ref.sample_images(5, res, seed=3) + np.float32(0.3)
    for level in swd.laplacian_pyramid(_dev(x)):
        s = level.shape[-1]
        pos = _positions_with_extremes(rng, 5, 37, s)
        desc, stats = swd.descriptors(level, _dev(pos, torch.int32), with_stats=True)
        want = ref.descriptors(level.cpu().numpy(), pos)
        assert desc.shape == (5 * 37, 147) and np.array_equal(desc.cpu().numpy(), want)
        mean, std = ref.channel_stats(want)
        got = stats.cpu().numpy()
        rel = np.abs(got - np.concatenate([mean, std])) / np.abs(np.concatenate([mean, std]))
        print(f'level {s}: statistics rel err {rel.max():.3e}')
        assert rel.max() <= 1e-6
    with pytest.raises(ValueError, match='centres'):
        swd.descriptors(level, torch.full((5, 2, 2), 2, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='centres'):
        swd.descriptors(level, torch.full((5, 2, 2), 13, dtype=torch.int32, device='cuda'))


def test_device_draws_are_in_range_uniform_and_unit_norm():
    from gan_lab_amd import rng as grng
    pos = grng.swd_positions(64, 128, 16, seed=5, offset=0).cpu().numpy()
    assert pos.shape == (64, 128, 2) and pos.min() == 3 and pos.max() == 12
    counts = np.bincount(pos.reshape(-1), minlength=13)[3:]
    assert counts.min() > 0.85 * pos.size / 10 and counts.max() < 1.15 * pos.size / 10
    # image i's centres do not depend on the call they were drawn in; an odd count per image works too
    again = grng.swd_positions(10, 128, 16, seed=5, offset=7 * 64).cpu().numpy()
    assert np.array_equal(again, pos[7:17])
    odd = grng.swd_positions(3, 5, 1024, seed=5, offset=0).cpu().numpy()
    assert odd.shape == (3, 5, 2) and odd.min() >= 3 and odd.max() <= 1020
    d = grng.swd_directions(512, seed=9, offset=0)
    dn = d.double().cpu().numpy()
    assert d.shape == (512, 147) and np.abs(np.sqrt((dn * dn).sum(1)) - 1).max() < 1e-6
    assert abs(dn.mean()) < 3e-3 and abs(dn.std() * math.sqrt(147) - 1) < 0.02
    assert torch.equal(grng.swd_directions(128, seed=9, offset=128 * 147), d[128:256])
    # explicit seed / offset: the process stream does not move; without them it does
    before = dict(grng._STATE)
    grng.swd_positions(2, 4, 16, seed=1, offset=3)
    grng.swd_directions(2, seed=1, offset=3)
    assert grng._STATE == before
    grng.swd_positions(2, 4, 16)
    grng.swd_directions(2)
    assert grng._STATE['offset'] == before['offset'] + 2 * 2 + 2 * 147


@pytest.mark.parametrize('m,d', [(1003, 512), (4096, 40)])
def test_projections_match_float64(m, d):
    """M = 1003: the scalar store tail and a partial last tile; D = 40: a partial direction tile."""
    from gan_lab_amd import ops
    rng = np.random.default_rng(m)
    desc = (rng.standard_normal((m, 147)) * np.repeat([2.0, 0.5, 1.0], 49) + np.repeat([0.3, -1.0, 0.0], 49)).astype(np.float32)
    dirs = ref.directions(rng, 1, d)[0].astype(np.float32)
    mean, std = ref.channel_stats(desc)
    stats = _dev(np.concatenate([mean, std]), torch.float64)
    got = ops.swd_project(_dev(desc), _dev(dirs), stats)
    want = dirs.astype(np.float64) @ ref.normalise(desc.astype(np.float64)).T
    assert got.shape == (d, m)
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    print(f'projection ({m}, {d}): max err {err:.3e}')
    assert err <= 1e-5


@pytest.mark.parametrize('segments,m', [(512, 1003), (6, 70001)])
def test_sort_rows_ascending_and_equal_to_torch_sort(segments, m):
    """Both paths of the entry point: the segmented sort (M below 65536) and the per-segment device-wide sort."""
    from gan_lab_amd import ops
    assert m % 64 != 0
    x = torch.randn(segments, m, device='cuda', generator=torch.Generator('cuda').manual_seed(m))
    keep = x.clone()
    got = ops.swd_sort(x)
    assert torch.equal(x, keep)
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    want = torch.sort(x, dim=1).values
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        ops.swd_sort(x, out=x)
    a, b = got, torch.sort(x + 0.25, dim=1).values
    dist = float(ops.swd_distance(a, b))
    assert abs(dist - float((a.double() - b.double()).abs().mean())) < 1e-12 and abs(dist - 0.25) < 1e-6


def _evaluate(sw, real, fake, batch):
    sw.reset()
    for i in range(0, len(real), batch):
        sw.feed_real(real[i:i + batch])
        sw.feed_fake(fake[i:i + batch])
    return sw.result()


def test_end_to_end_matches_the_float64_reference():
    """64 images at 64^2, 32 neighbourhoods each: 2048 descriptors per set, the device's own centres and directions."""
    from gan_lab_amd import swd
    real, fake = ref.sample_images(64, 64, seed=21), ref.sample_images(64, 64, seed=22, smooth=1)
    sw = swd.SlicedWasserstein(64, 64, nhoods_per_image=32, seed=3)
    got = _evaluate(sw, _dev(real), _dev(fake), 16)
    pos = [sw.positions(li).cpu().numpy() for li in range(3)]
    dirs = np.stack([sw.directions(r).double().cpu().numpy() for r in range(4)])
    want = ref.swd(real.astype(np.float64), fake.astype(np.float64), pos, dirs)
    assert got['levels'] == want['levels'] == [64, 32, 16]
    for lv, g, w in zip(got['levels'], got['swd'], want['swd']):
        print(f'level {lv}: hip {g:.9g} reference {w:.9g} rel err {abs(g - w) / w:.3e}')
    for g, w in zip(got['swd'] + [got['mean']], want['swd'] + [want['mean']]):
        assert abs(g - w) <= 1e-4 * w


@pytest.fixture(scope='module')
def big_sets():
    """2048 images at 128^2 (262144 descriptors per set and level at the default 128 neighbourhoods): two independent
    draws of one distribution and one draw of it smoothed by four more passes of f (x) f."""
    return tuple(_dev(ref.sample_images(2048, 128, seed=s, smooth=k)) for s, k in ((11, 0), (12, 0), (13, 4)))


def test_properties_at_size(big_sets):
    from gan_lab_amd import swd
    a, b, c = big_sets
    sw = swd.SlicedWasserstein(128, 2048, seed=1)
    assert sw.levels == [128, 64, 32, 16] and sw.m == 2048 * 128
    same = _evaluate(sw, a, a, 64)
    assert same['swd'] == [0.0] * 4 and same['mean'] == 0.0                 # a set against itself: exactly zero
    r64 = _evaluate(sw, a, c, 64)
    assert _evaluate(sw, a, c, 64) == r64                                   # same seed, same buffers: bitwise
    assert _evaluate(swd.SlicedWasserstein(128, 2048, seed=1), a, c, 64) == r64     # ... and in fresh ones
    assert _evaluate(sw, a, c, 7) == r64                                    # minibatches of 7 (2048 = 292 x 7 + 4) or of 64
    assert _evaluate(swd.SlicedWasserstein(128, 2048, seed=2), a, c, 64) != r64     # another seed: other centres / directions
    # discrimination.  The pair and the size were chosen with the float64 reference on the CPU (host-drawn centres and
    # directions, these very images): shifted / independent-draw = 90.7 / 3.73 (24x) at 128, 38.0 / 3.72 (10x) at 64,
    # 15.2 / 3.75 (4.0x) at 32; a single extra smoothing pass separates 32^2 by only 1.5x and was not used.  The 16^2
    # level sees the smoothing least (1.4x there) and is not part of the claim.
    floor = _evaluate(sw, a, b, 64)
    for lv, shifted, same_dist in zip(r64['levels'], r64['swd'], floor['swd']):
        print(f'level {lv}: shifted {shifted:.4g} vs independent draw {same_dist:.4g}')
    for lv, shifted, same_dist in zip(r64['levels'], r64['swd'], floor['swd']):
        if lv > 16:
            assert shifted > same_dist, lv
    assert all(math.isfinite(v) and v > 0 for v in floor['swd'])


def test_a_zero_variance_channel_is_nan_at_that_level_only():
    """Channel 2 is a +-1 checkerboard: f sums it to exactly zero, so the 16^2 level of that channel is constant 0 (zero
    variance: NaN, as the definition has it) while its 32^2 band is the checkerboard itself."""
    from gan_lab_amd import swd
    real, fake = ref.sample_images(32, 32, seed=5), ref.sample_images(32, 32, seed=6)
    board = (1.0 - 2.0 * ((np.arange(32)[:, None] + np.arange(32)[None, :]) % 2)).astype(np.float32)
    # per-image amplitudes k / 4: every partial sum of the filter is exact in fp32, so the cancellation is too
    real[:, 2] = board * ((2 + np.arange(32) % 5) / 4).astype(np.float32)[:, None, None]
    sw = swd.SlicedWasserstein(32, 32, nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=64)
    out = _evaluate(sw, _dev(real), _dev(fake), 32)
    assert out['levels'] == [32, 16]
    assert math.isfinite(out['swd'][0]) and out['swd'][0] > 0 and math.isnan(out['swd'][1]) and math.isnan(out['mean'])


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


def _run_learner(gen_metrics, iters=24):
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    torch.manual_seed(7)              # weight initialisation and style mixing draw from the host generators
    np.random.seed(7)
    L = make_learner('stylegan', 32, init_res=8, batch=4, loss='nonsaturating', gradient_penalty='r1', num_iters_valid=8,
                     gen_metrics=gen_metrics, disc_metrics=[], random_seed=4, swd_nhoods=16, swd_dir_repeats=2,
                     swd_dirs_per_repeat=32)
    gen = torch.Generator().manual_seed(9)
    z_dl = _ZLoader([(torch.randn(4, 16, generator=gen),) for _ in range(3)])
    x_dl = SyntheticImageLoader(8, 4, 8, seed=1)              # 8 reals, 12 latents: two whole batches are compared
    seen = []
    orig = L.compute_metrics

    def spy(*a, **kw):
        lines = orig(*a, **kw)
        seen.append((int(L.gen_model.curr_res), dict(L.last_metrics['generator']), lines))
        return lines
    L.compute_metrics = spy
    L.train(SyntheticImageLoader(4096, 4, 8), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=iters)
    return L, seen


def test_learner_reports_swd_per_level_and_leaves_training_untouched(_widths, capsys):
    """6 iterations per phase: validation at iterations 0 (8^2), 7 (16^2 fade-in), 15 (16^2), 23 (32^2 fade-in)."""
    L, seen = _run_learner(['generator loss', 'swd'])
    out = capsys.readouterr().out
    assert [res for res, _, _ in seen] == [8, 16, 16, 32]
    res, m, lines = seen[0]
    assert m['swd']['levels'] == [] and math.isnan(m['swd']['mean'])
    assert len(lines) == 2 and 'nan' in lines[1] and '16x16' in lines[1] and '8x8' in lines[1]
    for res, m, lines in seen[1:]:
        want = [32, 16] if res == 32 else [16]
        assert m['swd']['levels'] == want and len(m['swd']['swd']) == len(want)
        assert all(math.isfinite(v) and v > 0 for v in m['swd']['swd']) and math.isfinite(m['generator loss'])
        assert [ln.split(':')[0].strip() for ln in lines] == ['generator loss'] + [f'swd {r}x{r}' for r in want] + ['swd mean']
        assert abs(float(lines[-1].split(':')[1]) - m['swd']['mean']) <= 1e-3 * m['swd']['mean']
    assert out.count('swd mean:') == 3 and out.count('swd 32x32:') == 1 and out.count('swd 16x16:') == 3
    assert L.last_metrics['generator']['swd']['levels'] == [32, 16] and L.gen_model.training and L.disc_model.training
    # the same run without the metric: the same weights, bit for bit (the metric draws from its own sub-streams, and the
    # time-averaged generator's extra forward gives the process stream back)
    L2, seen2 = _run_learner(['generator loss'])
    assert 'swd' not in seen2[-1][1] and seen2[-1][1]['generator loss'] == seen[-1][1]['generator loss']
    for a, b in ((L.arena_g.flat, L2.arena_g.flat), (L.arena_d.flat, L2.arena_d.flat), (L.ewma.flat, L2.ewma.flat)):
        assert torch.equal(a, b)


def test_compute_metrics_checks_on_the_device(_widths):
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    L = make_learner('progan', 16, init_res=16, batch=4, gen_metrics=['swd'], swd_nhoods=8, swd_dir_repeats=1,
                     swd_dirs_per_repeat=16, use_ewma_gen=False)
    z_dl = _ZLoader([(torch.randn(4, 16),) for _ in range(2)])
    with pytest.raises(ValueError, match='valid_dl'):
        L.compute_metrics(['swd'], 'Generator', z_dl)
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['swd'], 'Discriminator', z_dl, SyntheticImageLoader(8, 4, 16))
    with pytest.raises(ValueError, match='whole batch'):
        L.compute_metrics(['swd'], 'Generator', z_dl, SyntheticImageLoader(3, 4, 16))
    lines = L.compute_metrics(['swd'], 'Generator', z_dl, SyntheticImageLoader(8, 4, 16))
    assert [ln.split(':')[0].strip() for ln in lines] == ['swd 16x16', 'swd mean']
    assert L.last_metrics['generator']['swd']['levels'] == [16]
