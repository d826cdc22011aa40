"""k-NN precision / recall / density / coverage on the GPU (csrc/prdc.hip, gan_lab_amd/prdc.py) against the
float64 brute-force restatement of its definition (tests/prdc_reference.py).

Rows with small integer entries make every partial sum an integer below 2^24: fp32 is exact in any order, so k-lists, counts,
minima, argmin indices and scores must EQUAL the reference, ties, duplicates, the <= rule and the exclusion of the row itself by
index included.  On real-valued rows the squared distances carry rounding error: radii and minima are held to twice the error of
ATen's CPU fp32 evaluation of the same formula (mm plus norms), in units of 2^-24 (|q|^2 + |k|^2), and a count may differ from the
reference only by pairs whose float64 distance is within that bar of the radius (there are none on these inputs).

Tile sizes the shapes are chosen around: 64 queries per workgroup, 64 keys per tile, depth chunks of 32, accumulation chains of
64 terms."""
import functools

import numpy as np
import pytest
import torch

import prdc_reference as ref

pytestmark = pytest.mark.gpu

TILE = 64


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device='cuda', dtype=dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _passes(real, fake, k):
    """Everything the kernels give for two sets, as numpy arrays named like the reference's parts."""
    from gan_lab_amd import ops
    r, f = _dev(real), _dev(fake)
    lists_r, lists_f = ops.prdc_knn(r, k), ops.prdc_knn(f, k)
    rad_r, rad_f = lists_r[:, k - 1].contiguous(), lists_f[:, k - 1].contiguous()
    c_fr, min_fr, arg_fr = ops.prdc_cross(f, r, rad_r, 'key')
    c_rf, min_rf, arg_rf = ops.prdc_cross(r, f, rad_f, 'key')
    c_cov, min_cov, arg_cov = ops.prdc_cross(r, f, rad_r, 'query')
    out = dict(lists_r=lists_r, lists_f=lists_f, c_fr=c_fr, min_fr=min_fr, arg_fr=arg_fr, c_rf=c_rf, min_rf=min_rf, arg_rf=arg_rf,
               c_cov=c_cov, min_cov=min_cov, arg_cov=arg_cov)
    return {name: _np(t) for name, t in out.items()}


def _scores(real, fake, k, batch=None):
    from gan_lab_amd import prdc
    ev = prdc.PRDC(real.shape[1], real.shape[0], fake.shape[0], k=k)
    r, f = _dev(real), _dev(fake)
    for which, rows in (('real', r), ('fake', f)):
        step = batch or len(rows)
        for i in range(0, len(rows), step):
            (ev.feed_real if which == 'real' else ev.feed_fake)(rows[i:i + step])
    return ev


def _assert_exact(got, want, k, tag):
    for name in ('lists_r', 'lists_f'):
        assert np.array_equal(got[name].astype(np.float64), want[name][:, :k]), (tag, name)
    for name in ('c_fr', 'c_rf', 'c_cov', 'arg_fr', 'arg_rf'):
        assert np.array_equal(got[name].astype(np.int64), want[name].astype(np.int64)), (tag, name)
    assert np.array_equal(got['arg_cov'], got['arg_rf']) and np.array_equal(got['min_cov'], got['min_rf']), tag
    for name in ('min_fr', 'min_rf'):
        assert np.array_equal(got[name].astype(np.float64), want[name]), (tag, name)


# ---- 1. exact on integer rows ------------------------------------------------------------------------------------------------
INT_KINDS = {'ternary D=6': (6, -1, 1), 'wide D=192': (192, -4, 4)}


@functools.lru_cache(maxsize=None)
def _int_case(kind, n, m):
    d, lo, hi = INT_KINDS[kind]
    real, fake = ref.integer_rows(n, d, lo, hi, seed=n), ref.integer_rows(m, d, lo, hi, seed=1000 + m)
    return real, fake, {k: ref.prdc(real, fake, k, parts=True) for k in (1, 3, 5, 16)}


@pytest.mark.parametrize('k', [1, 3, 5, 16])
@pytest.mark.parametrize('n,m', [(200, 136), (384, 320)])
@pytest.mark.parametrize('kind', sorted(INT_KINDS))
def test_integer_rows_equal_the_reference(kind, n, m, k):
    real, fake, by_k = _int_case(kind, n, m)
    want_scores, want = by_k[k]
    if kind.startswith('ternary'):
        # the input is what it is meant to be: duplicate rows within and across the sets, radii shared by many pairs
        assert len(np.unique(real, axis=0)) < n and (want['d_fr'] == 0).any() and (want['d_fr'] == want['rad_r'][None, :]).sum() > n
    _assert_exact(_passes(real, fake, k), want, k, (kind, n, m, k))
    ev = _scores(real, fake, k)
    assert ev.result() == want_scores
    idx, dist = ev.nearest_real()
    assert idx.dtype == torch.int64 and np.array_equal(_np(idx), want['arg_fr']) and np.array_equal(_np(dist).astype(np.float64), want['min_fr'])


# ---- 2. real-valued rows -------------------------------------------------------------------------------------------------
def _aten_sq(a, b):
    """ATen's CPU fp32 evaluation of |a|^2 + |b|^2 - 2 a.b, clamped at 0."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).clamp_min(0).double().numpy()


def _kth(d, k, exclude_self):
    """(values, indices) of the k-th smallest entry per row of a distance matrix."""
    d = d.copy()
    if exclude_self:
        d[np.arange(len(d)), np.arange(len(d))] = np.inf
    idx = np.argsort(d, axis=1, kind='stable')[:, k - 1]
    return d[np.arange(len(d)), idx], idx


@pytest.mark.parametrize('n,m,d,k', [(384, 320, 192, 5), (200, 136, 3072, 3), (130, 70, 50, 5)])
def test_real_valued_rows(n, m, d, k):
    real, fake = ref.manifold_rows(n, m, d, seed=d)
    want_scores, want = ref.prdc(real, fake, k, parts=True)
    got = _passes(real, fake, k)
    n2r, n2f = (real.astype(np.float64) ** 2).sum(1), (fake.astype(np.float64) ** 2).sum(1)
    eps = 2.0 ** -24
    unit = dict(rr=eps * (n2r[:, None] + n2r[None, :]), ff=eps * (n2f[:, None] + n2f[None, :]),
                fr=eps * (n2f[:, None] + n2r[None, :]))
    unit['rf'] = np.ascontiguousarray(unit['fr'].T)

    # radii and minima: error against float64 in units of 2^-24 (|q|^2 + |k|^2) of the pair the reference's value comes from
    err = {'kernel': {}, 'aten': {}}
    aten = dict(rr=_aten_sq(real, real), ff=_aten_sq(fake, fake), fr=_aten_sq(fake, real))
    aten['rf'] = _aten_sq(real, fake)
    unit_rad = {}
    for s, lists in (('rr', 'lists_r'), ('ff', 'lists_f')):
        val, idx = _kth(want['d_' + s], k, True)
        unit_rad[s] = unit[s][np.arange(len(idx)), idx]
        err['kernel']['radii ' + s] = float((np.abs(got[lists][:, k - 1] - val) / unit_rad[s]).max())
        err['aten']['radii ' + s] = float((np.abs(_kth(aten[s], k, True)[0] - val) / unit_rad[s]).max())
    for s in ('fr', 'rf'):
        val, idx = _kth(want['d_' + s], 1, False)
        u = unit[s][np.arange(len(idx)), idx]
        err['kernel']['minima ' + s] = float((np.abs(got['min_' + s] - val) / u).max())
        err['aten']['minima ' + s] = float((np.abs(aten[s].min(axis=1) - val) / u).max())
    for name in err['kernel']:
        print(f'({n}, {m}, {d}, k={k}) {name}: kernel {err["kernel"][name]:.2f} units, ATen CPU fp32 {err["aten"][name]:.2f} units')
    for group in ('radii', 'minima'):
        mine = max(v for name, v in err['kernel'].items() if name.startswith(group))
        theirs = max(v for name, v in err['aten'].items() if name.startswith(group))
        assert mine <= 2 * theirs, (group, mine, theirs)

    # a test of the inputs: no score is degenerate - the fakes are mostly inside the reals' manifold (precision 0.96 - 1.0,
    # density 1.04 - 1.13) and cover a part of it (recall 0.49 - 0.70, coverage 0.31 - 0.49)
    assert all(want_scores[name] > 0.2 for name in SCORES), want_scores
    assert want_scores['recall'] < 0.8 and want_scores['coverage'] < 0.8 and want_scores['density'] < 2.0, want_scores

    # counts: a pair is undecided if its float64 distance is within the bar - twice ATen's error, applied to the distance and to
    # the radius - of the radius; the kernel's count lies between the decided-inside pairs and those plus the undecided ones
    bar = 2 * max(err['aten'].values())
    undecided_total = pairs_total = 0
    for cnt, s, radius_of, rad, u_rad in (('c_fr', 'fr', 'key', want['rad_r'], unit_rad['rr']),
                                          ('c_rf', 'rf', 'key', want['rad_f'], unit_rad['ff']),
                                          ('c_cov', 'rf', 'query', want['rad_r'], unit_rad['rr'])):
        dist = want['d_' + s]
        rad2, u2 = (rad[None, :], u_rad[None, :]) if radius_of == 'key' else (rad[:, None], u_rad[:, None])
        undecided = np.abs(dist - rad2) <= bar * (unit[s] + u2)
        inside = (dist <= rad2) & ~undecided
        lo, hi = inside.sum(axis=1), inside.sum(axis=1) + undecided.sum(axis=1)
        assert ((got[cnt] >= lo) & (got[cnt] <= hi)).all(), (cnt, int(((got[cnt] < lo) | (got[cnt] > hi)).sum()))
        undecided_total += int(undecided.sum())
        pairs_total += dist.size
    print(f'({n}, {m}, {d}, k={k}) undecided pairs at a bar of {bar:.1f} units: {undecided_total} of {pairs_total}')
    assert undecided_total < 1e-3 * pairs_total
    if undecided_total == 0:
        assert _scores(real, fake, k).result() == want_scores


# ---- 3. tails and tiling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 7, 50])
@pytest.mark.parametrize('n,m', [(TILE - 1, 2 * TILE + 1), (TILE + 1, 2 * TILE - 1), (2 * TILE - 1, TILE + 1), (2 * TILE + 1, TILE - 1)])
def test_tails_in_rows_and_depth(n, m, d):
    """Each set is one more / one less than a multiple of the tile, as the queries of one pass and the keys of another; depths
    below, across and off the 32-wide chunk.  Integer rows: equality."""
    k = 5
    real, fake = ref.integer_rows(n, d, -3, 3, seed=n + d), ref.integer_rows(m, d, -3, 3, seed=m + 7 * d)
    want_scores, want = ref.prdc(real, fake, k, parts=True)
    _assert_exact(_passes(real, fake, k), want, k, (n, m, d))
    assert _scores(real, fake, k).result() == want_scores


def test_depth_across_an_accumulation_chain():
    """Depths one off the 64-term chain and one off two chains, keys past 2 tiles: integer rows, equality."""
    for d in (63, 65, 129):
        real, fake = ref.integer_rows(150, d, -4, 4, seed=d), ref.integer_rows(70, d, -4, 4, seed=d + 1)
        _, want = ref.prdc(real, fake, 3, parts=True)
        _assert_exact(_passes(real, fake, 3), want, 3, d)


def test_wrapper_argument_checks():
    from gan_lab_amd import ops
    x = torch.zeros(10, 4, device='cuda')
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match='k must be an integer'):
            ops.prdc_knn(x, bad)
    with pytest.raises(ValueError, match='below the number of rows'):
        ops.prdc_knn(x, 10)
    with pytest.raises(TypeError, match='float32'):
        ops.prdc_knn(x.double(), 3)
    with pytest.raises(ValueError, match='one width'):
        ops.prdc_cross(x, torch.zeros(6, 5, device='cuda'), torch.zeros(6, device='cuda'))
    with pytest.raises(ValueError, match='one per key'):
        ops.prdc_cross(x, torch.zeros(6, 4, device='cuda'), torch.zeros(10, device='cuda'), 'key')
    with pytest.raises(ValueError, match='one per query'):
        ops.prdc_cross(x, torch.zeros(6, 4, device='cuda'), torch.zeros(6, device='cuda'), 'query')
    with pytest.raises(ValueError, match='radius_of'):
        ops.prdc_cross(x, x, torch.zeros(10, device='cuda'), 'both')
    assert tuple(ops.prdc_knn(x[:, :3], 2).shape) == (10, 2)           # a strided view is made contiguous, as everywhere in ops


# ---- 4. the evaluation object ----------------------------------------------------------------------------------------------
def _state(ev):
    return [ev.radii('real'), ev.radii('fake')] + [t.clone() for p in sorted(ev._pass) for t in ev._pass[p]]


def test_evaluator_does_not_depend_on_how_it_was_fed_and_reuses_its_buffers():
    real, fake = ref.manifold_rows(200, 136, 50, seed=3)
    runs = [_scores(real, fake, 5, batch=b) for b in (8, 64, None, None)]
    base, base_state = runs[0].result(), _state(runs[0])
    for ev in runs[1:]:
        assert ev.result() == base
        assert all(torch.equal(a, b) for a, b in zip(_state(ev), base_state))
    assert 0 < base['recall'] < 1 and 0 < base['coverage'] < 1
    # reset(): another evaluation, the same buffers
    ev = runs[0]
    ptrs = [t.data_ptr() for t in ev._rows.values()] + [t.data_ptr() for p in ev._pass.values() for t in p]
    ev.reset()
    with pytest.raises(ValueError, match='were fed'):
        ev.result()
    ev.feed_real(_dev(real[::-1].copy()))
    ev.feed_fake(_dev(fake))
    again = ev.result()
    assert ptrs == [t.data_ptr() for t in ev._rows.values()] + [t.data_ptr() for p in ev._pass.values() for t in p]
    assert again == base                                                  # the scores do not depend on the order of the reals
    assert torch.equal(ev.nearest_real()[0], (len(real) - 1) - runs[1].nearest_real()[0])
    with pytest.raises(ValueError, match='declared with 136'):
        ev.feed_fake(_dev(fake[:1]))


def test_the_five_passes_replay_from_a_graph():
    """No host readback, no upload, no allocation inside: the passes captured with torch.cuda.graph replay to the eager bits."""
    real, fake = ref.manifold_rows(130, 70, 50, seed=5)
    ev = _scores(real, fake, 5)
    eager, eager_scores = _state(ev), ev.result()
    ev2 = _scores(real, fake, 5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev2._compute()
    for p in ev2._pass.values():                # a capture records, it does not run
        for t in p:
            t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, _state(ev2))) and ev2.result() == eager_scores


def test_no_distance_matrix_is_allocated():
    """N = M = 4096, D = 192: the distance matrix would be 64 MiB; the passes allocate under 8 MiB beyond the evaluation's buffers."""
    from gan_lab_amd import prdc
    n, d = 4096, 192
    gen = torch.Generator(device='cuda').manual_seed(0)
    real, fake = torch.randn(n, d, device='cuda', generator=gen), torch.randn(n, d, device='cuda', generator=gen) * 0.9 + 0.1
    ev = prdc.PRDC(d, n, n, k=5)
    ev.feed_real(real)
    ev.feed_fake(fake)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ev.result()
    idx, dist = ev.nearest_real()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'peak allocation above the buffers: {peak / 2 ** 20:.3f} MiB')
    assert peak < 8 * 2 ** 20
    assert all(0.0 <= out[name] <= 1.0 for name in ('precision', 'recall', 'coverage')) and out['density'] >= 0.0
    assert int(idx.min()) >= 0 and int(idx.max()) < n and bool((dist >= 0).all())


def test_features_are_repeated_2x2_means():
    from gan_lab_amd import prdc
    x = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    got = prdc.features(x.cuda(), 4)
    want = torch.nn.functional.avg_pool2d(torch.nn.functional.avg_pool2d(x.double(), 2), 2).reshape(3, -1)
    assert tuple(got.shape) == (3, 48) == (3, prdc.feature_dim(3, 16, 4))
    assert float((got.double().cpu() - want).abs().max()) <= 4 * 2.0 ** -24 * float(x.abs().max())
    assert torch.equal(prdc.features(x.cuda(), 32), x.cuda().reshape(3, -1))      # already small enough: the image itself
    with pytest.raises(ValueError, match='power of two'):
        prdc.features(x.cuda(), 12)


# ---- 5. learners ---------------------------------------------------------------------------------------------------------
class _ListLoader(object):
    """A loader over fixed batches (tuples): every pass yields the same tensors."""

    def __init__(self, batches):
        self.batches, self.dataset = batches, list(range(sum(len(b[0]) for b in batches)))
        self.batch_sampler = type('S', (), {'batch_size': len(batches[0][0])})()

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _fixed_loaders(batch, res, len_latent, n_z_batches=3, n_x_batches=2, seed=9):
    gen = torch.Generator().manual_seed(seed)
    z_dl = _ListLoader([(torch.randn(batch, len_latent, generator=gen),) for _ in range(n_z_batches)])
    x_dl = _ListLoader([(torch.rand(batch, 3, res, res, generator=gen) * 2 - 1, torch.zeros(batch, dtype=torch.int64))
                        for _ in range(n_x_batches)])
    return z_dl, x_dl


def _spy_features(monkeypatch):
    from gan_lab_amd import prdc
    seen, orig = [], prdc.features

    def spy(x, res):
        rows = orig(x, res)
        seen.append(rows.clone())
        return rows
    monkeypatch.setattr(prdc, 'features', spy)
    return seen


SCORES = ('precision', 'recall', 'density', 'coverage')


def test_progan_learner_scores_the_images_it_validates_on(monkeypatch, capsys):
    from gan_lab_amd import prdc, progressive as P
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    torch.manual_seed(7)
    np.random.seed(7)
    L = make_learner('progan', 8, init_res=8, batch=4, gen_metrics=['generator loss', 'prdc'], disc_metrics=[], prdc_k=3,
                     random_seed=4)
    z_dl, x_dl = _fixed_loaders(4, 8, 16)                    # 12 latents, 8 reals: two whole batches per set
    seen = _spy_features(monkeypatch)
    L.train(SyntheticImageLoader(64, 4, 8), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=2)
    out = capsys.readouterr().out
    got = L.last_metrics['generator']['prdc']
    assert set(SCORES) <= set(got) and (got['k'], got['n_real'], got['n_fake']) == (3, 8, 8)
    assert all(f'{name}:' in out for name in SCORES) and 'generator loss:' in out
    assert np.isfinite(L.last_metrics['generator']['generator loss'])
    # the rows it fed (fake, real, fake, real) through an evaluation of our own
    assert len(seen) == 4 and all(tuple(s.shape) == (4, 3 * 8 * 8) for s in seen)
    ev = prdc.PRDC(3 * 8 * 8, 8, 8, k=3)
    for i, rows in enumerate(seen):
        (ev.feed_real if i % 2 else ev.feed_fake)(rows)
    assert ev.result() == got
    assert torch.equal(seen[1], x_dl.batches[0][0].cuda().reshape(4, -1))         # 8x8, no fade-in: the reals as they are
    assert L.gen_model.training and L.disc_model.training


def _resnet_learner(**kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=8,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=1, len_latent=32, random_seed=7, **kw)
    cfg.fmap_g, cfg.fmap_d = 16, 16
    torch.manual_seed(7)
    return GANLearner(cfg)


RESNET_VARIANTS = {'plain': {}, 'cgan+ewma': dict(cgan='projection', num_classes=3, use_ewma_gen=True, ewma_decay=0.9)}


@pytest.mark.parametrize('variant', sorted(RESNET_VARIANTS))
def test_resnet_learner_compute_metrics_and_train(variant, monkeypatch, capsys):
    from gan_lab_amd import prdc, rng
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    kw = RESNET_VARIANTS[variant]
    z_dl, x_dl = _fixed_loaders(8, 32, 32)                   # 24 latents, 16 reals: two whole batches per set
    L = _resnet_learner(gen_metrics=['prdc'], prdc_k=3, prdc_res=8, **kw)
    L.set_requires_grad_disc(False)
    L.g_step()                                               # the averaged generator (where there is one) has seen an update
    L.set_requires_grad_disc(True)

    # compute_metrics = an evaluation of our own over generate()'s images; the process stream is where it was
    offset = rng._STATE['offset']
    lines = L.compute_metrics(['prdc'], 'Generator', z_dl, x_dl)
    assert rng._STATE['offset'] == offset
    got = L.last_metrics['generator']['prdc']
    assert [ln.split(':')[0].strip() for ln in lines] == list(SCORES)
    assert (got['k'], got['n_real'], got['n_fake']) == (3, 16, 16)
    ev = prdc.PRDC(3 * 8 * 8, 16, 16, k=3)
    for (zb,), (xb, _) in zip(z_dl.batches[:2], x_dl.batches):
        ev.feed_fake(prdc.features(L.generate(zs=zb.cuda(), truncation=None, time_average=True), 8))
        ev.feed_real(prdc.features(xb.cuda(), 8))
    rng._STATE['offset'] = offset
    assert ev.result() == got
    assert L.gen_model.training

    # anything else is refused by name
    with pytest.raises(ValueError, match='fake realness'):
        L.compute_metrics(['prdc', 'fake realness'], 'Generator', z_dl, x_dl)
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['prdc'], 'Discriminator', z_dl, x_dl)
    with pytest.raises(ValueError, match='valid_dl'):
        L.compute_metrics(['prdc'], 'Generator', z_dl, None)

    # train() with both loaders evaluates at iteration 0 (and not again before num_iters_valid)
    calls = []
    orig = L.compute_metrics
    monkeypatch.setattr(L, 'compute_metrics', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    L.last_metrics.clear()
    capsys.readouterr()
    L.train(SyntheticImageLoader(64, 8, 32), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=2)
    assert len(calls) == 1 and set(SCORES) <= set(L.last_metrics['generator']['prdc'])
    printed = capsys.readouterr().out
    assert all(f'{name}:' in printed for name in SCORES)
    # ... and without one of the loaders it does what it did before
    L.last_metrics.clear()
    L.train(SyntheticImageLoader(64, 8, 32), valid_dl=x_dl, num_main_iters=1)
    assert len(calls) == 1 and L.last_metrics == {}


def test_resnet_learner_default_metrics_leave_train_alone(monkeypatch):
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    z_dl, x_dl = _fixed_loaders(8, 32, 32)
    L = _resnet_learner()
    assert 'prdc' not in L.config.gen_metrics
    monkeypatch.setattr(L, 'compute_metrics', lambda *a, **k: pytest.fail('compute_metrics must not run'))
    L.train(SyntheticImageLoader(64, 8, 32), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=2)
    assert L.last_metrics == {}
