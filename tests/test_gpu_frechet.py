"""The Frechet distance's streamed moments on the GPU (csrc/frechet.hip, gan_lab_amd/frechet.py) against the
float64 restatement (tests/frechet_reference.py), and the learners' 'fd' / 'kid' metrics.

Rows with small integer entries about an integer pivot make every product and partial sum an integer below 2^24: fp32 is exact in
any order, so ``sum`` and ``gram`` must EQUAL the reference.  On rows ``100 + correlated noise`` the covariance is held to twice
the error of ATen's CPU fp32 evaluation of the same pivoted formula, and to a hundredth of the error of ATen's fp32
``E[xx^T] - mu mu^T``.

Sizes the shapes are chosen around: 64 x 64 tiles of the second-moment matrix, row chunks of 32, each one accumulation chain."""
import functools

import numpy as np
import pytest
import torch

import frechet_reference as ref

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device='cuda', dtype=dtype)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_case(d):
    rows, pivot = ref.integer_rows(200, d, -4, 4, seed=d), ref.integer_rows(1, d, -2, 2, seed=100 + d)[0]
    return rows, pivot


# ---- 1. exact on integer rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 37, 64, 200])
@pytest.mark.parametrize('d', [6, 48, 64, 200])
def test_integer_rows_equal_the_reference(d, n):
    """D = 200: four column tiles with a tail of 8, off-diagonal tiles and their mirrors.  A second launch adds to the first."""
    from gan_lab_amd import ops
    rows, pivot = _int_case(d)
    want_s, want_g = ref.pivoted_sums(rows[:n], pivot)
    assert np.abs(want_g).max() < 2 ** 24
    s, g = torch.zeros(d, dtype=torch.float64, device='cuda'), torch.zeros(d, d, dtype=torch.float64, device='cuda')
    ops.moments_accum(_dev(rows[:n]), _dev(pivot), s, g)
    assert np.array_equal(_np(s), want_s) and np.array_equal(_np(g), want_g), (d, n)
    assert torch.equal(g, g.T)
    ops.moments_accum(_dev(rows[:n]), _dev(pivot), s, g)
    assert np.array_equal(_np(s), 2 * want_s) and np.array_equal(_np(g), 2 * want_g), (d, n)


def _feed(rows, splits, pivot=None, which='real'):
    from gan_lab_amd import frechet
    ev = frechet.Frechet(rows.shape[1], pivot=None if pivot is None else _dev(pivot))
    x, lo = _dev(rows), 0
    for k in splits:
        (ev.feed_real if which == 'real' else ev.feed_fake)(x[lo:lo + k])
        lo += k
    assert lo == len(rows)
    return ev


def test_feeding_order_does_not_matter_on_integer_rows():
    rows, pivot = _int_case(200)
    one, four = _feed(rows, [200], pivot), _feed(rows, [1, 37, 64, 98], pivot)
    (n1, p1, s1, g1), (n4, p4, s4, g4) = one.raw('real'), four.raw('real')
    assert n1 == n4 == 200 and torch.equal(p1, p4) and torch.equal(s1, s4) and torch.equal(g1, g4)
    want_s, want_g = ref.pivoted_sums(rows, pivot)
    assert np.array_equal(_np(s4), want_s) and np.array_equal(_np(g4), want_g)
    mean, cov = four.moments('real')
    want_mean, want_cov = ref.moments(rows)
    assert mean.dtype == cov.dtype == torch.float64 and mean.is_cuda and cov.is_cuda
    assert np.abs(_np(mean) - want_mean).max() <= 2.0 ** -50 * 4 and np.abs(_np(cov) - want_cov).max() <= 2.0 ** -48 * 36


def test_the_same_feeds_give_the_same_bits():
    rows = ref.offset_rows(200, 200, seed=2)
    a, b = _feed(rows, [64, 37, 99]), _feed(rows, [64, 37, 99])
    assert all(torch.equal(x, y) for x, y in zip(a.raw('real')[1:], b.raw('real')[1:]))
    g = a.raw('real')[3]
    assert torch.equal(g, g.T)
    a.reset()                                                   # reset(): the same accumulators, from zero
    assert float(a.raw('real')[3].abs().max()) == 0.0 and a.raw('real')[0] == 0
    for k, lo in ((64, 0), (37, 64), (99, 101)):
        a.feed_real(_dev(rows[lo:lo + k]))
    assert all(torch.equal(x, y) for x, y in zip(a.raw('real')[1:], b.raw('real')[1:]))


# ---- 2. rows with a large common offset ----------------------------------------------------------------------------------------
def _aten_pivoted(rows):
    """ATen's CPU fp32 evaluation of the pivoted formula, the pivot being the fp32 mean: (mean, cov) as float64 arrays."""
    x = torch.as_tensor(rows)
    n = x.shape[0]
    c = x.mean(dim=0)
    y = x - c
    s, g = y.sum(dim=0), y.T @ y
    return (c + s / n).double().numpy(), ((g - torch.outer(s, s) / n) / (n - 1)).double().numpy()


def _aten_naive(rows):
    """ATen's CPU fp32 E[xx^T] - mu mu^T, scaled to the n - 1 denominator."""
    x = torch.as_tensor(rows)
    n = x.shape[0]
    mu = x.mean(dim=0)
    return (((x.T @ x) / n - torch.outer(mu, mu)) * (n / (n - 1))).double().numpy()


OFFSET_CASES = {'n=200 D=48': (200, 48), 'n=40 D=96': (40, 96)}


@pytest.mark.parametrize('case', sorted(OFFSET_CASES))
def test_covariance_of_rows_with_a_large_offset(case):
    n, d = OFFSET_CASES[case]
    rows = ref.offset_rows(n, d, seed=d)
    _, want = ref.moments(rows)
    mean, cov = _feed(rows, [n]).moments('real')
    err = float(np.abs(_np(cov) - want).max())
    err_aten = float(np.abs(_aten_pivoted(rows)[1] - want).max())
    err_naive = float(np.abs(_aten_naive(rows) - want).max())
    print(f'{case}: covariance of scale {np.abs(want).max():.1f}: kernel {err:.2e}, ATen CPU fp32 pivoted {err_aten:.2e}, '
          f'ATen CPU fp32 E[xx^T] - mu mu^T {err_naive:.2e} ({err_naive / err:.0f}x)')
    assert err <= 2 * err_aten
    assert 100 * err <= err_naive
    assert np.abs(_np(mean) - ref.moments(rows)[0]).max() <= 2.0 ** -24 * 100


@pytest.mark.parametrize('case', sorted(OFFSET_CASES))
def test_result_end_to_end(case):
    """The bar: twice the relative error of the same distance composed from ATen's CPU fp32 pivoted moments.  Measured on an
    MI355X: 4.87e-8 against ATen's 4.86e-8 at 200 x 48; 3.09e-5 against 3.98e-5 at 40 x 96, where the zero eigenvalues' rounding
    under the square root sets the error of any float64 solve (test_frechet_host.py)."""
    n, d = OFFSET_CASES[case]
    real = ref.offset_rows(n, d, seed=d)
    fake = ref.offset_rows(n + 10, d, seed=d + 1, offset=100.5, scale=1.2)
    want = ref.frechet(real, fake)
    ev = _feed(real, [n])
    x = _dev(fake)
    ev.feed_fake(x[:33])
    ev.feed_fake(x[33:])
    got = ev.result()
    assert set(got) == {'fd', 'mean_term', 'trace_term', 'n_real', 'n_fake'} and (got['n_real'], got['n_fake']) == (n, n + 10)
    aten = ref.distance(*_aten_pivoted(real), *_aten_pivoted(fake))
    rel, rel_aten = abs(got['fd'] - want['fd']) / want['fd'], abs(aten['fd'] - want['fd']) / want['fd']
    print(f'{case}: fd {got["fd"]:.9g} (float64 {want["fd"]:.9g}): relative error {rel:.2e}, from ATen CPU fp32 moments {rel_aten:.2e}')
    assert rel <= 2 * rel_aten
    assert got['fd'] == pytest.approx(got['mean_term'] + got['trace_term'], rel=1e-15)


def test_wrapper_argument_checks():
    from gan_lab_amd import frechet, ops
    x, c = torch.zeros(10, 4, device='cuda'), torch.zeros(4, device='cuda')
    s, g = torch.zeros(4, dtype=torch.float64, device='cuda'), torch.zeros(4, 4, dtype=torch.float64, device='cuda')
    with pytest.raises(TypeError, match='float32'):
        ops.moments_accum(x.double(), c, s, g)
    with pytest.raises(TypeError, match='float64'):
        ops.moments_accum(x, c, s.float(), g)
    with pytest.raises(ValueError, match='pivot'):
        ops.moments_accum(x, torch.zeros(5, device='cuda'), s, g)
    with pytest.raises(ValueError, match='gram'):
        ops.moments_accum(x, c, s, torch.zeros(4, 5, dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='gram'):
        ops.moments_accum(x, c, s, torch.zeros(8, 4, dtype=torch.float64, device='cuda')[::2])     # an accumulator is never copied
    with pytest.raises(ValueError, match='at most 4096'):
        ops.moments_accum(torch.zeros(2, 4097, device='cuda'), torch.zeros(4097, device='cuda'), s, g)
    with pytest.raises(ValueError, match='at least 2 fake rows'):
        _feed(np.zeros((5, 4), dtype=np.float32), [5]).result()
    assert frechet.Frechet(4).raw('fake')[0] == 0


# ---- 3. learners ---------------------------------------------------------------------------------------------------------
def test_progan_learner_reports_fd_and_kid(monkeypatch, capsys):
    from gan_lab_amd import frechet, kid, progressive as P
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_learner import make_learner
    from test_gpu_prdc import _fixed_loaders, _spy_features
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    torch.manual_seed(7)
    np.random.seed(7)
    L = make_learner('progan', 8, init_res=8, batch=4, gen_metrics=['generator loss', 'fd', 'kid'], disc_metrics=[], fd_res=4,
                     kid_res=8, kid_block=4, random_seed=4)
    z_dl, x_dl = _fixed_loaders(4, 8, 16)                    # 12 latents, 8 reals: two whole batches per set
    seen = _spy_features(monkeypatch)
    L.train(SyntheticImageLoader(64, 4, 8), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=2)
    out = capsys.readouterr().out
    got = L.last_metrics['generator']
    assert 'fd:' in out and 'kid:' in out and 'generator loss:' in out and np.isfinite(got['generator loss'])
    # the rows it fed, per batch (fd fake, fd real, kid fake, kid real), through evaluations of our own
    assert [tuple(s.shape) for s in seen] == [(4, 48), (4, 48), (4, 192), (4, 192)] * 2
    fd, kd = frechet.Frechet(48), kid.KID(192, 8, 8, block=4)
    for i, rows in enumerate(seen):
        ev = fd if i % 4 < 2 else kd
        (ev.feed_real if i % 2 else ev.feed_fake)(rows)
    assert fd.result() == got['fd'] and kd.result() == got['kid']
    assert (got['kid']['blocks'], got['kid']['n_real'], got['fd']['n_fake']) == (2, 8, 8)
    assert torch.equal(seen[3], x_dl.batches[0][0].cuda().reshape(4, -1))         # 8x8, no fade-in: the reals as they are
    assert L.gen_model.training and L.disc_model.training
    for name in ('fd', 'kid'):
        with pytest.raises(ValueError, match='valid_dl'):
            L.compute_metrics([name], 'Generator', z_dl, None)
        with pytest.raises(ValueError, match='generator metric'):
            L.compute_metrics([name], 'Discriminator', z_dl, x_dl)
        with pytest.raises(ValueError, match='at least one whole batch'):
            L.compute_metrics([name], 'Generator', z_dl, _fixed_loaders(3, 8, 16, n_x_batches=1)[1])


def test_resnet_learner_reports_fd_and_kid_and_leaves_prdc_alone(capsys):
    from gan_lab_amd import frechet, kid, prdc, rng
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    from test_gpu_prdc import SCORES, _fixed_loaders, _resnet_learner
    z_dl, x_dl = _fixed_loaders(8, 32, 32)                   # 24 latents, 16 reals: two whole batches per set
    L = _resnet_learner(gen_metrics=['prdc', 'fd', 'kid'], prdc_k=3, prdc_res=8, fd_res=8, kid_res=16, kid_block=8)
    L.set_requires_grad_disc(False)
    L.g_step()
    L.set_requires_grad_disc(True)

    # without the two names: what it reported before, and nothing of theirs is allocated
    offset = rng._STATE['offset']
    lines = L.compute_metrics(['prdc'], 'Generator', z_dl, x_dl)
    assert [ln.split(':')[0].strip() for ln in lines] == list(SCORES) and set(L._metric_evals) == {'prdc'}
    alone = L.last_metrics['generator']
    assert set(alone) == {'prdc'}
    pr = prdc.PRDC(3 * 8 * 8, 16, 16, k=3)
    for (zb,), (xb, _) in zip(z_dl.batches[:2], x_dl.batches):
        pr.feed_fake(prdc.features(L.generate(zs=zb.cuda(), truncation=None, time_average=True), 8))
        pr.feed_real(prdc.features(xb.cuda(), 8))
    rng._STATE['offset'] = offset
    assert pr.result() == alone['prdc']

    # with them: an evaluation of our own over generate()'s images; the process stream is where it was
    lines = L.compute_metrics(['prdc', 'fd', 'kid'], 'Generator', z_dl, x_dl)
    assert rng._STATE['offset'] == offset
    got = L.last_metrics['generator']
    assert [ln.split(':')[0].strip() for ln in lines] == list(SCORES) + ['fd', 'kid'] and got['prdc'] == alone['prdc']
    fd, kd = frechet.Frechet(3 * 8 * 8), kid.KID(3 * 16 * 16, 16, 16, block=8)
    for (zb,), (xb, _) in zip(z_dl.batches[:2], x_dl.batches):
        xgen = L.generate(zs=zb.cuda(), truncation=None, time_average=True)
        for ev, res in ((fd, 8), (kd, 16)):
            ev.feed_fake(prdc.features(xgen, res))
            ev.feed_real(prdc.features(xb.cuda(), res))
    rng._STATE['offset'] = offset
    assert fd.result() == got['fd'] and kd.result() == got['kid']
    assert (got['kid']['blocks'], got['fd']['n_real']) == (2, 16) and got['fd']['fd'] > 0
    assert L.gen_model.training

    for name in ('fd', 'kid'):
        with pytest.raises(ValueError, match='valid_dl'):
            L.compute_metrics([name], 'Generator', z_dl, None)
        with pytest.raises(ValueError, match='generator metric'):
            L.compute_metrics([name], 'Discriminator', z_dl, x_dl)
    with pytest.raises(ValueError, match='fake realness'):
        L.compute_metrics(['fd', 'fake realness'], 'Generator', z_dl, x_dl)

    # train() with both loaders evaluates all three at iteration 0
    L.last_metrics.clear()
    capsys.readouterr()
    L.train(SyntheticImageLoader(64, 8, 32), valid_dl=x_dl, z_valid_dl=z_dl, num_main_iters=1)
    printed = capsys.readouterr().out
    assert set(L.last_metrics['generator']) == {'prdc', 'fd', 'kid'} and 'fd:' in printed and 'kid:' in printed
