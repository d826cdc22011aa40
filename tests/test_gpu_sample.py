"""GPU tests of the sampling side of the ResNet GAN (csrc/sample.hip; gan_lab_amd/sampling.py): the truncated-normal draw, the
batched moving average, the averaged generator, standing statistics, ``learner.generate`` and checkpoints.

Bounds.  Distribution: the Kolmogorov bound at alpha = 1e-6 for n = 2^20, sqrt(ln(2 / 1e-6) / (2 n)) = 2.63e-3 - the draw is
deterministic, so this is a bar, not a flake budget - and 1 % on the variance.  Elementwise, against the float64 inverse CDF of the
restated Philox uniform: ELEM_ULPS fp32 ulps of t (2^-23 t each); measured on the MI355X 1.69 (t = 0.5), 1.98 (t = 1) and 2.14
(t = 2) ulps over the 4099-element draw - erfinvf plus the fp32 rounding of its argument, which the map stretches by
sqrt(pi / 2) exp(x^2 / 2) - and the bound is the 4x margin over the largest of them, 8.56.  ewma_many: one fp32 rounding
of the float64 result.  The averaged generator: the fp32 roundings of its three updates.  Standing statistics: 1e-6 relative (fp32
accumulation).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import sample_reference as ref
from util import rel_err

pytestmark = pytest.mark.gpu

SEED = 0x5A17ED0123456789
N_BIG = 1 << 20
ELEM_ULPS = 8.56        # 4 x the 2.14 ulps of t measured (module docstring)
THRESHOLDS = (0.5, 1.0, 2.0)
HIER = dict(hier_latent=True, shared_embed=8, cgan='projection', num_classes=3)


# ---- trunc_randn -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', THRESHOLDS)
def test_trunc_randn_distribution(t):
    from gan_lab_amd import ops
    x = ops.trunc_randn((N_BIG,), t, SEED, 12345, 'cuda')
    assert x.shape == (N_BIG,) and x.dtype == torch.float32
    x = x.cpu().numpy().astype(np.float64)
    d, bound, var = ref.ks_distance(x, t), ref.ks_bound(N_BIG), float(x.var())
    print(f't={t}: max|x| {np.abs(x).max():.7f}, KS {d:.3e} (bound {bound:.3e}), var {var:.6f} (analytic {ref.trunc_var(t):.6f})')
    assert np.all(np.abs(x) <= t)
    assert d <= bound
    assert abs(var / ref.trunc_var(t) - 1.0) <= 0.01


@pytest.mark.parametrize('t', THRESHOLDS)
def test_trunc_randn_elementwise_and_geometry(t):
    """Tails and sizes that are no multiple of 4, at an offset that crosses a 32-bit boundary of the counter: every element is
    the reference's map of the restated uniform, and a shorter draw is the prefix of a longer one."""
    from gan_lab_amd import ops
    offset = 2 ** 32 - 2
    want = ref.trunc_icdf(ref.stream_uniforms(SEED, offset, 4099), t)
    full = ops.trunc_randn((4099,), t, SEED, offset, 'cuda')
    worst = 0.0
    for n in (1, 3, 4, 5, 4099):
        got = ops.trunc_randn((n,), t, SEED, offset, 'cuda')
        assert torch.equal(got, full[:n]), n                       # geometry independence, bitwise
        err = np.abs(got.cpu().numpy().astype(np.float64) - want[:n]).max() / (2.0 ** -23 * t)
        worst = max(worst, err)
        print(f't={t} n={n}: max error {err:.2f} ulps of t')
    assert worst <= ELEM_ULPS
    assert torch.equal(ops.trunc_randn((4099,), t, SEED, offset, 'cuda'), full)       # two runs, bitwise
    shifted = ops.trunc_randn((8,), t, SEED, offset + 1, 'cuda')                       # one counter on = four elements on
    assert torch.equal(shifted, full[4:12])
    unaligned = torch.empty(4099 + 1, device='cuda')[1:]                                  # the scalar-store path: same values
    from gan_lab_amd import _lib
    import ctypes
    _lib.check(_lib.lib().ganlab_trunc_randn_f32(ctypes.c_void_p(unaligned.data_ptr()), 4099, t, SEED, offset, ops._st()), 'trunc')
    assert torch.equal(unaligned, full)


def test_rng_trunc_randn_advances_the_stream_like_randn():
    from gan_lab_amd import ops, rng
    saved = dict(rng._STATE)
    try:
        for shape in ((1,), (3, 5), (4, 32), (7, 11, 3)):
            rng.manual_seed(99)
            rng.randn((5,))
            start = rng._STATE['offset']
            rng.randn(shape)
            step = rng._STATE['offset'] - start
            after_plain = rng.randn((8,))
            rng.manual_seed(99)
            rng.randn((5,))
            got = rng.trunc_randn(shape, 0.75)
            assert rng._STATE['offset'] - start == step == (int(np.prod(shape)) + 3) // 4
            assert torch.equal(got, ops.trunc_randn(shape, 0.75, rng._STATE['seed'], start, 'cuda'))
            assert torch.equal(rng.randn((8,)), after_plain)         # whatever follows sees the same stream
            assert tuple(got.shape) == shape and float(got.abs().max()) <= 0.75
        with pytest.raises(ValueError):
            rng.trunc_randn((4,), 0.0)
    finally:
        rng._STATE.update(saved)


# ---- ewma_many -----------------------------------------------------------------------------------------------------------------
def _segments(counts, seed):
    g = torch.Generator().manual_seed(seed)
    lag = [torch.randn(c, generator=g).cuda() for c in counts]
    src = [(torch.randn(c, generator=g) * 3).cuda() for c in counts]
    return lag, src


@pytest.mark.parametrize('counts', [(1000,), (1, 3, 64, 1000, 3, 64, 1)], ids=['1job', '7jobs'])
def test_ewma_many_against_float64(counts):
    from gan_lab_amd import ops
    decay = 0.9
    lag, src = _segments(counts, 3)
    lag2 = [a.clone() for a in lag]
    d32 = float(np.float32(decay))
    want = [d32 * a.double().cpu() + (1.0 - d32) * b.double().cpu() for a, b in zip(lag, src)]
    src_before = [b.clone() for b in src]
    ops.ewma_many(ops.EwmaTable(list(zip(lag, src))), decay)
    ops.ewma_many(ops.EwmaTable(list(zip(lag2, src))), decay)
    for a, a2, b, b0, w in zip(lag, lag2, src, src_before, want):
        err = ((a.double().cpu() - w).abs() / w.abs().clamp_min(2.0 ** -126)).max().item()
        print(f'count {a.numel()}: max relative error {err:.3e} (one rounding: {2.0 ** -24:.3e})')
        assert err <= 2.0 ** -24 * (1 + 1e-6)
        assert torch.equal(a, a2) and torch.equal(b, b0)             # bitwise reproducible; the source is only read


def test_ewma_many_decay_zero_copies_bitwise_even_over_nan():
    from gan_lab_amd import ops
    lag, src = _segments((1, 3, 64, 1000), 5)
    for a in lag:
        a.fill_(float('nan'))
    lag[2][::2] = float('inf')
    src[3][17] = -0.0
    table = ops.EwmaTable(list(zip(lag, src)))
    ops.ewma_many(table, 0.0)
    for a, b in zip(lag, src):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        ops.ewma_many(table, 1.0)
    with pytest.raises(ValueError):
        ops.ewma_many(table, -0.5)


# ---- the learner ---------------------------------------------------------------------------------------------------------------
def _learner(**kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    kw.setdefault('random_seed', 7)
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=1, len_latent=32, **kw)
    cfg.fmap_g, cfg.fmap_d = 16, 16
    torch.manual_seed(7)
    return GANLearner(cfg)


def _latents(step):
    return torch.randn(4, 32, generator=torch.Generator().manual_seed(100 + step)).cuda()


def _state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _three_steps(L):
    """3 generator updates on fixed latents -> the generator's state before them and after each."""
    L.gen_model.train()
    L.set_requires_grad_disc(False)
    snaps = [_state(L.gen_model)]
    for step in range(3):
        L.g_step(zb=_latents(step))
        snaps.append(_state(L.gen_model))
    return snaps


@pytest.mark.parametrize('kw', [dict(), HIER], ids=['plain', 'hier'])
def test_generator_ema_follows_the_recurrence_and_leaves_training_alone(kw):
    L = _learner(use_ewma_gen=True, ewma_start=2, ewma_decay=0.5, **kw)
    snaps = _three_steps(L)
    ema = L.gen_ema.state_dict()
    assert ema['updates'] == 3
    worst = 0.0
    for k, got in ema['model'].items():
        series = [s[k].double().cpu().numpy() for s in snaps]
        if not got.dtype.is_floating_point:                      # num_batches_tracked: copied, not averaged
            assert torch.equal(got, snaps[-1][k].cpu()), k
            continue
        want = ref.ema_replay(series[0], series[1:], 0.5, 2)
        scale = np.max(np.abs(np.stack(series)), axis=0)
        # update 1 copies; updates 2 and 3 each round two products and a sum of values up to `scale`: 3 roundings each
        diff = np.abs(got.double().numpy() - want)
        worst = max(worst, float((diff / np.maximum(2.0 ** -24 * scale, 1e-300)).max()))
        assert np.all(diff <= 6 * 2.0 ** -24 * scale), (k, float(diff.max()))
    moved = max(float((snaps[3][k].double() - snaps[0][k].double()).abs().max()) for k in snaps[0]
                if snaps[0][k].dtype.is_floating_point)
    print(f'{len(ema["model"])} tensors: worst error {worst:.2f} roundings (bound 6); the generator moved by up to {moved:.3e}')
    assert moved > 1e-5
    # the hook changes nothing in training: the same seed without the copy gives the same generator, bit for bit
    base = _three_steps(_learner(**kw))
    for k, v in snaps[3].items():
        assert torch.equal(v, base[3][k]), k
    # ... and the averaged copy is another network than the live one
    z = _latents(9)
    labels = torch.tensor([0, 2, 1, 2]) if kw else None
    avg, live = L.generate(zs=z, labels=labels, time_average=True), L.generate(zs=z, labels=labels, time_average=False)
    assert L.gen_model.training and not L.gen_ema.model.training
    assert avg.shape == live.shape == (4, 3, 32, 32) and bool(torch.isfinite(avg).all()) and not torch.equal(avg, live)
    if kw:      # the copy's modulation reads the copy's arena: every weight of its job table lies there, none in the live arena
        lo = L.gen_ema.arena.flat.data_ptr()
        table = L.gen_ema.model.hier.table
        assert table is not L.gen_model.hier.table
        assert all(lo <= w.data_ptr() < lo + 4 * L.gen_ema.arena.total for w in table.weights + [table.shared])
        # its gains and shifts are those of the AVERAGED linears: the same forward on a deep copy that never saw the live arena
        import copy
        twin = copy.deepcopy(L.gen_ema.model)
        twin.hier.table = None
        with torch.no_grad():
            assert torch.equal(twin(z, L._device_labels(labels, 4, draw=True)), avg)


@pytest.mark.parametrize('kw', [dict(), HIER, dict(cgan='projection', num_classes=3)], ids=['plain', 'hier', 'cbn'])
def test_standing_stats_are_the_plain_average_of_the_batch_statistics(kw):
    from gan_lab_amd import sampling
    L = _learner(**kw)
    gen = L.gen_model.eval()
    norms = sampling._norms(gen)
    assert len(norms) == 7
    seen = {m: [] for m in norms}
    hooks = [m.register_forward_hook(lambda mod, args, out: seen[mod].append(args[0].detach().clone())) for m in norms]
    for i, m in enumerate(norms):
        m.momentum = 0.1 + 0.01 * i
    try:
        sampling.standing_stats(gen, 3, 4, 32, truncation=1.0)
    finally:
        for h in hooks:
            h.remove()
    worst = 0.0
    for i, m in enumerate(norms):
        assert len(seen[m]) == 3 and m.momentum == 0.1 + 0.01 * i and not m.training
        mean, var, count = ref.cumulative_bn_stats(seen[m])
        e_m, e_v = rel_err(m.running_mean, mean), rel_err(m.running_var, var)
        worst = max(worst, e_m, e_v)
        assert int(m.num_batches_tracked) == count == 3
        assert e_m <= 1e-6 and e_v <= 1e-6, (i, e_m, e_v)
    print(f'{len(norms)} norms: worst relative error {worst:.3e}')
    assert not any(m.training for m in gen.modules())
    with pytest.raises(ValueError):
        sampling.standing_stats(gen, 0, 4, 32)


def test_generate_truncated_reproducible_and_mode_preserving():
    from gan_lab_amd import rng
    L = _learner(use_ewma_gen=True, truncation=0.5, standing_stat_batches=2)
    L.gen_model.train()
    rng.manual_seed(5)
    a = L.generate(n=4, truncation=0.5)
    b = L.generate(n=4, truncation=0.5, time_average=False, standing_stats=True)
    end = rng._STATE['offset']
    assert a.shape == b.shape == (4, 3, 32, 32) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert not a.requires_grad and L.gen_model.training and not L.gen_ema.model.training
    assert end == 32 + 32 + 2 * 32          # 4 x 32 latents = 32 counters per draw: two draws and two standing-statistics batches
    rng.manual_seed(5)
    assert torch.equal(L.generate(n=4), a)                          # the default truncation is config.truncation
    rng.manual_seed(5)
    z = rng.trunc_randn((4, 32), 0.5)
    assert torch.equal(L.generate(zs=z), a) and float(z.abs().max()) <= 0.5
    rng.manual_seed(5)
    assert not torch.equal(L.generate(n=4, truncation=None), a)
    L.gen_model.eval()
    L.generate(n=2, time_average=False)
    assert not L.gen_model.training
    with pytest.raises(ValueError):
        L.generate(n=4, truncation=-1.0)
    with pytest.raises(ValueError):
        L.generate(zs=z, n=3)
    plain = _learner()                                               # no copy: time_average falls back to the live generator
    assert plain.gen_ema is None and plain.generate(n=3).shape == (3, 3, 32, 32)


def test_checkpoint_round_trip_restores_the_copy_bit_for_bit(tmp_path):
    L = _learner(use_ewma_gen=True, ewma_decay=0.5, **HIER)
    _three_steps(L)
    L.not_trained_yet = False
    L.save_model(tmp_path / 'm.tar')
    want, flat = L.gen_ema.state_dict(), L.gen_ema.arena.flat.clone()
    z, labels = _latents(3), torch.tensor([1, 0, 2, 2])
    img = L.generate(zs=z, labels=labels)
    M = _learner(use_ewma_gen=True, ewma_decay=0.5, random_seed=8, **HIER)
    assert not torch.equal(M.gen_ema.arena.flat, flat)
    M.load_model(tmp_path / 'm.tar')
    got = M.gen_ema.state_dict()
    assert got['updates'] == want['updates'] == 3 and list(got['model']) == list(want['model'])
    for k, v in want['model'].items():
        assert torch.equal(got['model'][k], v), k
    assert torch.equal(M.gen_ema.arena.flat, flat) and M.gen_ema.arena_src is M.arena_g
    assert torch.equal(M.generate(zs=z, labels=labels), img)
    M.set_requires_grad_disc(False)
    M.g_step(zb=_latents(4))                                         # the restored copy keeps averaging the rebuilt arena
    assert M.gen_ema.updates == 4 and not torch.equal(M.gen_ema.arena.flat, flat)
