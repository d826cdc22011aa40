"""Host-side tests of the sampling side of the ResNet GAN (gan_lab_amd/sampling.py): config fields and validation, the
reference's own truncated normal (tests/sample_reference.py) against the bar the GPU draw is held to, the averaged generator's
construction, and checkpoints with and without it."""
import math

import numpy as np
import pytest
import torch

import sample_reference as ref

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)
NEW_FIELDS = ('ewma_decay', 'ewma_start', 'truncation', 'standing_stat_batches')


def _config(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', **{**COMMON, **kw})


def _learner(**kw):
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = _config(batch_size=4, len_latent=32, num_iters_save_model=10 ** 9, log_every=0, random_seed=1, **kw)
    cfg.fmap_g = cfg.fmap_d = 16
    torch.manual_seed(1)
    return GANLearner(cfg)


def test_config_defaults():
    from gan_lab_amd import sampling
    from gan_lab_amd.config import _float_or_none, _spec
    cfg = _config()
    assert cfg.use_ewma_gen is False and cfg.ewma_decay == 0.9999 and cfg.ewma_start == 0
    assert cfg.truncation is None and cfg.standing_stat_batches == 16
    assert sampling.validate_config(cfg) == (False, 0.9999, 0, None, 16)
    assert sampling.validate_config(_config(use_ewma_gen=True, ewma_decay=0, ewma_start=3, truncation=0.5,
                                            standing_stat_batches=1)) == (True, 0.0, 3, 0.5, 1)
    rows = {row[0]: row[1:] for row in _spec('ResNet GAN')}
    assert rows['use_ewma_gen'] == (bool, False) and rows['ewma_decay'] == (float, 0.9999) and rows['ewma_start'] == (int, 0)
    assert rows['truncation'] == (_float_or_none, None) and rows['standing_stat_batches'] == (int, 16)
    for model in ('ProGAN', 'StyleGAN'):              # the progressive models keep their own use_ewma_gen and get nothing new
        rows = {row[0]: row[1:] for row in _spec(model)}
        assert rows['use_ewma_gen'] == (bool, True)
        assert not any(k in rows for k in NEW_FIELDS)


@pytest.mark.parametrize('field,bad', [
    ('use_ewma_gen', 1), ('use_ewma_gen', 'yes'), ('use_ewma_gen', None),
    ('ewma_decay', 1.0), ('ewma_decay', -0.1), ('ewma_decay', float('nan')), ('ewma_decay', '0.5'), ('ewma_decay', None),
    ('ewma_decay', True), ('ewma_decay', 1.0 - 1e-12),
    ('ewma_start', -1), ('ewma_start', 1.5), ('ewma_start', True), ('ewma_start', None),
    ('truncation', 0.0), ('truncation', -1.0), ('truncation', float('inf')), ('truncation', float('nan')), ('truncation', 'x'),
    ('truncation', 1e-60),
    ('standing_stat_batches', 0), ('standing_stat_batches', -3), ('standing_stat_batches', 2.0), ('standing_stat_batches', None),
])
def test_invalid_values_raise_when_the_learner_is_built(monkeypatch, field, bad):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd import sampling
    cfg = _config()
    setattr(cfg, field, bad)
    with pytest.raises(ValueError, match=field if field != 'truncation' else 'truncation'):
        sampling.validate_config(cfg)
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = _config(batch_size=4, len_latent=32, log_every=0)
    cfg.fmap_g = cfg.fmap_d = 16
    setattr(cfg, field, bad)
    with pytest.raises(ValueError):
        GANLearner(cfg)


def test_truncation_threshold_is_checked_before_any_launch():
    from gan_lab_amd import ops, rng
    for bad in (0, -0.5, float('inf'), float('nan'), None, 'half'):
        with pytest.raises(ValueError):
            ops.trunc_randn((4,), bad, 1, 0, 'cpu')
        with pytest.raises(ValueError):
            rng.trunc_randn((4,), bad, 'cpu')
    with pytest.raises(TypeError):          # a good threshold, no GPU tensor: no CPU path
        ops.trunc_randn((4,), 0.5, 1, 0, 'cpu')


def test_trunc_randn_refuses_a_step_graph_capture():
    from gan_lab_amd import rng
    before = rng._STATE['offset']
    rng.begin_device_offsets(object())
    try:
        with pytest.raises(RuntimeError, match='captured'):
            rng.trunc_randn((4,), 0.5, 'cpu')
    finally:
        rng.end_device_offsets()
    assert rng._STATE['offset'] == before


@pytest.mark.parametrize('t', [0.5, 1.0, 2.0])
def test_reference_inverse_cdf_stays_inside_the_bar(t):
    """The reference alone, on uniforms from numpy on the device's lattice ((k + 1/2) 2^-23), at the GPU test's size."""
    n = 1 << 20
    k = np.random.default_rng(20240 + int(10 * t)).integers(0, 1 << 23, size=n)
    x = ref.trunc_icdf((k + 0.5) * 2.0 ** -23, t)
    assert np.all(np.abs(x) <= t)
    d, bound = ref.ks_distance(x, t), ref.ks_bound(n)
    print(f't={t}: KS {d:.3e} (bound {bound:.3e}), var {x.var():.6f} vs {ref.trunc_var(t):.6f}')
    assert abs(bound - 2.63e-3) < 1e-5
    assert d <= bound
    assert abs(x.var() / ref.trunc_var(t) - 1.0) <= 0.01


def test_reference_pieces_agree_with_each_other():
    for t in (0.5, 1.0, 2.0):
        u = np.linspace(0.001, 0.999, 999)
        assert np.allclose(ref.trunc_cdf(ref.trunc_icdf(u, t), t), u, atol=1e-12)
        xs = np.linspace(-t, t, 200001)                      # the variance formula against a quadrature of x^2 dF
        pdf = np.exp(-0.5 * xs * xs) / math.sqrt(2 * math.pi) / math.erf(t / math.sqrt(2))
        f = xs * xs * pdf
        assert abs(float(np.sum((f[1:] + f[:-1]) * 0.5 * np.diff(xs))) - ref.trunc_var(t)) < 1e-8
    u = ref.stream_uniforms(0x0123456789ABCDEF, 2 ** 32 - 1, 9)
    assert u.shape == (9,) and np.all((u > 0) & (u < 1))
    assert np.array_equal(u[:5], ref.stream_uniforms(0x0123456789ABCDEF, 2 ** 32 - 1, 5))
    # the start rule: with start = 2, update 1 copies, updates 2 and 3 average
    got = ref.ema_replay([8.0], [[1.0], [3.0], [5.0]], 0.5, 2)
    assert got.tolist() == [0.5 * (0.5 * 1.0 + 0.5 * 3.0) + 0.5 * 5.0]
    assert ref.ema_replay([8.0], [[1.0], [3.0]], 0.5, 0).tolist() == [0.5 * (0.5 * 8.0 + 0.5 * 1.0) + 0.5 * 3.0]
    xs = [torch.randn(4, 3, 2, 2, generator=torch.Generator().manual_seed(s)) for s in range(3)]
    mean, var, count = ref.cumulative_bn_stats(xs)
    want_mean = torch.stack([x.double().mean((0, 2, 3)) for x in xs]).mean(0)
    want_var = torch.stack([x.double().transpose(0, 1).reshape(3, -1).var(1, unbiased=True) for x in xs]).mean(0)
    assert count == 3 and torch.allclose(mean, want_mean, atol=1e-14) and torch.allclose(var, want_var, atol=1e-14)


@pytest.mark.parametrize('kw', [dict(), dict(hier_latent=True, shared_embed=8, cgan='projection', num_classes=3)],
                         ids=['plain', 'hier'])
def test_averaged_generator_is_a_copy_in_its_own_arena(monkeypatch, kw):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    L = _learner(use_ewma_gen=True, ewma_decay=0.5, ewma_start=2, **kw)
    e = L.gen_ema
    assert e is not None and e.model is not L.gen_model and not e.model.training
    assert not any(p.requires_grad for p in e.model.parameters())
    assert e.arena.names == L.arena_g.names and e.arena.offsets == L.arena_g.offsets
    lo = e.arena.flat.data_ptr()
    assert all(lo <= p.data_ptr() < lo + 4 * e.arena.total for p in e.model.parameters())
    assert e.arena.flat.data_ptr() != L.arena_g.flat.data_ptr() and torch.equal(e.arena.flat, L.arena_g.flat)
    assert [e.decay_of_update(j) for j in (1, 2, 3)] == [0.0, 0.5, 0.5]
    if kw:      # the copy's modulation manager is its own, over its own modules, and holds no table of the live generator
        h = e.model.hier
        assert h is not L.gen_model.hier and h.generator is e.model and h.table is None
        own = set(e.model.modules())
        assert all(m in own for m, _, _ in h.norms)
    assert _learner(**kw).gen_ema is None


def test_checkpoints_with_and_without_the_averaged_generator(monkeypatch, tmp_path):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    off = _learner()
    off.not_trained_yet = False
    off.save_model(tmp_path / 'off.tar')
    ck_off = torch.load(tmp_path / 'off.tar', weights_only=False)
    assert 'gen_ema_state_dict' not in ck_off and 'ewma_updates' not in ck_off
    assert not any(k in ck_off['config'] for k in ('use_ewma_gen',) + NEW_FIELDS)       # the keys of before the options

    L = _learner(use_ewma_gen=True, ewma_decay=0.5, truncation=0.7)
    with torch.no_grad():
        L.gen_ema.arena.flat.mul_(0.5)
        L.gen_ema.updates = 5
    L.not_trained_yet = False
    with pytest.raises(ValueError, match='reference_format'):
        L.save_model(tmp_path / 'ref.tar', reference_format=True)
    L.save_model(tmp_path / 'on.tar')
    ck = torch.load(tmp_path / 'on.tar', weights_only=False)
    assert set(ck) - set(ck_off) == {'gen_ema_state_dict', 'ewma_updates'} and ck['ewma_updates'] == 5
    assert ck['config']['use_ewma_gen'] is True and ck['config']['ewma_decay'] == 0.5 and ck['config']['truncation'] == 0.7
    assert list(ck['gen_ema_state_dict']) == list(ck['gen_model_state_dict'])
    want = L.gen_ema.arena.flat.clone()
    with torch.no_grad():
        L.gen_ema.arena.flat.zero_()
    L.gen_ema.updates = 0
    L.load_model(tmp_path / 'on.tar')
    assert torch.equal(L.gen_ema.arena.flat, want) and L.gen_ema.updates == 5
    assert L.gen_ema.arena_src is L.arena_g and not torch.equal(L.gen_ema.arena.flat, L.arena_g.flat)
    # a checkpoint written without the copy (before the option existed) loads: a fresh copy of the loaded generator
    L.load_model(tmp_path / 'off.tar')
    assert torch.equal(L.gen_ema.arena.flat, L.arena_g.flat) and L.gen_ema.updates == 0
    for (k, a), (_, b) in zip(L.gen_ema.model.state_dict().items(), L.gen_model.state_dict().items()):
        assert torch.equal(a, b), k
