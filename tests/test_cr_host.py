"""Host-side tests of consistency regularisation (gan_lab_amd/consistency.py): config fields, CLI flags and validation, and the
float64 reference (tests/cr_reference.py) against itself - the transform's identities, the gradients against finite differences."""
import numpy as np
import pytest
import torch

import cr_reference as ref

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)
FIELDS = ('cr_real', 'cr_fake', 'cr_latent_d', 'cr_latent_g', 'cr_sigma', 'cr_shift', 'cr_flip')


def _config(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', **{**COMMON, **kw})


# ---- 1: defaults and the command line ----------------------------------------------------------------------------------------
def test_defaults_and_cli_round_trip(monkeypatch, tmp_path):
    from gan_lab_amd import config, consistency
    cfg = _config()
    assert tuple(getattr(cfg, f) for f in FIELDS) == (0., 0., 0., 0., 0.03, None, True)
    assert consistency.validate_config(cfg) is None                       # all weights 0: the feature is off
    rows = {row[0]: row[1:] for row in config._spec('ResNet GAN')}
    assert all(rows[f] == (float, 0.) for f in FIELDS[:4]) and rows['cr_sigma'] == (float, 0.03)
    assert rows['cr_shift'] == (config._int_or_none, None) and rows['cr_flip'] == (bool, True)
    for model in ('ProGAN', 'StyleGAN'):
        assert not any(row[0].startswith('cr_') for row in config._spec(model))
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['resnetgan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(args)
    assert tuple(getattr(c, f) for f in FIELDS) == (0., 0., 0., 0., 0.03, None, True)
    c = config.main(args + ['--cr_real=10', '--cr_fake', '10', '--cr_latent_d=5', '--cr_latent_g=0.5', '--cr_sigma=0.05',
                            '--cr_shift=3', '--cr_flip=False'])
    assert tuple(getattr(c, f) for f in FIELDS) == (10., 10., 5., 0.5, 0.05, 3, False)
    assert all(isinstance(getattr(c, f), float) for f in FIELDS[:5]) and isinstance(c.cr_shift, int)
    assert config.main(args + ['--cr_shift=none']).cr_shift is None
    assert config.main(args + ['--cr_shift=None', '--cr_flip']).cr_flip is True
    on = consistency.validate_config(_config(cr_real=10., cr_latent_g=0.5))
    assert (on.real, on.fake, on.latent_d, on.latent_g, on.sigma, on.shift, on.flip) == (10., 0., 0., 0.5, 0.03, 4, True)
    assert consistency.validate_config(_config(cr_fake=1., res_samples=64, res_dataset=64)).shift == 8
    assert consistency.validate_config(_config(cr_fake=1., cr_shift=0, cr_flip=False)).shift == 0


def test_checkpoint_config_is_unchanged_while_off():
    from gan_lab_amd import consistency
    cfg = vars(_config())
    assert not any(k.startswith('cr_') for k in consistency.saved_config_fields(cfg))
    on = consistency.saved_config_fields(vars(_config(cr_latent_d=5.)))
    assert all(f in on for f in FIELDS)


# ---- 2: every ValueError --------------------------------------------------------------------------------------------------------
BAD = [(dict(cr_real=-1.), 'cr_real'), (dict(cr_fake=float('nan')), 'cr_fake'), (dict(cr_latent_d=float('inf')), 'cr_latent_d'),
       (dict(cr_latent_g=-0.5), 'cr_latent_g'), (dict(cr_real='1'), 'cr_real'), (dict(cr_fake=True), 'cr_fake'),
       (dict(cr_latent_d=1., cr_sigma=0.), 'cr_sigma'), (dict(cr_latent_g=1., cr_sigma=-0.03), 'cr_sigma'),
       (dict(cr_real=1., cr_sigma=float('nan')), 'cr_sigma'),
       (dict(cr_real=1., cr_shift=-1), 'cr_shift'), (dict(cr_fake=1., cr_shift=32), 'cr_shift'),
       (dict(cr_fake=1., cr_shift=2.5), 'cr_shift'),
       (dict(cr_real=1., cr_flip=1), 'cr_flip'),
       (dict(cr_real=1., diffaugment='color'), 'diffaugment'), (dict(cr_latent_g=1., diffaugment='translation'), 'diffaugment'),
       (dict(cr_fake=1., ada='blit'), 'ada'), (dict(cr_latent_d=1., ada='blit,geom'), 'ada')]


@pytest.mark.parametrize('kw,match', BAD, ids=[f'{m}-{i}' for i, (_, m) in enumerate(BAD)])
def test_invalid_values_raise_when_the_learner_is_built(monkeypatch, kw, match):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd import consistency
    from gan_lab_amd.resnetgan.learner import GANLearner
    with pytest.raises(ValueError, match=match):
        consistency.validate_config(_config(**kw))
    cfg = _config(batch_size=4, len_latent=32, log_every=0, **kw)
    cfg.fmap_g = cfg.fmap_d = 16
    with pytest.raises(ValueError, match=match):
        GANLearner(cfg)


def test_sigma_is_not_checked_without_a_latent_weight():
    from gan_lab_amd import consistency
    assert consistency.validate_config(_config(cr_real=1., cr_sigma=0.)).sigma == 0.
    assert consistency.validate_config(_config(cr_sigma=-1.)) is None           # the feature is off


@pytest.mark.parametrize('model', ['progan', 'stylegan'])
def test_progressive_models_have_no_such_field(model):
    from gan_lab_amd import consistency
    from gan_lab_amd.config import make_config
    for field in FIELDS:
        with pytest.raises(AttributeError, match=field):
            make_config(model, **{field: 1.})
    cfg = make_config(model, dev='cpu', pin_memory=False)
    assert consistency.validate_config(cfg) is None
    cfg.cr_real = 1.                                # set behind make_config's back: a progressive model with a positive weight
    with pytest.raises(ValueError, match='ResNet GAN'):
        consistency.validate_config(cfg)


def test_off_learner_builds_nothing(monkeypatch):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd import rng
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = _config(batch_size=4, len_latent=32, log_every=0, random_seed=1)
    cfg.fmap_g = cfg.fmap_d = 16
    L = GANLearner(cfg)
    assert L.cr is None and rng._STATE['offset'] == 0
    cfg = _config(batch_size=4, len_latent=32, log_every=0, random_seed=1, cr_real=10., cr_fake=10., cr_latent_d=5.,
                  cr_latent_g=0.5)
    cfg.fmap_g = cfg.fmap_d = 16
    L = GANLearner(cfg)
    assert (L.cr.real, L.cr.fake, L.cr.latent_d, L.cr.latent_g, L.cr.shift) == (10., 10., 5., 0.5, 4)


def test_ops_have_no_cpu_path():
    from gan_lab_amd import ops
    a = torch.zeros(4)
    for call in (lambda: ops.cr_msd(a, a), lambda: ops.cr_imsd(a.view(1, 1, 2, 2), a.view(1, 1, 2, 2)),
                 lambda: ops.cr_imsd(a.view(2, 1, 1, 2)), lambda: ops.cr_transform(a.view(1, 1, 2, 2), torch.zeros(1, 4).int()),
                 lambda: ops.cr_params(4, 1, True, 0, 0, 'cpu')):
        with pytest.raises(TypeError, match='no CPU fallback'):
            call()


# ---- 3: the reference against itself ---------------------------------------------------------------------------------------------
def _images(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


def test_transform_identity_and_double_flip():
    x = _images((3, 2, 5, 7), 0)
    zero = np.zeros((3, 4), dtype=np.int32)
    assert np.array_equal(ref.transform(x, zero), x)
    flip = zero.copy()
    flip[:, 0] = 1
    once = ref.transform(x, flip)
    assert np.array_equal(once, x[:, :, :, ::-1]) and not np.array_equal(once, x)
    assert np.array_equal(ref.transform(once, flip), x)
    mixed = zero.copy()
    mixed[1, 0] = 1                                # per image: only image 1 is mirrored
    y = ref.transform(x, mixed)
    assert np.array_equal(y[0], x[0]) and np.array_equal(y[1], x[1][:, :, ::-1]) and np.array_equal(y[2], x[2])


@pytest.mark.parametrize('dx,dy', [(2, 1), (-3, 2), (0, -2), (3, 0), (-1, -1)])
def test_shift_and_back_is_the_identity_on_the_interior(dx, dy):
    h, w = 6, 8
    x = _images((2, 3, h, w), 1)
    there = np.array([[0, dx, dy, 0]] * 2, dtype=np.int32)
    back = np.array([[0, -dx, -dy, 0]] * 2, dtype=np.int32)
    moved = ref.transform(x, there)
    assert np.array_equal(moved[:, :, max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)],
                          x[:, :, max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)])      # a shift by (dx, dy)
    y = ref.transform(moved, back)
    keep = np.zeros((h, w), dtype=bool)             # what survived the trip: not pushed out on the way there
    keep[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)] = True
    assert np.array_equal(y[:, :, keep], x[:, :, keep])
    assert np.all(y[:, :, ~keep] == 0) and (~keep).sum() == h * w - (h - abs(dy)) * (w - abs(dx))


def test_shift_past_the_image_leaves_zeros_and_flip_composes():
    x = _images((1, 1, 4, 4), 2)
    assert np.all(ref.transform(x, np.array([[0, 4, 0, 0]])) == 0) and np.all(ref.transform(x, np.array([[1, 0, -4, 0]])) == 0)
    y = ref.transform(x, np.array([[1, 1, 0, 0]]))          # mirror, then one pixel to the right
    assert np.all(y[..., 0] == 0) and np.array_equal(y[..., 1:], x[..., ::-1][..., :3])


@pytest.mark.parametrize('shape', [(1,), (5,), (7, 1), (2, 3, 4, 5)])
def test_gradients_match_finite_differences(shape):
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    fn, grads = (ref.msd, ref.msd_grads) if len(shape) <= 2 else (ref.imsd, ref.imsd_grads)
    ta, tb = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    value = fn(ta, tb)
    assert abs(value.item() - np.mean((a - b) ** 2)) <= 1e-15 * max(value.item(), 1.0)
    (1.7 * value).backward()
    ga, gb = grads(a, b, 1.7)
    assert np.allclose(ta.grad.numpy(), ga.reshape(shape), rtol=1e-13, atol=0) and np.array_equal(gb, -ga)
    assert np.allclose(tb.grad.numpy(), gb.reshape(shape), rtol=1e-13, atol=0)
    h = 1e-6
    for idx in list(np.ndindex(*shape))[:7]:
        for which, g in ((0, ga), (1, gb)):
            pa, pb, ma, mb = a.copy(), b.copy(), a.copy(), b.copy()
            (pa if which == 0 else pb)[idx] += h
            (ma if which == 0 else mb)[idx] -= h
            fd = 1.7 * (np.mean((pa - pb) ** 2) - np.mean((ma - mb) ** 2)) / (2 * h)
            assert abs(fd - g.reshape(shape)[idx]) <= 1e-8 * max(1.0, abs(fd))


def test_terms_on_toy_networks():
    """The term functions on a linear critic and generator, against the formulas written out."""
    torch.manual_seed(4)
    wd, wg = torch.randn(3 * 4 * 4).double(), torch.randn(3 * 4 * 4, 6).double()
    disc = lambda x: x.double().reshape(x.shape[0], -1) @ wd                          # noqa: E731
    gen = lambda z: (z.double() @ wg.t()).reshape(z.shape[0], 3, 4, 4)                # noqa: E731
    x, z, noise = torch.randn(2, 3, 4, 4).double(), torch.randn(2, 6).double(), torch.randn(2, 6).double()
    params = np.array([[1, 1, 0, 0], [0, 0, -1, 0], [0, 2, 1, 0], [1, 0, 0, 0]], dtype=np.int32)
    terms, (g_z, d_gen, d_real) = ref.critic_terms(disc, gen, x, z, noise, params, 0.03)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-13)      # a matmul over 4 rows rounds unlike one over 2  # noqa: E731
    assert close(g_z, gen(z)) and close(d_gen, disc(gen(z))) and torch.equal(d_real, disc(x))
    assert torch.allclose(terms['cr_real'], ((disc(x) - disc(ref.transform_t(x, params[2:]))) ** 2).mean(), rtol=1e-14)
    assert torch.allclose(terms['cr_fake'], ((d_gen - disc(ref.transform_t(g_z, params[:2]))) ** 2).mean(), rtol=1e-14)
    assert torch.allclose(terms['cr_latent_d'], ((d_gen - disc(gen(z + 0.03 * noise))) ** 2).mean(), rtol=1e-12)
    only, _ = ref.critic_terms(disc, gen, x, z, noise, params, 0.03, real=False, latent=False)
    assert list(only) == ['cr_fake']
    term, first = ref.generator_term(gen, z, noise, 0.03)
    assert close(first, gen(z)) and torch.allclose(term, ((gen(z) - gen(z + 0.03 * noise)) ** 2).mean(), rtol=1e-12)
