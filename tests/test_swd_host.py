"""Host-side tests of the sliced Wasserstein metric (gan_lab_amd/swd.py): the float64 numpy reference on its
own, the config options and their CLI flags, the learners' and the evaluation object's argument checks (no GPU:
GANLAB_HOST_LOGIC_ONLY=1 where a constructor would touch the device)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import swd_reference as ref  # noqa: E402


# ---- the reference on its own ------------------------------------------------------------------------------------------
def _positions(rng, n_img, n, sizes):
    return [rng.integers(3, s - 3, size=(n_img, n, 2)) for s in sizes]


def test_reference_identical_sets_give_exactly_zero():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 3, 32, 32))
    out = ref.swd(x, x.copy(), _positions(rng, 6, 16, (32, 16)), ref.directions(rng, 2, 8))
    assert out['levels'] == [32, 16] and out['swd'] == [0.0, 0.0] and out['mean'] == 0.0


def test_reference_shift_in_one_dimension_is_the_shift():
    """Two point sets on a line, one shifted by delta: every sorted pair differs by delta."""
    rng = np.random.default_rng(1)
    delta = 0.375
    a = np.zeros((500, 147))
    a[:, 0] = rng.standard_normal(500)
    b = a.copy()
    b[:, 0] += delta
    e0 = np.zeros((1, 1, 147))
    e0[0, 0, 0] = 1.0
    assert abs(ref.sliced_distance(a, b, e0) - delta) < 1e-12


def test_reference_pyramid_reconstructs():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 3, 64, 64))
    pyr = ref.laplacian_pyramid(x)
    assert [p.shape[-1] for p in pyr] == [64, 32, 16]
    assert np.abs(ref.reconstruct(pyr) - x).max() < 1e-12


def test_reference_mirror_rule_keeps_constants():
    """A constant plane stays that constant up to and including the borders under ``down``, and under ``up`` (whose two
    parities both sum to one): the boundary mirrors without repeating the edge sample and loses no weight."""
    c = np.full((1, 1, 16, 16), 0.75)
    assert np.array_equal(ref.down(c), np.full((1, 1, 8, 8), 0.75))
    assert np.array_equal(ref.up(c), np.full((1, 1, 32, 32), 0.75))
    # reflect, not edge-repeat: an impulse at column 1 reaches output column 0 twice (directly and mirrored)
    x = np.zeros((1, 1, 16, 16))
    x[0, 0, 0, 1] = 1.0
    f = ref.F
    assert abs(ref.down(x)[0, 0, 0, 0] - f[2] * (f[1] + f[3])) < 1e-15


def test_reference_descriptor_order_is_channel_dy_dx():
    lv = np.arange(2 * 3 * 16 * 16, dtype=np.float64).reshape(2, 3, 16, 16)
    pos = np.array([[[3, 3], [12, 5]], [[7, 12], [3, 12]]])
    d = ref.descriptors(lv, pos)
    assert d.shape == (4, 147)
    assert d[1, 0] == lv[0, 0, 9, 2] and d[1, 146] == lv[0, 2, 15, 8] and d[2, 49 + 7 + 1] == lv[1, 1, 5, 10]
    mean, std = ref.channel_stats(d)
    nd = ref.normalise(d).reshape(-1, 3, 49)
    assert np.abs(nd.mean(axis=(0, 2))).max() < 1e-12 and np.abs(nd.std(axis=(0, 2)) - 1).max() < 1e-12


def test_reference_zero_variance_channel_is_nan():
    rng = np.random.default_rng(3)
    d = rng.standard_normal((40, 147))
    d[:, 49:98] = 0.25
    assert np.isnan(ref.normalise(d)[:, 49:98]).all() and np.isfinite(ref.normalise(d)[:, :49]).all()
    assert np.isnan(ref.sliced_distance(ref.normalise(d), ref.normalise(d), ref.directions(rng, 1, 4)))


# ---- config ------------------------------------------------------------------------------------------------------------
FIELDS = ('swd_nhoods', 'swd_dir_repeats', 'swd_dirs_per_repeat', 'swd_seed')


@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_defaults_and_overrides(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    c = make_config(model, **kw)
    assert tuple(getattr(c, f) for f in FIELDS) == (128, 4, 128, 0)
    c = make_config(model, swd_nhoods=32, swd_dir_repeats=2, swd_dirs_per_repeat=64, swd_seed=7, **kw)
    assert tuple(getattr(c, f) for f in FIELDS) == (32, 2, 64, 7)


def test_config_cli_flags(monkeypatch, tmp_path):
    from gan_lab_amd import config
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['stylegan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(args)
    assert tuple(getattr(c, f) for f in FIELDS) == (128, 4, 128, 0)
    c = config.main(args + ['--swd_nhoods=64', '--swd_dir_repeats', '2', '--swd_dirs_per_repeat=32', '--swd_seed=5'])
    assert tuple(getattr(c, f) for f in FIELDS) == (64, 2, 32, 5)


def _resnet_cfg(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4, **kw)


@pytest.mark.parametrize('field,bad', [('swd_nhoods', 0), ('swd_nhoods', -3), ('swd_nhoods', 1.5), ('swd_dir_repeats', 0),
                                       ('swd_dir_repeats', '4'), ('swd_dirs_per_repeat', 0), ('swd_dirs_per_repeat', None),
                                       ('swd_seed', -1), ('swd_seed', 0.5), ('swd_seed', 2 ** 63)])
def test_learner_validates_the_options_and_names_the_field(monkeypatch, field, bad):
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    with pytest.raises(ValueError, match=field):
        GANLearner(_resnet_cfg(**{field: bad}))


def test_learner_refuses_swd_among_the_critic_metrics(monkeypatch):
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    with pytest.raises(ValueError, match='disc_metrics'):
        GANLearner(_resnet_cfg(disc_metrics=['discriminator loss', 'SWD']))
    GANLearner(_resnet_cfg(gen_metrics=['generator loss', 'swd']))       # legal among the generator's
    GANLearner(_resnet_cfg())


class _Loader(object):
    def __init__(self, batches):
        self.batches = batches
        self.dataset = list(range(sum(len(b[0]) for b in batches)))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _progan_host_learner(monkeypatch):
    from gan_lab_amd import progressive as P
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    return ProGANLearner(make_config('progan', dev='cpu', pin_memory=False, res_samples=16, res_dataset=16, init_res=4,
                                     batch_size=4, len_latent=16, gen_metrics=['generator loss', 'swd']))


def test_compute_metrics_refuses_swd_without_reals_or_for_the_critic(monkeypatch):
    """Both checks come before any forward, so they run without a GPU."""
    L = _progan_host_learner(monkeypatch)
    z_dl = _Loader([(torch.zeros(4, 16),)])
    x_dl = _Loader([(torch.zeros(4, 3, 4, 4), torch.zeros(4))])
    with pytest.raises(ValueError, match='valid_dl'):
        L.compute_metrics(['generator loss', 'swd'], 'Generator', z_dl)
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['fake realness', 'swd'], 'Discriminator', z_dl, x_dl)


# ---- the evaluation object ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [8, 24, 0, -16, 16.0, 48])
def test_bad_resolutions_raise_before_any_allocation(res, monkeypatch):
    """No GANLAB_HOST_LOGIC_ONLY here: the ValueError must come before the device is looked at, let alone allocated on."""
    from gan_lab_amd import swd
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(ValueError, match='power of two'):
        swd.SlicedWasserstein(res, 64, device='cuda')


def test_bad_options_raise_before_any_allocation():
    from gan_lab_amd import swd
    for kw, name in ((dict(n_images=0), 'n_images'), (dict(nhoods_per_image=0), 'nhoods_per_image'),
                     (dict(dir_repeats=0), 'dir_repeats'), (dict(dirs_per_repeat=-1), 'dirs_per_repeat'),
                     (dict(seed=-1), 'seed')):
        args = dict(n_images=8)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            swd.SlicedWasserstein(32, device='cuda', **args)
    with pytest.raises(ValueError, match='2\\^32'):
        swd.SlicedWasserstein(32, 2 ** 20, nhoods_per_image=128, dirs_per_repeat=128, device='cuda')


def test_a_cpu_device_is_a_type_error_without_the_host_logic_switch(monkeypatch):
    from gan_lab_amd import swd
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(TypeError):
        swd.SlicedWasserstein(32, 8, device='cpu')


def test_unequal_or_short_feeds_raise(monkeypatch):
    from gan_lab_amd import swd
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    sw = swd.SlicedWasserstein(32, 8, nhoods_per_image=4, dir_repeats=1, dirs_per_repeat=16, device='cpu')
    assert sw.levels == [32, 16]
    x = torch.zeros(3, 3, 32, 32)
    sw.feed_real(x)
    sw.feed_real(x)
    sw.feed_fake(x)
    with pytest.raises(ValueError, match='same number'):
        sw.result()
    sw.feed_fake(x)
    with pytest.raises(ValueError, match='8 images per set were declared, 6 were fed'):
        sw.result()
    with pytest.raises(ValueError, match='declared with 8'):
        sw.feed_real(x)                              # 9 > 8
    for bad in (torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 32, 32), torch.zeros(2, 3, 32, 32, dtype=torch.float64),
                np.zeros((2, 3, 32, 32), dtype=np.float32)):
        with pytest.raises(ValueError, match='feed must be'):
            sw.feed_fake(bad)
    sw.reset()
    sw.feed_real(x)
    with pytest.raises(ValueError, match='same number'):
        sw.result()


def test_levels_and_substreams():
    from gan_lab_amd import swd
    assert swd.levels_of(16) == [16] and swd.levels_of(1024) == [1024, 512, 256, 128, 64, 32, 16]
    keys = {swd._substream(s, k) for s in range(4) for k in range(8)}
    assert len(keys) == 32 and all(0 <= k < 2 ** 64 for k in keys)
    assert swd.wanted(['generator loss', 'SWD']) and not swd.wanted(['generator loss']) and not swd.wanted(None)


def test_ops_refuse_cpu_tensors():
    from gan_lab_amd import ops, rng
    x = torch.zeros(1, 3, 32, 32)
    for call in (lambda: ops.swd_down(x), lambda: ops.swd_band(x, torch.zeros(1, 3, 16, 16)),
                 lambda: ops.swd_sort(torch.zeros(4, 8)), lambda: ops.swd_distance(torch.zeros(4, 8), torch.zeros(4, 8)),
                 lambda: ops.swd_stats(torch.zeros(2, 6, dtype=torch.float64), 49),
                 lambda: ops.swd_project(torch.zeros(8, 147), torch.zeros(16, 147), torch.zeros(6, dtype=torch.float64)),
                 lambda: rng.swd_positions(2, 4, 16, device='cpu', seed=1, offset=0),
                 lambda: rng.swd_directions(4, device='cpu', seed=1, offset=0)):
        with pytest.raises(TypeError):
            call()
