"""Host-side tests of the MS-SSIM metric (gan_lab_amd/msssim.py): the numpy reference on its own, the config
option and its CLI flag, the learners' and the evaluation object's argument checks (no GPU: GANLAB_HOST_LOGIC_ONLY=1 where a
constructor would touch the device)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import msssim_reference as ref  # noqa: E402


# ---- the reference on its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [16, 32, 64])
def test_reference_identical_images_give_exactly_one(res):
    a, _ = ref.sample_pairs('noise', 3, res, seed=res)
    tab = ref.table(a, a.copy())
    assert np.array_equal(tab, np.ones_like(tab))
    assert np.array_equal(ref.per_pair(a, a.copy()), np.ones(3)) and ref.msssim(a, a.copy())['msssim'] == 1.0


@pytest.mark.parametrize('kind', ['noise', 'smooth', 'near'])
def test_reference_is_symmetric(kind):
    a, b = ref.sample_pairs(kind, 4, 32, seed=1)
    assert np.array_equal(ref.table(a, b), ref.table(b, a))
    assert np.array_equal(ref.per_pair(a, b), ref.per_pair(b, a))


@pytest.mark.parametrize('p,q,data_range', [(0.5, 0.25, 2.0), (1.0, -0.5, 2.0), (0.3, 0.9, 1.0), (0.0, 0.7, 2.0)])
def test_reference_constant_images_closed_form(p, q, data_range):
    """All variances vanish: every CS_i is C2 / C2 = 1 and SSIM_4 is the luminance term, so the product is that term to
    the power w_4.  (p q < 0 makes the term negative only when 2 |p q| > C1; the clamp then gives 0.)"""
    a, b = np.full((2, 3, 32, 32), p), np.full((2, 3, 32, 32), q)
    c1, _ = ref.constants(data_range)
    lum = max((2 * p * q + c1) / (p * p + q * q + c1), 0.)
    got = ref.per_pair(a, b, data_range)
    assert np.abs(got - lum ** 0.1333).max() <= 1e-12
    assert np.abs(ref.table(a, b, data_range)[:, :4, 0] - 1.).max() <= 1e-12


def test_reference_anticorrelated_pair_is_clamped_to_exactly_zero():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((4, 3, 32, 32))
    raw = ref.raw_table(a, -a)
    assert (raw[:, 0, 0] < -0.1).all()                     # CS_0 is negative before the clamp ...
    with np.errstate(invalid='ignore'):
        assert np.isnan(raw[:, 0, 0] ** 0.0448).all()      # ... where the power would be NaN
    assert np.array_equal(ref.per_pair(a, -a), np.zeros(4)) and ref.msssim(a, -a)['msssim'] == 0.0


def test_reference_window_shrinks_below_eleven():
    for side, taps in ((1024, 11), (16, 11), (8, 8), (4, 4), (2, 2), (1, 1)):
        g = ref.window(side)
        assert g.shape == (taps,) and abs(g.sum() - 1.) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() in (taps // 2,
                                                                                                                  (taps - 1) // 2)
    assert ref.window(1).tolist() == [1.0]
    g = ref.window(64)
    assert abs(g[4] / g[5] - np.exp(-1. / (2 * 1.5 ** 2))) < 1e-15          # 11 taps: sigma is the paper's 1.5
    # every level of a 16^2 pair: output sides 6, 1, 1, 1, 1
    a, b = ref.sample_pairs('near', 1, 16, seed=0)
    sides = []
    for lv_a, lv_b in zip(ref.pyramid(a.astype(np.float64)), ref.pyramid(b.astype(np.float64))):
        sides.append(ref.level_maps(lv_a, lv_b)[0].shape[-1])
    assert sides == [6, 1, 1, 1, 1]


def test_reference_pool_is_the_papers_reflect_convolution():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 3, 16, 16))
    want = np.stack([np.stack([ndimage.convolve(pl, np.full((2, 2), 0.25), mode='reflect')[::2, ::2] for pl in img]) for img in x])
    assert np.abs(ref.pool(x) - want).max() < 1e-15


def test_reference_fp32_run_stays_near_float64():
    """The yardstick of the GPU tests: the same steps in fp32 agree with float64 to well below 1e-6 on pairs off the clamp."""
    a, b = ref.sample_pairs('near', 4, 32, seed=3)
    d = np.abs(ref.per_pair(a, b, dtype=np.float32) - ref.per_pair(a, b)).max()
    assert d < 1e-6 and ref.table(a, b)[:, :, 0].min() > 0.99


# ---- config ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_default_and_override(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    assert make_config(model, **kw).msssim_range == 2.0
    assert make_config(model, msssim_range=1.0, **kw).msssim_range == 1.0
    assert 'msssim' not in [m.casefold() for m in make_config(model, **kw).gen_metrics]         # off by default


def test_config_cli_flag(monkeypatch, tmp_path):
    from gan_lab_amd import config
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['stylegan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    assert config.main(args).msssim_range == 2.0
    c = config.main(args + ['--msssim_range=4.5'])
    assert c.msssim_range == 4.5 and isinstance(c.msssim_range, float)


def _resnet_cfg(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4, **kw)


@pytest.mark.parametrize('bad', [0, 0.0, -2.0, float('nan'), float('inf'), '2', None, True])
def test_learner_validates_the_range_and_names_the_field(monkeypatch, bad):
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    with pytest.raises(ValueError, match='msssim_range'):
        GANLearner(_resnet_cfg(msssim_range=bad))


def test_learner_refuses_msssim_among_the_critic_metrics(monkeypatch):
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    with pytest.raises(ValueError, match='disc_metrics'):
        GANLearner(_resnet_cfg(disc_metrics=['discriminator loss', 'MSSSIM']))
    GANLearner(_resnet_cfg(gen_metrics=['generator loss', 'msssim'], msssim_range=1))     # legal among the generator's
    GANLearner(_resnet_cfg())


class _Loader(object):
    def __init__(self, batches):
        self.batches = batches
        self.dataset = list(range(sum(len(b[0]) for b in batches)))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _progan_host_learner(monkeypatch, batch=4):
    from gan_lab_amd import progressive as P
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    return ProGANLearner(make_config('progan', dev='cpu', pin_memory=False, res_samples=16, res_dataset=16, init_res=4,
                                     batch_size=batch, len_latent=16, gen_metrics=['generator loss', 'msssim'],
                                     mbstd_group_size=-1))


def test_compute_metrics_refuses_msssim_for_the_critic_and_an_odd_batch(monkeypatch):
    """Both checks come before any forward, so they run without a GPU."""
    L = _progan_host_learner(monkeypatch)
    z_dl = _Loader([(torch.zeros(4, 16),)])
    x_dl = _Loader([(torch.zeros(4, 3, 4, 4), torch.zeros(4))])
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['fake realness', 'msssim'], 'Discriminator', z_dl, x_dl)
    L = _progan_host_learner(monkeypatch, batch=3)
    with pytest.raises(ValueError, match='batch_size'):
        L.compute_metrics(['msssim'], 'Generator', _Loader([(torch.zeros(3, 16),)]))


def test_reference_format_checkpoint_omits_the_field_while_the_metric_is_off():
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    for model in ('stylegan', 'progan'):
        off = make_config(model, dev='cpu', pin_memory=False)
        assert 'msssim_range' in vars(off)
        assert not [k for k in checkpoint.reference_config_fields(off) if k.startswith('msssim')]
        on = make_config(model, dev='cpu', pin_memory=False, gen_metrics=['generator loss', 'MSSSIM'], msssim_range=1.5)
        kept = checkpoint.reference_config_fields(on)
        assert kept['msssim_range'] == 1.5 and not [k for k in kept if k.startswith('swd_')]


# ---- the evaluation object ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [8, 24, 0, -16, 16.0, 48, True])
def test_bad_resolutions_raise_before_any_allocation(res, monkeypatch):
    """No GANLAB_HOST_LOGIC_ONLY here: the ValueError must come before the device is looked at, let alone allocated on."""
    from gan_lab_amd import msssim
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(ValueError, match='power of two'):
        msssim.MultiScaleSSIM(res, 64, device='cuda')


def test_bad_options_raise_before_any_allocation(monkeypatch):
    from gan_lab_amd import msssim
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    for n in (0, 1, 7, -2, 8.0, True):
        with pytest.raises(ValueError, match='n_images'):
            msssim.MultiScaleSSIM(32, n, device='cuda')
    for r in (0, -1.0, float('nan'), float('inf'), '2'):
        with pytest.raises(ValueError, match='data_range'):
            msssim.MultiScaleSSIM(32, 8, data_range=r, device='cuda')


def test_a_cpu_device_is_a_type_error_without_the_host_logic_switch(monkeypatch):
    from gan_lab_amd import msssim
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(TypeError):
        msssim.MultiScaleSSIM(32, 8, device='cpu')


def test_odd_overfull_and_malformed_feeds_raise(monkeypatch):
    from gan_lab_amd import msssim
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    ms = msssim.MultiScaleSSIM(32, 8, device='cpu')
    assert ms.n_pairs == 4 and (ms.c1, ms.c2) == ((0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2)
    ms.feed(torch.zeros(4, 3, 32, 32))
    with pytest.raises(ValueError, match='even number'):
        ms.feed(torch.zeros(3, 3, 32, 32))
    with pytest.raises(ValueError, match='8 images were declared, 4 were fed'):
        ms.result()
    with pytest.raises(ValueError, match='declared with 8'):
        ms.feed(torch.zeros(6, 3, 32, 32))                         # 10 > 8
    for bad in (torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 32, 32), torch.zeros(2, 3, 32, 32, dtype=torch.float64),
                np.zeros((2, 3, 32, 32), dtype=np.float32)):
        with pytest.raises(ValueError, match='feed must be'):
            ms.feed(bad)
    ms.feed(torch.zeros(4, 3, 32, 32))
    with pytest.raises(RuntimeError, match='GANLAB_HOST_LOGIC_ONLY'):
        ms.result()                                               # complete, but this switch computes nothing
    ms.reset()
    with pytest.raises(ValueError, match='0 were fed'):
        ms.result()


def test_wanted():
    from gan_lab_amd import msssim
    assert msssim.wanted(['generator loss', 'MSSSIM']) and not msssim.wanted(['generator loss', 'swd']) and not msssim.wanted(None)
    assert msssim.WEIGHTS == ref.WEIGHTS and msssim.LEVELS == ref.LEVELS == 5 and msssim.MIN_RES == 16


def test_ops_refuse_cpu_tensors():
    from gan_lab_amd import msssim, ops
    x = torch.zeros(2, 3, 16, 16)
    ws = torch.zeros(64, dtype=torch.float64)
    for call in (lambda: ops.msssim_workspace(2, 16, 'cpu'),
                 lambda: ops.msssim_level(x, x, 0, 16, 4e-4, 3.6e-3, ws, 0, 2),
                 lambda: ops.msssim_finish(ws, 2, 16, torch.zeros(2, 5, 2, dtype=torch.float64),
                                           torch.zeros(2, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)),
                 lambda: msssim.pairs(x, x)):
        with pytest.raises(TypeError):
            call()


def test_workspace_query_is_a_host_call():
    """5 levels of a 64^2 pair: 2, 1, 1, 1, 1 tiles per axis, 3 channels, (cs, ssim) doubles."""
    from gan_lab_amd import _lib
    L = _lib.lib()
    assert L.ganlab_msssim_workspace(7, 64) == 7 * 3 * (4 + 1 + 1 + 1 + 1) * 2 * 8
    assert L.ganlab_msssim_workspace(1, 1024) == 3 * (32 * 32 + 16 * 16 + 8 * 8 + 4 * 4 + 2 * 2) * 2 * 8
    for p, r in ((0, 64), (4, 8), (4, 48), (4, 32768)):
        assert L.ganlab_msssim_workspace(p, r) == 0
