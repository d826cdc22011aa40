"""Host-side tests of the power-spectrum regulariser (gan_lab_amd/spectrum_reg.py): the float64 reference on its
own (tests/spectrum_reg_reference.py: against the metric's numpy reference, a brute-force DFT, torch.autograd and gradcheck), the
config fields and their CLI flags, every refusal, the checkpoint's saved config and the learner with the option off (no GPU:
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

import spectrum_reference as metric_ref  # noqa: E402
import spectrum_reg_reference as ref  # noqa: E402


# ---- the reference on its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('res', [16, 32, 64])
def test_reference_profile_is_the_metrics(res, window):
    x = ref.smooth_noisy(3, res, seed=res)
    want = metric_ref.profiles(x.numpy(), window)
    got = ref.profiles(x, window).numpy()
    assert got.shape == want.shape == (3, res // 2 + 1)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(ref.bin_index(res).numpy(), metric_ref.bin_index(res))
    assert want.min() > 1e-12                                     # the test images keep every bin far above the 1e-30 floor


@pytest.mark.parametrize('window', ref.WINDOWS)
def test_reference_forward_is_a_brute_force_dft(window):
    x = ref.smooth_noisy(2, 16, seed=5)
    want = ref.dft_matrix_profiles(x, window)
    got = ref.profiles(x, window)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    t = ref.set_profile(ref.smooth_noisy(2, 16, seed=6), window)
    for band in ref.BANDS:
        b = ref.band_bins(16, band)
        d = torch.log(want.mean(dim=0)[b]) - torch.log(t[b])
        assert abs(float(ref.loss(x, t, band, window)) - float((d * d).mean())) <= 1e-12 * float((d * d).mean())
    assert ref.band_bins(16, 'all') == list(range(1, 9)) and ref.band_bins(16, 'hf') == [5, 6, 7, 8]


@pytest.mark.parametrize('band', ref.BANDS)
@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('res,n', [(16, 2), (32, 3)])
def test_reference_backward_is_autograd_through_fft2(res, n, window, band):
    x = ref.smooth_noisy(n, res, seed=1).double().requires_grad_(True)
    t = ref.set_profile(ref.smooth_noisy(n, res, seed=2), window)
    L = ref.loss(x, t, band, window)
    want, = torch.autograd.grad(1.7 * L, x)
    L2, got = ref.loss_and_grad(x, t, band, window, grad_out=1.7)
    assert float(L2) == pytest.approx(float(L.detach()), rel=1e-13) and float(L.detach()) > 1e-4
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10 * float(want.abs().max()))
    assert float((got - want).norm() / want.norm()) < 1e-10


def test_reference_gradcheck():
    x = ref.smooth_noisy(2, 16, seed=3).double().requires_grad_(True)
    for window in ref.WINDOWS:
        t = ref.set_profile(ref.smooth_noisy(2, 16, seed=4), window)
        for band in ref.BANDS:
            assert torch.autograd.gradcheck(lambda v: ref.Loss.apply(v, t, band, window), (x,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_reference_special_cases():
    x = ref.smooth_noisy(2, 16, seed=7)
    s = ref.set_profile(x)
    L, dx = ref.loss_and_grad(x, s, 'all')
    assert float(L) == 0.0 and float(dx.abs().max()) == 0.0      # the set against its own profile
    L, dx = ref.loss_and_grad(torch.zeros(1, 3, 16, 16), s, 'hf')
    assert float(dx.abs().max()) == 0.0 and float(L) > 1000.      # every bin on the floor: no gradient, ln 1e-30 in the loss
    a = ref.ema([s, 2 * s, 4 * s], 0.5)
    assert torch.allclose(a, s * (0.25 + 0.5 + 2.0), rtol=1e-15)
    # the float32 run of the same steps stays near float64: the yardstick of the GPU tests
    t = ref.set_profile(ref.smooth_noisy(2, 16, seed=8))
    L64, d64 = ref.loss_and_grad(x, t, 'hf')
    L32, d32 = ref.loss_and_grad(x, t, 'hf', dtype=torch.float32)
    assert L32.dtype == d32.dtype == torch.float32
    assert abs(float(L32) - float(L64)) < 1e-5 * float(L64) and float((d32.double() - d64).norm() / d64.norm()) < 1e-5


# ---- config ------------------------------------------------------------------------------------------------------------
KW = dict(dev='cpu', pin_memory=False)


@pytest.mark.parametrize('model', ['stylegan', 'progan'])
def test_config_defaults_and_overrides(model):
    from gan_lab_amd import config, spectrum_reg
    c = config.make_config(model, **KW)
    assert (c.spectrum_reg, c.spectrum_reg_band, c.spectrum_reg_decay) == (0.0, 'hf', 0.99)
    assert spectrum_reg.validate_config(c) is None
    c = config.make_config(model, spectrum_reg=0.5, spectrum_reg_band='all', spectrum_reg_decay=0.9, spectrum_window='none', **KW)
    assert spectrum_reg.validate_config(c) == dict(weight=0.5, band='all', decay=0.9, window='none')
    for field in spectrum_reg.FIELDS:
        assert field in config.__doc__
    assert 'nothing was tuned here' in config.__doc__.split('``spectrum_reg`` (ProGAN')[1].split('``--gradient_penalty')[0]


def test_config_cli_round_trip(monkeypatch, tmp_path):
    from gan_lab_amd import config
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['stylegan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(args)
    assert (c.spectrum_reg, c.spectrum_reg_band, c.spectrum_reg_decay) == (0.0, 'hf', 0.99)
    c = config.main(args + ['--spectrum_reg=0.25', '--spectrum_reg_band=ALL', '--spectrum_reg_decay=0.5'])
    assert (c.spectrum_reg, c.spectrum_reg_band, c.spectrum_reg_decay) == (0.25, 'all', 0.5)
    import pickle
    with open(tmp_path / '.config.p', 'rb') as f:
        back = pickle.load(f)
    assert (back.spectrum_reg, back.spectrum_reg_band, back.spectrum_reg_decay) == (0.25, 'all', 0.5)
    with pytest.raises(SystemExit):
        config.main(['resnetgan', '--dev=cpu', '--pin_memory=False', '--spectrum_reg=0.25'])


def test_the_resnet_gan_config_has_no_such_field():
    from gan_lab_amd import config, spectrum_reg
    c = config.make_config('resnetgan', **KW)
    for field in spectrum_reg.FIELDS:
        assert not hasattr(c, field)
        with pytest.raises(AttributeError, match=field):
            config.make_config('resnetgan', **dict(KW, **{field: 0.5}))
    assert spectrum_reg.validate_config(c) is None


def _learner(monkeypatch, kind='stylegan', **kw):
    from gan_lab_amd import progressive as P
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    common = dict(dev='cpu', pin_memory=False, res_samples=16, res_dataset=16, batch_size=4, len_latent=16, mbstd_group_size=-1)
    common.update(kw)
    if kind == 'stylegan':
        return StyleGANLearner(make_config('stylegan', init_res=8, len_dlatent=16, mapping_num_fcs=2, cutoff_trunc_trick=None,
                                           **common))
    return ProGANLearner(make_config('progan', init_res=4, **common))


@pytest.mark.parametrize('kind', ['progan', 'stylegan'])
@pytest.mark.parametrize('field,bad', [
    ('spectrum_reg', -0.5), ('spectrum_reg', float('nan')), ('spectrum_reg', float('inf')), ('spectrum_reg', '1'),
    ('spectrum_reg', True), ('spectrum_reg', None),
    ('spectrum_reg_band', 'lf'), ('spectrum_reg_band', 'HF'), ('spectrum_reg_band', None), ('spectrum_reg_band', 1),
    ('spectrum_reg_decay', 1.0), ('spectrum_reg_decay', -0.1), ('spectrum_reg_decay', float('nan')), ('spectrum_reg_decay', 'x')])
def test_every_refusal_names_its_field(monkeypatch, kind, field, bad):
    """Whether or not the weight is on: a bad band or decay beside weight 0 is refused too."""
    with pytest.raises(ValueError, match=r'config\.' + field + r'\b'):
        _learner(monkeypatch, kind, **{field: bad})
    if field != 'spectrum_reg':
        with pytest.raises(ValueError, match=r'config\.' + field + r'\b'):
            _learner(monkeypatch, kind, spectrum_reg=1.0, **{field: bad})


def test_the_field_on_a_resnet_gan_config_is_refused(monkeypatch):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    cfg = make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4)
    cfg.spectrum_reg = 1.0
    with pytest.raises(ValueError, match=r'config\.spectrum_reg\b'):
        GANLearner(cfg)
    del cfg.spectrum_reg
    cfg.spectrum_reg_band = 'hf'
    with pytest.raises(ValueError, match=r'config\.spectrum_reg\b'):
        GANLearner(cfg)
    del cfg.spectrum_reg_band
    assert GANLearner(cfg).spectrum_reg is None


@pytest.mark.parametrize('kind', ['progan', 'stylegan'])
def test_learner_has_no_regulariser_while_the_option_is_off(monkeypatch, kind):
    L = _learner(monkeypatch, kind)
    assert L.spectrum_reg is None and L._spectrum_reg_fields() == {} and 'spectrum_reg' not in L.last_losses
    L = _learner(monkeypatch, kind, spectrum_reg=0.5, spectrum_reg_band='all', spectrum_window='none')
    r = L.spectrum_reg
    assert (r.weight, r.band, r.decay, r.window, r.target) == (0.5, 'all', 0.99, 'none', None)
    assert L._spectrum_reg_fields() == {'spectrum_reg_target': None}
    assert not r.active(4) and not r.active(8) and r.active(16) and r.active(1024) and not r.active(2048)
    # no target yet: the generator step's term raises and names the way out, before any launch
    with pytest.raises(RuntimeError, match='set_target'):
        r.loss(torch.zeros(4, 3, 16, 16))
    assert r.loss(torch.zeros(4, 3, 8, 8)) is None                # below the transform's smallest size: nothing at all
    r.observe(torch.zeros(4, 3, 8, 8))
    assert r.target is None
    # a growth event drops the target
    r.target = torch.zeros(9, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='set_target'):
        r.loss(torch.zeros(4, 3, 32, 32))                         # nine bins are not a 32 x 32 profile
    r.reset()
    assert r.target is None
    # the checkpoint round trip of the target
    r.restore({'spectrum_reg_target': torch.arange(9, dtype=torch.float64)})
    assert r.state()['spectrum_reg_target'].tolist() == list(range(9))
    r.restore({})
    assert r.target is None


def test_the_step_graph_is_not_eligible_with_the_option_on(monkeypatch):
    from gan_lab_amd import graphs
    monkeypatch.setattr(graphs._StepGraphs, 'eligible', lambda self: True)      # as on one GPU, single process
    off, on = _learner(monkeypatch), _learner(monkeypatch, spectrum_reg=1.0)
    for L in (off, on):
        L.gen_model.fade_in_phase = False
    assert graphs.GraphedStep(off).eligible() and not graphs.GraphedStep(on).eligible()


def test_saved_config_is_unchanged_while_off():
    from gan_lab_amd import checkpoint, spectrum_reg
    from gan_lab_amd.config import make_config
    for model in ('stylegan', 'progan'):
        off = make_config(model, **KW)
        before = {k: v for k, v in vars(off).items() if k not in spectrum_reg.FIELDS}      # the config before the fields existed
        assert spectrum_reg.saved_config_fields(dict(vars(off))) == before
        assert list(spectrum_reg.saved_config_fields(dict(vars(off)))) == list(before)     # the order too: the file's bytes
        assert not [k for k in checkpoint.reference_config_fields(off) if k.startswith('spectrum')]
        on = make_config(model, spectrum_reg=0.5, **KW)
        assert spectrum_reg.saved_config_fields(dict(vars(on))) == dict(vars(on))
        kept = checkpoint.reference_config_fields(on)               # written although the 'spectrum' metric is not requested
        assert {k: kept[k] for k in spectrum_reg.FIELDS} == dict(spectrum_reg=0.5, spectrum_reg_band='hf', spectrum_reg_decay=0.99)
        assert 'spectrum_window' not in kept
        # the 'spectrum' metric requested, the option off: the plain checkpoint's config has none of the three fields; the
        # reference-format file writes every ``spectrum_*`` field of the config as the metric's row
        # (tests/test_validation_host.py::test_reference_format_checkpoint_keeps_a_rows_fields_only_while_its_metric_is_on pins
        # exactly that set), the three at their defaults
        both = make_config(model, gen_metrics=['generator loss', 'spectrum'], **KW)
        assert not [k for k in spectrum_reg.saved_config_fields(dict(vars(both))) if k in spectrum_reg.FIELDS]
        row = {k: v for k, v in checkpoint.reference_config_fields(both).items() if k.startswith('spectrum_')}
        assert row == dict(spectrum_window='hann', spectrum_reg=0.0, spectrum_reg_band='hf', spectrum_reg_decay=0.99)


def test_plain_checkpoint_carries_the_target_only_while_on(monkeypatch):
    def saved(L):
        monkeypatch.setattr(L, 'materialize_lagged_generator', lambda: L.gen_model)
        return L._plain_checkpoint_dict()
    off = saved(_learner(monkeypatch))
    assert not [k for k in off if k.startswith('spectrum')] and not [k for k in off['config'] if k.startswith('spectrum_reg')]
    L = _learner(monkeypatch, spectrum_reg=2.0)
    L.spectrum_reg.target = torch.arange(9, dtype=torch.float64)
    on = saved(L)
    assert on['spectrum_reg_target'].tolist() == list(range(9))
    assert (on['config']['spectrum_reg'], on['config']['spectrum_reg_band'], on['config']['spectrum_reg_decay']) == (2.0, 'hf', 0.99)
    assert set(on) - set(off) == {'spectrum_reg_target'} and set(on['config']) - set(off['config']) == set(
        ('spectrum_reg', 'spectrum_reg_band', 'spectrum_reg_decay'))


def test_ops_refuse_host_tensors_and_bad_arguments():
    from gan_lab_amd import ops
    x, t = torch.zeros(2, 3, 16, 16), torch.zeros(9, dtype=torch.float64)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.spectrum_loss(x, t)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.spectrum_profile_mean(x)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.spectrum_target_update(x, t, 0.5, True)
    with pytest.raises(ValueError, match='band'):
        ops.spectrum_loss(x, t, band='lf')
    with pytest.raises(ValueError, match='window'):
        ops.spectrum_loss(x, t, window='hamming')
    assert ops.SPECTRUM_BANDS == {'all': 0, 'hf': 1}
    L = __import__('gan_lab_amd._lib', fromlist=['lib']).lib()
    assert L.ganlab_spectrum_reg_scratch(0, 16) == 0 and L.ganlab_spectrum_reg_scratch(1, 24) == 0
    assert L.ganlab_spectrum_reg_scratch(2, 16) == 2 * 16 * 4 + 2 * 3 * 16 * 9 * 8
