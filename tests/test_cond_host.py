"""CPU tests of class conditioning (gan_lab_amd/conditional.py): the reference restatement against ``nn.BatchNorm2d``, the config
field and its validation, the conditional networks' parameter shapes, the unchanged layout with the option off, and the host-side
label check."""
import pytest
import torch

import cond_reference as ref
from util import load_golden, rel_err, sub

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)


def test_reference_with_equal_rows_is_batchnorm():
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm2d(5).double().train()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.5)
        bn.bias.normal_(0.0, 0.5)
    x = torch.randn(4, 5, 6, 7, dtype=torch.float64)
    labels = torch.tensor([2, 0, 1, 2])
    y = ref.cond_batch_norm(x, bn.weight.detach().expand(3, 5), bn.bias.detach().expand(3, 5), labels, eps=bn.eps)
    assert rel_err(y, bn(x).detach()) <= 1e-12
    bn.eval()
    y = ref.cond_batch_norm_eval(x, bn.weight.detach().expand(3, 5), bn.bias.detach().expand(3, 5), labels, bn.running_mean,
                                 bn.running_var, eps=bn.eps)
    assert rel_err(y, bn(x).detach()) <= 1e-12


def test_reference_projection_pieces_are_each_others_derivatives():
    torch.manual_seed(1)
    f, W = torch.randn(6, 9, dtype=torch.float64), torch.randn(4, 9, dtype=torch.float64)
    base, g = torch.randn(6, dtype=torch.float64), torch.randn(6, dtype=torch.float64)
    labels = torch.tensor([3, 0, 0, 2, 3, 3])             # class 1 absent
    out, gf, gw, gbase = ref.projection_with_grads(f, W, labels, base, g, torch.float64)
    assert rel_err(gf, ref.proj_dfeat(g, W, labels)) <= 1e-12
    assert rel_err(gw, ref.proj_dweight(g, f, labels, 4)) <= 1e-12
    assert torch.equal(gbase, g) and bool((gw[1] == 0).all())
    assert rel_err(out, base + torch.stack([W[l] @ f[n] for n, l in enumerate(labels.tolist())])) <= 1e-12


def test_config_field_default_and_validation():
    from gan_lab_amd import conditional
    from gan_lab_amd.config import make_config
    cfg = make_config('resnetgan', **COMMON)
    assert cfg.cgan is None and conditional.validate_config(cfg) is False
    assert conditional.validate_config(make_config('resnetgan', cgan='projection', num_classes=10, **COMMON)) is True
    with pytest.raises(ValueError, match='projection'):
        conditional.validate_config(make_config('resnetgan', cgan='concat', num_classes=10, **COMMON))
    for k in (0, 1):
        with pytest.raises(ValueError, match='num_classes'):
            conditional.validate_config(make_config('resnetgan', cgan='projection', num_classes=k, **COMMON))
    for model in ('progan', 'stylegan'):
        with pytest.raises(ValueError, match='ResNet GAN'):
            conditional.validate_config(make_config(model, cgan='projection', num_classes=10, dev='cpu', pin_memory=False))
    # orthogonal to the other options; critic attention keeps requiring gradient_penalty=None
    from gan_lab_amd import attention, spectral_norm
    cfg = make_config('resnetgan', cgan='projection', num_classes=10, loss='hinge', gradient_penalty=None, spectral_norm=True,
                      self_attention='gd', diffaugment='color,translation', **COMMON)
    assert conditional.validate_config(cfg) and spectral_norm.validate_config(cfg) and attention.validate_config(cfg) == (True, True)
    with pytest.raises(ValueError, match='hinge'):
        attention.validate_config(make_config('resnetgan', cgan='projection', num_classes=10, self_attention='d', **COMMON))
    with pytest.raises(ValueError, match='reference_format'):
        conditional.check_save_format('projection', True)
    conditional.check_save_format('projection', False)
    conditional.check_save_format(None, True)


def test_command_line_spelling():
    from gan_lab_amd.config import _spec
    rows = {name: (typ, default) for name, typ, default in _spec('ResNet GAN')}
    typ, default = rows['cgan']
    assert default is None and typ('none') is None and typ('Projection') == 'projection'
    assert 'cgan' in {name for name, _, _ in _spec('StyleGAN')}      # the field exists everywhere; the learner refuses it there


def _learner(monkeypatch, **kw):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', batch_size=4, len_latent=32, log_every=0, **COMMON, **kw)
    cfg.fmap_g, cfg.fmap_d = 32, 32
    return GANLearner(cfg)


def test_learner_refuses_bad_settings(monkeypatch):
    with pytest.raises(ValueError, match='projection'):
        _learner(monkeypatch, cgan='acgan', num_classes=3)
    with pytest.raises(ValueError, match='num_classes'):
        _learner(monkeypatch, cgan='projection')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    with pytest.raises(ValueError, match='ResNet GAN'):
        ProGANLearner(make_config('progan', dev='cpu', pin_memory=False, res_samples=8, res_dataset=8, num_classes=3,
                                  cgan='projection'))


def test_reference_conditioning_still_raises(monkeypatch):
    """class_condition / use_auxiliary_classifier are not this option: they keep their NotImplementedError, and it comes first."""
    for kw in (dict(class_condition=True), dict(use_auxiliary_classifier=True)):
        with pytest.raises(NotImplementedError, match='conditional_probe'):
            _learner(monkeypatch, num_classes=3, **kw)
        with pytest.raises(NotImplementedError, match='conditional_probe'):
            _learner(monkeypatch, num_classes=3, cgan='bogus', **kw)


def test_conditional_learner_builds_on_the_host(monkeypatch):
    from gan_lab_amd.utils.custom_layers import BatchNorm2d, ConditionalBatchNorm2d, NormalizeLayer
    L = _learner(monkeypatch, cgan='projection', num_classes=3)
    g, d = L.gen_model, L.disc_model
    norms = [m for m in g.modules() if isinstance(m, NormalizeLayer)]
    assert len(norms) == 7                                  # two per block, three blocks, and the final one
    assert all(isinstance(m.norm, ConditionalBatchNorm2d) for m in norms)
    assert not any(isinstance(m, BatchNorm2d) for m in g.modules())
    sd = g.state_dict()
    for m in norms:
        c = m.norm.num_features
        assert m.norm.weight.shape == (3, c) and m.norm.bias.shape == (3, c)
        assert bool((m.norm.weight == 1).all()) and bool((m.norm.bias == 0).all())
        assert m.norm.running_mean.shape == (c,) and m.norm.running_var.shape == (c,)
        assert m.norm.num_batches_tracked.dtype == torch.int64 and m.norm.labels is None
    assert sd['generator_model.6.norm.weight'].shape == (3, 32)
    assert sd['generator_model.1.linear.weight'].shape[1] == 32          # the latent input keeps its width
    assert d.proj.linear.weight.shape == (3, 32) and d.proj.linear.bias is None
    assert d.state_dict()['proj.linear.weight'].shape == (3, 32)
    assert d.conv1.conv_layer_1[0].conv2d.weight.shape[1] == 3           # the image input keeps its 3 channels
    # the tables and the projection live in the arenas like every other parameter
    assert getattr(d.proj.linear.weight, '_ganlab_arena', None) is L.arena_d
    assert getattr(norms[0].norm.weight, '_ganlab_arena', None) is L.arena_g
    with pytest.raises(TypeError, match='labels'):
        g(torch.zeros(2, 32))
    with pytest.raises(TypeError, match='labels'):
        d(torch.zeros(2, 3, 32, 32))


def test_64_pixel_projection_reads_linear1s_feature():
    from gan_lab_amd.resnetgan import architectures as A
    d = A.Discriminator64PixResnet(fmap=4, cgan=True, num_classes=5)
    assert d.proj.linear.weight.shape == (5, A.RES_FEATURE_SPACE ** 2 * 8 * 4) == (5, d.linear1.linear.weight.shape[1])
    g = A.Generator64PixResnet(fmap=4, len_latent=8, cgan=True, num_classes=5)
    assert len(g._cond_norms) == 9 and g.generator_model[1].linear.weight.shape[1] == 8
    with pytest.raises(ValueError, match='num_classes'):
        A.Generator64PixResnet(fmap=4, len_latent=8, cgan=True)


def test_spectral_norm_picks_up_the_projection():
    from gan_lab_amd.resnetgan import architectures as A
    from gan_lab_amd.spectral_norm import normalised_layers
    d = A.Discriminator32PixResnet(fmap=32, cgan=True, num_classes=3, spectral_norm=True)
    assert 'proj.linear' in [prefix for prefix, _, _ in normalised_layers(d)]
    sd = d.state_dict()
    assert sd['proj.linear.weight_u'].shape == (3,) and sd['proj.linear.weight_v'].shape == (32,)


@pytest.mark.parametrize('res', [32, 64])
def test_layout_is_unchanged_with_the_option_off(monkeypatch, res):
    """cgan=None: the learner's networks have the keys and shapes of networks built without the keyword - which are the
    reference's own (tests/golden/resnet{32,64}.npz) - and no class-conditional module."""
    from gan_lab_amd.resnetgan import architectures as A
    from gan_lab_amd.utils.custom_layers import ConditionalBatchNorm2d
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    G = load_golden(f'resnet{res}.npz')
    cfg = make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=res, res_dataset=res, batch_size=4,
                      len_latent=int(G['len_latent']), log_every=0)
    cfg.fmap_g, cfg.fmap_d = int(G['fmap_g']), int(G['fmap_d'])
    L = GANLearner(cfg)
    assert L.cgan is False and L.disc_model.proj is None and L.gen_model.cgan is False
    gen_cls, disc_cls = (A.Generator64PixResnet, A.Discriminator64PixResnet) if res == 64 else \
        (A.Generator32PixResnet, A.Discriminator32PixResnet)
    plain_g = gen_cls(len_latent=cfg.len_latent, fmap=cfg.fmap_g)
    plain_d = disc_cls(fmap=cfg.fmap_d)
    for net, plain, prefix in ((L.gen_model, plain_g, 'g0.'), (L.disc_model, plain_d, 'd0.')):
        sd, sd0 = net.state_dict(), plain.state_dict()
        assert list(sd.keys()) == list(sd0.keys()) == list(sub(G, prefix).keys())
        assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in sd0.values()]
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in plain.named_parameters()]
        assert [type(m).__name__ for m in net.modules()] == [type(m).__name__ for m in plain.modules()]
        assert not any(isinstance(m, ConditionalBatchNorm2d) for m in net.modules())
    with pytest.raises(ValueError, match='not class-conditional'):
        L._device_labels(torch.zeros(4, dtype=torch.long), 4, draw=False)


def test_out_of_range_host_labels_are_refused_before_any_upload(monkeypatch):
    from gan_lab_amd import conditional
    L = _learner(monkeypatch, cgan='projection', num_classes=3)
    x = torch.zeros(4, 3, 32, 32)
    uploads = []
    monkeypatch.setattr(torch.Tensor, 'to', lambda self, *a, **k: uploads.append(a) or self)
    for bad in (torch.tensor([0, 1, 3, 2]), torch.tensor([0, -1, 1, 2]), torch.tensor([0, 1, 2]),
                torch.tensor([0., 1., 2., 1.]), torch.tensor([[0, 1, 2, 1]])):
        with pytest.raises(ValueError, match='labels'):
            L.d_step(x, labels=bad)
    assert uploads == []                                                  # refused on the host, nothing was moved
    monkeypatch.undo()
    with pytest.raises(ValueError, match='labels'):                       # and a D step cannot do without them
        L.d_step(x)
    good = conditional.check_host_labels(torch.tensor([0, 2, 1, 2]), 3, 4)
    assert good.dtype == torch.int32 and good.tolist() == [0, 2, 1, 2]
    assert conditional.check_host_labels([1, 0], 2).tolist() == [1, 0]


def test_ops_refuse_host_tensors():
    from gan_lab_amd import ops
    x, w = torch.zeros(2, 3, 4, 4), torch.ones(2, 3)
    labels = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.cond_batch_norm(x, w, torch.zeros(2, 3), labels, torch.zeros(3), torch.ones(3), True)
    with pytest.raises(TypeError):
        ops.class_projection(torch.zeros(2, 5), torch.zeros(3, 5), labels, torch.zeros(2))


def test_saved_config_leaves_the_field_out_when_off():
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    off = checkpoint.reference_config_fields(make_config('progan', dev='cpu', pin_memory=False))
    assert 'cgan' not in off and 'self_attention' not in off


def test_documented_command_line_configures_the_recipe(monkeypatch, tmp_path):
    """``python -m gan_lab_amd.config resnetgan --cgan=projection ...`` as the README gives it: 'none' means no penalty."""
    import os
    from gan_lab_amd import attention, conditional, config, spectral_norm
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    cfg = config.main(['resnetgan', '--cgan=projection', '--num_classes=10', '--loss=hinge', '--gradient_penalty=none',
                       '--spectral_norm', '--self_attention=gd', '--dev=cpu', '--pin_memory=false',
                       f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m'])
    assert os.path.exists(tmp_path / '.config.p')
    assert (cfg.cgan, cfg.num_classes, cfg.loss, cfg.gradient_penalty) == ('projection', 10, 'hinge', None)
    assert conditional.validate_config(cfg) and spectral_norm.validate_config(cfg)
    assert attention.validate_config(cfg) == (True, True)
