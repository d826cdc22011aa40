"""Host-side tests of BigGAN's generator conditioning (gan_lab_amd/hier_latent.py): config validation, the chunk layout, module
trees and state_dict keys with the options on and - unchanged - off, checkpoint config keys, ortho_reg's layer collection, and the
torch reference (tests/hier_reference.py) itself: gradcheck in float64 and its reduction to nn.BatchNorm2d for equal rows."""
import pytest
import torch

import hier_reference as ref
from util import load_golden, rel_err, sub

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)


def _config(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', **{**COMMON, **kw})


def test_config_fields_and_validation():
    from gan_lab_amd import hier_latent
    from gan_lab_amd.config import _spec
    cfg = _config()
    assert cfg.hier_latent is False and cfg.shared_embed == 0
    assert hier_latent.validate_config(cfg) == (False, 0)
    assert hier_latent.validate_config(_config(hier_latent=True)) == (True, 0)                    # self-modulation: no labels
    assert hier_latent.validate_config(_config(hier_latent=True, shared_embed=8, cgan='projection', num_classes=3)) == (True, 8)
    assert hier_latent.validate_config(_config(shared_embed=128, cgan='projection', num_classes=3)) == (False, 128)
    with pytest.raises(ValueError, match='cgan'):
        hier_latent.validate_config(_config(shared_embed=8))
    with pytest.raises(ValueError, match='cgan'):
        hier_latent.validate_config(_config(hier_latent=True, shared_embed=8))
    with pytest.raises(ValueError, match='shared_embed'):
        hier_latent.validate_config(_config(shared_embed=-1, cgan='projection', num_classes=3))
    cfg = _config()
    for bad in (1, 'yes', None):
        cfg.hier_latent = bad
        with pytest.raises(ValueError, match='hier_latent'):
            hier_latent.validate_config(cfg)
    cfg = _config(cgan='projection', num_classes=3)
    for bad in (True, 8.0, '8'):
        cfg.shared_embed = bad
        with pytest.raises(ValueError, match='shared_embed'):
            hier_latent.validate_config(cfg)
    with pytest.raises(ValueError, match='len_latent'):
        hier_latent.validate_config(_config(hier_latent=True, len_latent=3))                      # 32 pixels: B + 1 = 4
    hier_latent.validate_config(_config(hier_latent=True, len_latent=4))
    with pytest.raises(ValueError, match='len_latent'):
        hier_latent.validate_config(_config(hier_latent=True, len_latent=4, res_samples=64, res_dataset=64))
    with pytest.raises(ValueError, match='reference_format'):
        hier_latent.check_save_format(True, 0, True)
    with pytest.raises(ValueError, match='reference_format'):
        hier_latent.check_save_format(False, 8, True)
    hier_latent.check_save_format(True, 8, False)
    hier_latent.check_save_format(False, 0, True)
    for model in ('ProGAN', 'StyleGAN'):                      # the progressive models do not get the fields
        names = {row[0] for row in _spec(model)}
        assert 'hier_latent' not in names and 'shared_embed' not in names
    rows = {row[0]: row[1:] for row in _spec('ResNet GAN')}
    assert rows['hier_latent'] == (bool, False) and rows['shared_embed'] == (int, 0)


def test_progressive_learners_refuse_the_options(monkeypatch):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    for kw in (dict(hier_latent=True), dict(shared_embed=8, cgan='projection', num_classes=3)):
        cfg = make_config('progan', dev='cpu', pin_memory=False, res_samples=8, res_dataset=8)
        for k, v in kw.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError, match='ResNet GAN'):
            ProGANLearner(cfg)


@pytest.mark.parametrize('len_latent,blocks,first,chunk', [(128, 4, 28, 25), (128, 3, 32, 32), (120, 4, 24, 24),
                                                          (120, 3, 30, 30), (5, 4, 1, 1), (4, 3, 1, 1)])
def test_chunk_layout(len_latent, blocks, first, chunk):
    from gan_lab_amd import hier_latent
    got = hier_latent.chunk_layout(len_latent, blocks)
    assert got == (first, [(first + b * chunk, chunk) for b in range(blocks)]) == ref.chunk_layout(len_latent, blocks)
    assert got[1][-1][0] + got[1][-1][1] == len_latent                      # the chunks tile the latent exactly
    with pytest.raises(ValueError, match='len_latent'):
        hier_latent.chunk_layout(blocks, blocks)
    assert hier_latent.num_blocks(32) == 3 and hier_latent.num_blocks(64) == 4


def _gen(res, **kw):
    from gan_lab_amd.resnetgan import architectures as A
    cls = A.Generator64PixResnet if res == 64 else A.Generator32PixResnet
    return cls(fmap=8, **kw)


@pytest.mark.parametrize('res,blocks', [(32, 3), (64, 4)])
def test_state_dict_keys_with_each_option_on(res, blocks):
    from gan_lab_amd.utils.custom_layers import BatchNorm2d, ConditionalBatchNorm2d, ModulatedBatchNorm2d, NormalizeLayer
    off = _gen(res, len_latent=20)
    keys_off = list(off.state_dict().keys())
    norm_keys = [k for k in keys_off if '.norm.' in k and not k.startswith(f'generator_model.{3 + blocks}.')]
    for kw, d_extra in ((dict(hier_latent=True), 0), (dict(shared_embed=6, cgan=True, num_classes=5), 6),
                        (dict(hier_latent=True, shared_embed=6, cgan=True, num_classes=5), 6)):
        g = _gen(res, len_latent=20, **kw)
        sd = g.state_dict()
        first, chunks = ref.chunk_layout(20, blocks) if kw.get('hier_latent') else (20, [(0, 0)] * blocks)
        assert sd['generator_model.1.linear.weight'].shape[1] == first
        # every block norm: buffers as before, gain / shift linears instead of weight / bias; everything else as before
        want = []
        for k in keys_off:
            if k in norm_keys and k.endswith(('norm.weight', 'norm.bias')):
                continue
            want.append(k)
            if k in norm_keys and k.endswith('num_batches_tracked'):
                want += [k.replace('num_batches_tracked', 'gain.linear.weight'),
                         k.replace('num_batches_tracked', 'shift.linear.weight')]
        if 'shared_embed' in kw:
            want.append('shared.weight')
        assert sorted(sd.keys()) == sorted(want)
        if 'shared_embed' in kw:
            assert sd['shared.weight'].shape == (5, 6)
        mods = [m for m in g.modules() if isinstance(m, ModulatedBatchNorm2d)]
        assert len(mods) == 2 * blocks and not any(isinstance(m, ConditionalBatchNorm2d) for m in g.modules())
        assert not any(v.dim() == 2 and v.shape[0] == 5 and 'norm' in k for k, v in sd.items())      # no (K, C) table is left
        for i, m in enumerate(mods):
            d = chunks[i // 2][1] + d_extra
            assert m.gain.linear.weight.shape == m.shift.linear.weight.shape == (m.num_features, d)
            assert m.gain.linear.bias is None and m.shift.linear.bias is None
        assert [(zo, zl) for _, zo, zl in g.hier.norms] == [c for c in chunks for _ in range(2)]
        last = [m for m in g.modules() if isinstance(m, NormalizeLayer)][-1].norm
        assert type(last) is BatchNorm2d                                       # BigGAN's output layer
        with pytest.raises(ValueError, match='no modulation'):
            mods[0](torch.zeros(2, mods[0].num_features, 4, 4))
    eq = _gen(res, len_latent=20, hier_latent=True, equalized_lr=True)
    m = [m for m in eq.modules() if isinstance(m, ModulatedBatchNorm2d)][0]
    assert m.gain.scale != 1.0 and m.gain.scale == m.gain.wscale           # use_equalized_lr reaches the modulation linears
    with pytest.raises(ValueError, match='cgan'):
        _gen(res, len_latent=20, shared_embed=6)
    with pytest.raises(ValueError, match='len_latent'):
        _gen(res, len_latent=blocks, hier_latent=True)
    assert _gen(res, len_latent=blocks + 1, hier_latent=True).generator_model[1].linear.weight.shape[1] == 1


def _learner(monkeypatch, **kw):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    kw = {**COMMON, **kw}
    cfg = make_config('resnetgan', batch_size=4, len_latent=kw.pop('len_latent', 32), log_every=0, **kw)
    cfg.fmap_g, cfg.fmap_d = 32, 32
    return GANLearner(cfg)


def test_learner_refuses_bad_settings(monkeypatch):
    with pytest.raises(ValueError, match='cgan'):
        _learner(monkeypatch, shared_embed=8)
    with pytest.raises(ValueError, match='shared_embed'):
        _learner(monkeypatch, shared_embed=-8, cgan='projection', num_classes=3)
    with pytest.raises(ValueError, match='len_latent'):
        _learner(monkeypatch, hier_latent=True, len_latent=3)


def _saved_config_keys(L, tmp_path, monkeypatch):
    from gan_lab_amd import checkpoint
    L.not_trained_yet = False
    path = tmp_path / 'm.tar'
    L.save_model(path)
    return checkpoint.load_checkpoint(path, 'cpu')


@pytest.mark.parametrize('res', [32, 64])
def test_layout_and_checkpoint_are_unchanged_with_the_options_off(monkeypatch, tmp_path, res):
    """Both off: the generator has the keys, shapes and module tree of one built without the keywords - the reference's own
    (tests/golden/resnet{32,64}.npz) - and a checkpoint carries neither field."""
    from gan_lab_amd.resnetgan import architectures as A
    from gan_lab_amd.utils.custom_layers import ModulatedBatchNorm2d
    G = load_golden(f'resnet{res}.npz')
    L = _learner(monkeypatch, res_samples=res, res_dataset=res, len_latent=int(G['len_latent']))
    gen_cls = A.Generator64PixResnet if res == 64 else A.Generator32PixResnet
    plain = gen_cls(len_latent=L.config.len_latent, fmap=32)
    sd, sd0 = L.gen_model.state_dict(), plain.state_dict()
    assert list(sd.keys()) == list(sd0.keys()) == list(sub(G, 'g0.').keys())
    assert [type(m).__name__ for m in L.gen_model.modules()] == [type(m).__name__ for m in plain.modules()]
    assert L.gen_model.hier is None and not any(isinstance(m, ModulatedBatchNorm2d) for m in L.gen_model.modules())
    ck = _saved_config_keys(L, tmp_path, monkeypatch)
    assert 'hier_latent' not in ck['config'] and 'shared_embed' not in ck['config']
    assert set(vars(L.config)) - set(ck['config']) >= {'hier_latent', 'shared_embed'}
    assert list(ck['gen_model_state_dict'].keys()) == list(sd0.keys())
    # ... and with them on it carries both, and the reference format is refused
    L2 = _learner(monkeypatch, res_samples=res, res_dataset=res, hier_latent=True, shared_embed=8, cgan='projection',
                  num_classes=3)
    ck2 = _saved_config_keys(L2, tmp_path, monkeypatch)
    assert ck2['config']['hier_latent'] is True and ck2['config']['shared_embed'] == 8
    assert set(ck2['config']) - set(ck['config']) == {'hier_latent', 'shared_embed', 'cgan'}
    assert 'shared.weight' in ck2['gen_model_state_dict']
    with pytest.raises(ValueError, match='reference_format'):
        L2.save_model(tmp_path / 'r.tar', reference_format=True)
    assert getattr(L2.gen_model.shared.weight, '_ganlab_arena', None) is L2.arena_g


def test_ortho_reg_collects_gain_and_shift_and_not_shared():
    from gan_lab_amd.ortho_reg import regularised_layers
    g = _gen(32, len_latent=20, hier_latent=True, shared_embed=6, cgan=True, num_classes=5)
    prefixes = [p for p, _, _ in regularised_layers(g)]
    assert sum(p.endswith('norm.gain.linear') for p in prefixes) == 6
    assert sum(p.endswith('norm.shift.linear') for p in prefixes) == 6
    assert not any('shared' in p for p in prefixes)
    plain = [p for p, _, _ in regularised_layers(_gen(32, len_latent=20))]
    assert [p for p in prefixes if '.norm.' not in p] == plain


def test_reference_passes_gradcheck():
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    z, shared, labels = rnd(3, 5).requires_grad_(True), rnd(4, 2).requires_grad_(True), torch.tensor([3, 0, 3])
    W1, W2 = rnd(3, 4).requires_grad_(True), rnd(3, 4).requires_grad_(True)
    x = rnd(3, 3, 2, 2).requires_grad_(True)

    def f(z, shared, W1, W2, x):
        mod = ref.modulation(z, [(W1, 1, 2, 0.7, 1.0), (W2, 1, 2, 0.7, 0.0)], shared, labels)
        return ref.mod_batch_norm(x, mod[:, :3], mod[:, 3:])

    assert torch.autograd.gradcheck(f, (z, shared, W1, W2, x), eps=1e-6, atol=1e-5)
    rm, rv = rnd(3), rnd(3).abs() + 0.5
    assert torch.autograd.gradcheck(lambda x, a, b: ref.mod_batch_norm_eval(x, a, b, rm, rv), (x, rnd(3, 3).requires_grad_(True),
                                    rnd(3, 3).requires_grad_(True)), eps=1e-6, atol=1e-5)
    # the gradient towards z is zero outside the chunk, the gradient of an absent class is exactly zero
    out = f(z, shared, W1, W2, x)
    dz, ds = torch.autograd.grad(out.square().sum(), (z, shared))
    assert bool((dz[:, 0] == 0).all()) and bool((dz[:, 3:] == 0).all()) and bool((dz[:, 1:3] != 0).all())
    assert bool((ds[1] == 0).all()) and bool((ds[2] == 0).all()) and bool((ds[0] != 0).all())


@pytest.mark.parametrize('training', [True, False])
def test_equal_rows_reduce_the_reference_to_batchnorm(training):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(5).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(5, generator=g))
        bn.bias.copy_(torch.randn(5, generator=g))
        bn.running_mean.copy_(torch.randn(5, generator=g))
        bn.running_var.copy_(torch.rand(5, generator=g) + 0.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(training)
    want = bn(x)
    gain, shift = bn.weight.detach().expand(4, 5), bn.bias.detach().expand(4, 5)
    got = ref.mod_batch_norm(x, gain, shift, bn.eps) if training else ref.mod_batch_norm_eval(x, gain, shift, rm, rv, bn.eps)
    assert rel_err(got, want.detach()) <= 1e-12
