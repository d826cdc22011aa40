"""CPU tests of the self-attention option: the config field and its validation, the exported kernels and their geometry
query, the networks' ``state_dict`` keys with and without the block, and the float64 reference's own gradients."""
import pytest
import torch

import attn_reference as ref

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)


def test_config_accepts_the_field():
    from gan_lab_amd import attention
    from gan_lab_amd.config import make_config
    assert make_config('resnetgan', **COMMON).self_attention is None
    assert attention.validate_config(make_config('resnetgan', **COMMON)) == (False, False)
    cfg = make_config('resnetgan', self_attention='gd', gradient_penalty=None, **COMMON)
    assert cfg.self_attention == 'gd' and attention.validate_config(cfg) == (True, True)
    assert attention.validate_config(make_config('resnetgan', self_attention='g', **COMMON)) == (True, False)
    for model in ('progan', 'stylegan'):                     # the row exists for every model; None is fine everywhere
        assert make_config(model, dev='cpu', pin_memory=False).self_attention is None


def test_cli_flag():
    from gan_lab_amd.config import _spec
    row = {name: typ for name, typ, _ in _spec('ResNet GAN')}['self_attention']
    assert row('GD') == 'gd' and row('none') is None and row('None') is None


def test_bad_values_are_rejected():
    from gan_lab_amd import attention
    from gan_lab_amd.config import make_config
    for bad in ('dg', 'both', True, 1, ''):
        with pytest.raises(ValueError, match='self_attention'):
            attention.validate_config(make_config('resnetgan', self_attention=bad, gradient_penalty=None, **COMMON))
    for model in ('progan', 'stylegan'):
        with pytest.raises(ValueError, match='ResNet GAN'):
            attention.validate_config(make_config(model, self_attention='g', dev='cpu', pin_memory=False))
    for sa in ('d', 'gd'):
        with pytest.raises(ValueError, match='gradient_penalty=None'):
            attention.validate_config(make_config('resnetgan', self_attention=sa, **COMMON))      # default: wgan-gp
    with pytest.raises(ValueError, match='reference_format'):
        attention.check_save_format('g', True)
    attention.check_save_format('g', False)
    attention.check_save_format(None, True)


def test_learner_refuses_critic_attention_with_a_penalty(monkeypatch):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    with pytest.raises(ValueError, match='hinge'):
        GANLearner(make_config('resnetgan', batch_size=4, self_attention='d', **COMMON))


def test_progressive_learners_refuse_the_option(monkeypatch):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    with pytest.raises(ValueError, match='ResNet GAN'):
        ProGANLearner(make_config('progan', dev='cpu', pin_memory=False, self_attention='g'))


def test_library_exports_the_kernels():
    from gan_lab_amd import _lib
    L = _lib.lib()
    for name in ('ganlab_attn_supported', 'ganlab_attn_fwd_f32', 'ganlab_attn_bwd_f32', 'ganlab_attn_bwd_workspace',
                 'ganlab_maxpool2x2_f32', 'ganlab_maxpool2x2_bwd_f32', 'ganlab_maxpool2x2_bits_bytes',
                 'ganlab_gated_residual_f32', 'ganlab_dot_f32'):
        assert name in _lib.SIGNATURES and hasattr(L, name), name


def test_supported_agrees_with_the_table():
    from gan_lab_amd import _lib
    L = _lib.lib()
    for dk in list(range(0, 72)) + [128]:
        for dv in list(range(0, 280, 8)) + [17, 250, 512]:
            want = dk % 4 == 0 and 4 <= dk <= 64 and dv % 16 == 0 and 16 <= dv <= 256
            assert bool(L.ganlab_attn_supported(2, dk, dv, 37, 5)) == want, (dk, dv)
    assert L.ganlab_attn_supported(1, 4, 16, 1, 1) == 1
    for n, l, s in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.ganlab_attn_supported(n, 4, 16, l, s) == 0
    # the launcher agrees without touching memory: an unsupported geometry is refused before any launch
    assert L.ganlab_attn_fwd_f32(1, 1, 1, 1, 1, 1, 6, 16, 1, 1, None) == -4
    assert L.ganlab_maxpool2x2_f32(1, 1, 1, 1, 3, 4, None) == -1          # odd H: GANLAB_EINVAL


def test_critic_keys_with_attention_and_spectral_norm():
    from gan_lab_amd.resnetgan.architectures import Discriminator64PixResnet
    plain = list(Discriminator64PixResnet(fmap=16).state_dict().keys())
    sn = list(Discriminator64PixResnet(fmap=16, spectral_norm=True).state_dict().keys())
    d = Discriminator64PixResnet(fmap=16, self_attention=True, spectral_norm=True)
    keys = list(d.state_dict().keys())
    for conv in ('theta', 'phi', 'g', 'o'):
        for leaf in ('weight', 'weight_u', 'weight_v'):
            assert f'self_attn.{conv}.conv2d.{leaf}' in keys
        assert f'self_attn.{conv}.conv2d.bias' not in keys
    assert 'self_attn.gamma' in keys and 'self_attn.gamma_u' not in keys
    assert float(d.self_attn.gamma.detach()) == 0.0
    assert [k for k in keys if not k.startswith('self_attn.')] == sn              # the rest: unchanged and in order
    assert [k for k in keys if k in set(plain)] == plain
    assert d.self_attn.ni == 32 and tuple(d.self_attn.theta.conv2d.weight.shape) == (4, 32, 1, 1)
    assert tuple(d.self_attn.g.conv2d.weight.shape) == (16, 32, 1, 1)
    assert 'self_attn' not in dict(d.resblocks.named_children())                     # beside the Sequential, not in it


@pytest.mark.parametrize('name,kw', [('Generator32PixResnet', dict(fmap=32)), ('Generator64PixResnet', dict(fmap=16)),
                                     ('Discriminator32PixResnet', dict(fmap=32)),
                                     ('Discriminator64PixResnet', dict(fmap=16))])
def test_only_self_attn_keys_are_added(name, kw):
    from gan_lab_amd.resnetgan import architectures as A
    off = getattr(A, name)(**kw)
    on = getattr(A, name)(self_attention=True, **kw)
    k_off, k_on = list(off.state_dict().keys()), list(on.state_dict().keys())
    assert off.self_attn is None and not any('self_attn' in k for k in k_off)
    assert [k for k in k_on if not k.startswith('self_attn.')] == k_off
    assert sorted(k for k in k_on if k.startswith('self_attn.')) == sorted(
        ['self_attn.gamma'] + [f'self_attn.{c}.conv2d.weight' for c in ('theta', 'phi', 'g', 'o')])
    assert on.self_attn.ni == 32


def test_block_rejects_widths_outside_the_kernel_range():
    from gan_lab_amd.attention import SelfAttention2d
    for ni in (48, 16, 0, 544, 1024):
        with pytest.raises(ValueError, match='ni'):
            SelfAttention2d(ni)
    SelfAttention2d(32)
    SelfAttention2d(512)


def test_reference_gradients():
    """The yardstick's own gradients (float64 gradcheck at (N, Dk, Dv, L, S) = (1, 4, 16, 5, 3)), and its lse."""
    g = torch.Generator().manual_seed(0)
    q = torch.randn(1, 4, 5, dtype=torch.float64, generator=g, requires_grad=True)
    k = torch.randn(1, 4, 3, dtype=torch.float64, generator=g, requires_grad=True)
    v = torch.randn(1, 16, 3, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b, c: ref.attention(a, b, c)[0], (q, k, v))
    o, lse = ref.attention(q, k, v)
    s = torch.einsum('ndl,nds->nls', q, k)
    assert torch.allclose(lse, s.exp().sum(2).log(), rtol=1e-12, atol=0)
    assert torch.allclose(o, torch.einsum('ncs,nls->ncl', v, torch.softmax(s, 2)), rtol=1e-12, atol=1e-14)
    x = torch.randn(1, 8, 4, 4, dtype=torch.float64, generator=g, requires_grad=True)
    ws = [torch.randn(*shape, dtype=torch.float64, generator=g, requires_grad=True)
          for shape in ((1, 8, 1, 1), (1, 8, 1, 1), (4, 8, 1, 1), (8, 4, 1, 1))]
    gamma = torch.tensor([0.7], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(ref.block, (x, *ws, gamma))
