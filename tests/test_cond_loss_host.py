"""CPU tests of the classifier-based class conditioning (gan_lab_amd/conditional.py; csrc/cond_loss.hip): the reference
restatement (cc_reference.py) against ``F.cross_entropy`` and against its own autograd, the config fields and their validation,
the critics' heads, the unchanged layout in the other modes, and the C ABI's new entry points."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import cc_reference as ref
from util import rel_err

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)
MODES = ('contra', 'reacgan')
ENTRY_POINTS = ('ganlab_class_ce_fwd_f32', 'ganlab_class_ce_bwd_f32', 'ganlab_cl_supported', 'ganlab_cl_fwd_f32',
                'ganlab_cl_bwd_workspace', 'ganlab_cl_bwd_f32')


def _data(n=9, e=6, k=4, seed=0, labels=None):
    g = torch.Generator().manual_seed(seed)
    h, proxy = torch.randn(n, e, generator=g, dtype=torch.float64), torch.randn(k, e, generator=g, dtype=torch.float64)
    labels = torch.tensor(labels) if labels is not None else torch.randint(0, k, (n,), generator=g)
    return h, proxy, labels


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_cross_entropy_is_torchs():
    g = torch.Generator().manual_seed(0)
    z, labels = torch.randn(11, 5, generator=g, dtype=torch.float64) * 3, torch.randint(0, 5, (11,), generator=g)
    assert rel_err(ref.cross_entropy(z, labels), F.cross_entropy(z, labels)) <= 1e-12
    assert rel_err(ref.cross_entropy_rows(z, labels), F.cross_entropy(z, labels, reduction='none')) <= 1e-12


def test_2c_with_distinct_labels_is_a_cross_entropy_over_the_similarities():
    h, proxy, _ = _data(n=5, k=5)
    labels = torch.tensor([3, 0, 4, 1, 2])
    tau = 0.3
    s, S = ref.similarities(h, proxy, labels)
    rows = []
    for i in range(5):
        logits = torch.cat((s[i:i + 1], torch.cat((S[i, :i], S[i, i + 1:])))) / tau
        # with no second row of the class M_i = u_i: l_i = LSE - u_i
        rows.append(F.cross_entropy(logits[None], torch.zeros(1, dtype=torch.long)))
    assert rel_err(ref.contrastive_rows(h, proxy, labels, '2c', tau), torch.stack(rows)) <= 1e-12


def test_d2d_with_the_clamps_pinned_is_a_cross_entropy_over_the_negatives():
    h, proxy, labels = _data(n=8, k=3, labels=[0, 2, 2, 0, 1, 2, 0, 1])
    tau, mp, mn = 0.7, 1.5, -1.5                      # s - m_p < 0 always, S - m_n > 0 always
    s, S = ref.similarities(h, proxy, labels)
    rows = []
    for i in range(8):
        neg = S[i][labels != labels[i]]
        logits = torch.cat(((s[i:i + 1] - mp), neg - mn)) / tau
        rows.append(F.cross_entropy(logits[None], torch.zeros(1, dtype=torch.long)))
    assert rel_err(ref.contrastive_rows(h, proxy, labels, 'd2d', tau, mp, mn), torch.stack(rows)) <= 1e-12


def test_a_row_without_negatives_is_exactly_zero():
    h, proxy, _ = _data(n=6, k=3)
    labels = torch.tensor([1, 1, 1, 1, 1, 1])
    rows = ref.contrastive_rows(h, proxy, labels, 'd2d', 0.5, 0.98, 0.02)
    assert bool((rows == 0).all())
    dh, dp = ref.contrastive_grads(h, proxy, labels, 'd2d', 0.5, 0.98, 0.02)
    assert bool((dh == 0).all()) and bool((dp == 0).all())
    one = ref.contrastive_rows(h[:1], proxy, labels[:1], '2c', 0.5)         # N = 1 is legal
    assert one.shape == (1,) and float(one) == 0


@pytest.mark.parametrize('mode,kw', [('2c', dict(temperature=0.4)), ('d2d', dict(temperature=0.6)),
                                     ('d2d', dict(temperature=0.5, margin_pos=0.1, margin_neg=0.05))])
def test_analytic_gradients_equal_autograd(mode, kw):
    h, proxy, labels = _data(n=12, e=5, k=4, seed=3, labels=[0, 2, 2, 0, 3, 2, 0, 3, 3, 0, 2, 2])       # class 1 absent
    g = 0.7
    _, _, dh, dp = ref.contrastive_with_grads(h, proxy, labels, g, torch.float64, mode=mode, **kw)
    ah, ap = ref.contrastive_grads(h, proxy, labels, mode, g=g, **kw)
    assert rel_err(ah, dh) <= 1e-12 and rel_err(ap, dp) <= 1e-12
    assert bool((ap[1] == 0).all()) and bool((dp[1] == 0).all())
    if 'margin_pos' in kw:      # the case in which both clamps are in both of their states
        s, S = ref.similarities(h, proxy, labels)
        neg = S[labels[:, None] != labels[None, :]]
        assert (s < 0.1).any() and (s > 0.1).any() and (neg < 0.05).any() and (neg > 0.05).any()


def test_analytic_cross_entropy_gradient_equals_autograd():
    g = torch.Generator().manual_seed(5)
    z, labels = torch.randn(7, 3, generator=g, dtype=torch.float64), torch.tensor([0, 2, 2, 0, 2, 0, 0])
    _, _, dz = ref.cross_entropy_with_grads(z, labels, 0.7, torch.float64)
    assert rel_err(ref.cross_entropy_grad(z, labels, 0.7), dz) <= 1e-12


# ---- config -------------------------------------------------------------------------------------------------------------------
def test_config_fields_and_modes():
    from gan_lab_amd import conditional
    from gan_lab_amd.config import _spec, make_config
    cfg = make_config('resnetgan', **COMMON)
    assert (cfg.cond_lambda, cfg.cond_embed, cfg.cond_temperature, cfg.cond_margin_pos, cfg.cond_margin_neg) == \
        (1.0, 512, 1.0, 0.98, 0.02)
    assert 'cond_lambda' not in {name for name, _, _ in _spec('StyleGAN')}
    assert conditional.mode(cfg) is None and conditional.validate_loss_config(cfg) is None
    assert conditional.validate_loss_config(make_config('resnetgan', cgan='projection', num_classes=4, **COMMON)) is None
    for m in MODES:
        cfg = make_config('resnetgan', cgan=m, num_classes=4, **COMMON)
        assert conditional.validate_config(cfg) is True and conditional.mode(cfg) == m
        assert conditional.validate_loss_config(cfg) == dict(weight=1.0, embed=512, temperature=1.0, margin_pos=0.98,
                                                             margin_neg=0.02)
        with pytest.raises(ValueError, match='num_classes'):
            conditional.validate_config(make_config('resnetgan', cgan=m, num_classes=1, **COMMON))
        for model in ('progan', 'stylegan'):
            with pytest.raises(ValueError, match='ResNet GAN'):
                conditional.validate_config(make_config(model, cgan=m, num_classes=4, dev='cpu', pin_memory=False))
        with pytest.raises(ValueError, match='reference_format'):
            conditional.check_save_format(m, True)
    for unknown in ('auxiliary', 'acgan'):      # AC-GAN's pieces exist (below), its config value is still refused
        with pytest.raises(ValueError, match='projection'):
            conditional.validate_config(make_config('resnetgan', cgan=unknown, num_classes=4, **COMMON))
    assert conditional.mode(make_config('resnetgan', cgan='ReACGAN', num_classes=4, **COMMON)) == 'reacgan'


@pytest.mark.parametrize('field,bad', [('cond_lambda', -0.1), ('cond_lambda', math.inf), ('cond_lambda', math.nan),
                                       ('cond_temperature', 0.0), ('cond_temperature', -1.0), ('cond_embed', 0),
                                       ('cond_embed', 1025), ('cond_margin_neg', 0.98), ('cond_margin_neg', 1.2)])
def test_bad_values_raise_and_name_their_field(monkeypatch, field, bad):
    with pytest.raises(ValueError, match=field):
        _learner(monkeypatch, cgan='reacgan', num_classes=3, **{field: bad})
    with pytest.raises(ValueError, match=field):       # checked when the learner is built, in every mode
        _learner(monkeypatch, **{field: bad})


def test_saved_config_leaves_the_fields_out_when_off():
    from gan_lab_amd import conditional
    from gan_lab_amd.config import make_config
    off = conditional.saved_config_fields(vars(make_config('resnetgan', cgan='projection', num_classes=3, **COMMON)))
    assert not any(k.startswith('cond_') for k in off) and off['cgan'] == 'projection'
    on = conditional.saved_config_fields(vars(make_config('resnetgan', cgan='contra', num_classes=3, **COMMON)))
    assert on['cond_embed'] == 512


def test_shared_embedding_accepts_every_mode():
    from gan_lab_amd import hier_latent
    from gan_lab_amd.config import make_config
    for m in ('projection',) + MODES:
        cfg = make_config('resnetgan', cgan=m, num_classes=3, hier_latent=True, shared_embed=8, **COMMON)
        assert hier_latent.validate_config(cfg) == (True, 8)


# ---- networks -----------------------------------------------------------------------------------------------------------------
def _learner(monkeypatch, **kw):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', batch_size=4, len_latent=32, log_every=0, **COMMON, **kw)
    cfg.fmap_g, cfg.fmap_d = 8, 8
    return GANLearner(cfg)


def test_heads_per_mode(monkeypatch):
    from gan_lab_amd.spectral_norm import normalised_layers
    from gan_lab_amd.resnetgan import architectures as A
    d = A.Discriminator32PixResnet(fmap=8, cgan='acgan', num_classes=3)
    assert d.cond_mode == 'acgan' and d.proj is None and not hasattr(d, 'embed')
    assert d.cls.linear.weight.shape == (3, 8) and d.cls.linear.bias.shape == (3,)
    for m in ('contra', 'reacgan'):
        L = _learner(monkeypatch, cgan=m, num_classes=3, cond_embed=24)
        d = L.disc_model
        assert d.cond_mode == m and d.proj is None and not hasattr(d, 'cls')
        assert d.embed.linear.weight.shape == (24, 8) and d.embed.linear.bias.shape == (24,)
        assert d.proxy.linear.weight.shape == (3, 24) and d.proxy.linear.bias is None
        assert not hasattr(d, 'linear_aux')
        # the arena, the state_dict and spectral norm carry them like proj
        assert getattr(d.proxy.linear.weight, '_ganlab_arena', None) is L.arena_d
        assert getattr(d.embed.linear.bias, '_ganlab_arena', None) is L.arena_d
        sn = A.Discriminator32PixResnet(fmap=8, cgan=m, num_classes=3, cond_embed=24, spectral_norm=True)
        names = [prefix for prefix, _, _ in normalised_layers(sn)]
        assert 'embed.linear' in names and 'proxy.linear' in names
        sd = sn.state_dict()
        assert sd['proxy.linear.weight_u'].shape == (3,) and sd['embed.linear.weight_v'].shape == (8,)
        # the generator is the projection mode's
        P = _learner(monkeypatch, cgan='projection', num_classes=3)
        assert list(L.gen_model.state_dict().keys()) == list(P.gen_model.state_dict().keys())
        with pytest.raises(TypeError, match='labels'):
            d(torch.zeros(2, 3, 32, 32))
    # the paired critic pass stays available with the new heads
    x = torch.zeros(4, 3, 32, 32)
    assert L._pair_critic_batches(x, x) is True


def test_64_pixel_heads_read_linear1s_feature():
    from gan_lab_amd.resnetgan import architectures as A
    d = A.Discriminator64PixResnet(fmap=4, cgan='reacgan', num_classes=5, cond_embed=16)
    feat = d.linear1.linear.weight.shape[1]
    assert d.embed.linear.weight.shape == (16, feat) and d.proxy.linear.weight.shape == (5, 16)
    assert A.Discriminator64PixResnet(fmap=4, cgan='acgan', num_classes=5).cls.linear.weight.shape == (5, feat)
    with pytest.raises(ValueError, match='cond_embed'):
        A.Discriminator32PixResnet(fmap=8, cgan='contra', num_classes=5, cond_embed=2048)
    with pytest.raises(ValueError, match='cgan'):
        A.Discriminator32PixResnet(fmap=8, cgan='concat', num_classes=5)


@pytest.mark.parametrize('cgan', [None, 'projection'])
def test_other_modes_keep_their_layout(monkeypatch, cgan):
    from gan_lab_amd.resnetgan import architectures as A
    kw = dict(cgan=cgan, num_classes=3) if cgan else {}
    L = _learner(monkeypatch, **kw)
    plain_kw = dict(cgan=True, num_classes=3) if cgan else {}
    plain_d = A.Discriminator32PixResnet(fmap=8, **plain_kw)
    plain_g = A.Generator32PixResnet(len_latent=32, fmap=8, **plain_kw)
    for net, plain in ((L.disc_model, plain_d), (L.gen_model, plain_g)):
        assert list(net.state_dict().keys()) == list(plain.state_dict().keys())
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in plain.named_parameters()]
        assert [type(m).__name__ for m in net.modules()] == [type(m).__name__ for m in plain.modules()]
    assert L._cond is None and L._cond_on is False
    assert not any(hasattr(L.disc_model, name) for name in ('cls', 'embed', 'proxy'))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_the_abi_declares_binds_and_exports_the_entry_points():
    from gan_lab_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.CSRC), '..', 'include', 'ganlab_hip.h')).read()
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _lib.SIGNATURES, name
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.SO_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(handle, name), name
    L = _lib.lib()
    assert L.ganlab_cl_supported(64, 512, 10) == 1 and L.ganlab_cl_supported(1, 1, 2) == 1
    assert L.ganlab_cl_supported(8193, 512, 10) == 0 and L.ganlab_cl_supported(64, 1025, 10) == 0
    assert L.ganlab_cl_supported(64, 512, 1) == 0 and L.ganlab_cl_supported(0, 512, 10) == 0
    assert L.ganlab_cl_bwd_workspace(64, 512, 10) == (64 * 512 + 64 + 10) * 4
    assert L.ganlab_cl_fwd_f32(None, None, None, None, None, 64, 512, 10, 0, 1.0, 0.98, 0.02, None) == -1


def test_ops_refuse_host_tensors_and_sizes_outside_the_range():
    from gan_lab_amd import ops
    labels = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.class_cross_entropy(torch.zeros(4, 3), labels)
    with pytest.raises(TypeError):
        ops.class_contrastive(torch.zeros(4, 8), torch.zeros(3, 8), labels)
    with pytest.raises(ValueError, match='mode'):
        ops.class_contrastive(torch.zeros(4, 8), torch.zeros(3, 8), labels, mode='ce')
