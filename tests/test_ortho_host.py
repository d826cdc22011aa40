"""CPU tests of the orthogonal regulariser: the float64 reference (tests/ortho_reference.py) against its own autograd and its two
restatements, the config fields and their validation, the layer enumeration, and the host-side layout of the job table."""
import types

import pytest
import torch

import ortho_reference as ref
from util import rel_err

SHAPES = [(2, 3), (5, 7), (3, 576), (64, 27), (33, 130), (128, 64)]


def _w(r, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, k, generator=g, dtype=torch.float64) * (2.0 / k) ** 0.5


@pytest.mark.parametrize('r,k', SHAPES)
def test_closed_form_is_the_autograd_gradient(r, k):
    W = _w(r, k)
    _, g = ref.gradient(W, 1e-2)
    assert rel_err(ref.closed_form(W, 1e-2), g) <= 1e-12
    # a conv-shaped weight is its (Cout, -1) view
    if k % 9 == 0:
        W4 = W.reshape(r, k // 9, 3, 3)
        p4, g4 = ref.gradient(W4, 1e-2)
        assert g4.shape == W4.shape and rel_err(g4.reshape(r, k), g) <= 1e-12
        assert abs(p4.item() - ref.penalty(W, 1e-2).item()) <= 1e-12 * abs(p4.item())


@pytest.mark.parametrize('r,k', SHAPES)
def test_row_and_column_form_agree(r, k):
    W = _w(r, k, seed=1)
    p, g = ref.gradient(W, 0.5)
    for form in (ref.row_form, ref.column_form):
        pf, gf = form(W, 0.5)
        assert rel_err(gf, g) <= 1e-11, form.__name__
        assert abs(pf.item() - p.item()) <= 1e-11 * abs(p.item()), form.__name__


def test_one_row_has_no_penalty():
    W = _w(1, 64)
    p, g = ref.gradient(W, 1.0)
    assert p.item() == 0 and not g.any()


def test_config_fields_and_validation():
    from gan_lab_amd import ortho_reg
    from gan_lab_amd.config import make_config
    common = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)
    cfg = make_config('resnetgan', **common)
    assert cfg.ortho_reg == 0. and cfg.ortho_reg_d == 0. and ortho_reg.validate_config(cfg) == (0., 0.)
    cfg = make_config('resnetgan', ortho_reg=1e-4, ortho_reg_d=2e-4, **common)
    assert ortho_reg.validate_config(cfg) == (1e-4, 2e-4) and ortho_reg.OrthoReg.validate_config(cfg) == (1e-4, 2e-4)
    for field in ('ortho_reg', 'ortho_reg_d'):
        for bad in (-1, -1e-9, float('nan'), float('inf'), 'x', None, True):
            ns = types.SimpleNamespace(model='ResNet GAN', ortho_reg=0., ortho_reg_d=0.)
            setattr(ns, field, bad)
            with pytest.raises(ValueError, match=field):
                ortho_reg.validate_config(ns)
    with pytest.raises(ValueError, match='ResNet GAN'):
        ortho_reg.validate_config(types.SimpleNamespace(model='ProGAN', ortho_reg=1e-4))
    for model in ('progan', 'stylegan'):         # ResNet GAN rows only
        for field in ('ortho_reg', 'ortho_reg_d'):
            with pytest.raises(AttributeError):
                make_config(model, dev='cpu', pin_memory=False, **{field: 1e-4})


def test_learner_validates_the_strength(monkeypatch):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4, ortho_reg=-1.)
    with pytest.raises(ValueError, match='ortho_reg'):
        GANLearner(cfg)


def test_layer_enumeration():
    """Every Conv2dEx / LinearEx weight of a conditional generator with attention, and nothing else: no BatchNorm table, no
    bias, no gamma."""
    from gan_lab_amd.ortho_reg import regularised_layers
    from gan_lab_amd.resnetgan.architectures import Discriminator32PixResnet, Generator32PixResnet
    from gan_lab_amd.utils.custom_layers import Conv2dEx, LinearEx
    g = Generator32PixResnet(fmap=32, cgan=True, num_classes=3, self_attention=True)
    keys = [prefix + '.weight' for prefix, _, _ in regularised_layers(g)]
    params = dict(g.named_parameters())
    want = [k for k in params if k.endswith(('conv2d.weight', 'linear.weight'))]
    assert sorted(keys) == sorted(want) and len(set(keys)) == len(keys)
    n_layers = sum(isinstance(m, (Conv2dEx, LinearEx)) for m in g.modules())
    assert len(keys) == n_layers >= 10
    for prefix, _, holder in regularised_layers(g):
        assert params[prefix + '.weight'] is holder.weight and holder.weight.dim() in (2, 4)
    for name in ('theta', 'phi', 'g', 'o'):                  # attention's 1x1 convolutions are in
        assert f'self_attn.{name}.conv2d.weight' in keys
    left = [k for k in params if k not in keys]
    assert any(k.endswith('gamma') for k in left)
    assert any(params[k].shape[0] == 3 and params[k].dim() == 2 for k in left), 'the (num_classes, C) tables are exempt'
    assert all(not k.endswith('gamma') and 'bias' not in k for k in keys)
    assert all(not (params[k].dim() == 2 and params[k].shape[0] == 3) for k in keys)
    d = Discriminator32PixResnet(fmap=32, cgan=True, num_classes=3)
    assert 'proj.linear.weight' in [prefix + '.weight' for prefix, _, _ in regularised_layers(d)]


def test_job_table_layout():
    from gan_lab_amd import _lib, ops
    shapes = [(1, 64), (2, 3), (5, 7), (3, 576), (64, 27), (33, 130), (128, 64), (128, 576), (512, 4608), (2048, 128), (64, 64)]
    entries, need, (bg, ba) = ops.ortho_plan(shapes)
    assert len(entries) == len(shapes) and entries[0] is None          # R == 1 is skipped
    T, QR = _lib.ORTHO_TILE, _lib.ORTHO_QROWS
    areas, g0, a0 = [], 0, 0
    for (r, k), e in zip(shapes, entries):
        if r == 1:
            assert e is None
            continue
        m = min(r, k)
        assert e['m'] == m and e['form'] == (_lib.ORTHO_ROW if r <= k else _lib.ORTHO_COL)
        tm = -(-m // T)
        assert e['n_part'] == tm * tm + (0 if r <= k else -(-r // QR))
        assert (e['q'] is None) == (r <= k)
        assert e['blk_g0'] == g0 and e['blk_a0'] == a0                 # monotone, gap-free block offsets
        g0 += e['n_part']
        a0 += -(-r // T) * -(-k // T)
        areas.append((e['s'], m * m))
        areas.append((e['part'], e['n_part']))
        if e['q'] is not None:
            areas.append((e['q'], r))
    assert (bg, ba) == (g0, a0)
    assert ops.ortho_plan([(2048, 128)])[0][0]['m'] == 128             # never the (R, R) matrix
    areas.sort()
    for (o, n), (o2, _) in zip(areas, areas[1:]):
        assert o % 4 == 0 and o + n <= o2, 'scratch areas overlap or lose their 16-byte alignment'
    assert areas[-1][0] + areas[-1][1] <= need
    with pytest.raises(ValueError):
        ops.ortho_plan([(0, 4)])
    with pytest.raises(ValueError, match='no layers'):
        ops.OrthoTable([])
