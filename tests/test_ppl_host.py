"""Host-side tests of the perceptual path length (gan_lab_amd/ppl.py, csrc/ppl.hip): the config fields, their CLI
flags and every refusal; the float64 reference (tests/ppl_reference.py) against independent compositions; the C entry points'
declarations, exports and argument checks (no GPU: the checks come before any launch)."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ppl_reference as ref  # noqa: E402

PROGRESSIVE = ('stylegan', 'progan')
FIELDS = ('ppl_samples', 'ppl_space', 'ppl_sampling', 'ppl_epsilon', 'ppl_seed')


def _ns(**kw):
    return types.SimpleNamespace(**kw)


# ---- config ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', PROGRESSIVE)
def test_config_defaults_and_overrides(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    c = make_config(model, **kw)
    assert (c.ppl_samples, c.ppl_space, c.ppl_sampling, c.ppl_epsilon, c.ppl_seed) == (1024, None, 'full', 1e-4, 0)
    assert 'ppl' not in {m.casefold() for m in c.gen_metrics}
    c = make_config(model, ppl_samples=64, ppl_space='z', ppl_sampling='end', ppl_epsilon=1e-3, ppl_seed=7, **kw)
    assert (c.ppl_samples, c.ppl_space, c.ppl_sampling, c.ppl_epsilon, c.ppl_seed) == (64, 'z', 'end', 1e-3, 7)


def test_resnet_gan_has_no_such_fields():
    from gan_lab_amd import config
    assert not any(row[0].startswith('ppl_') for row in config._spec('ResNet GAN'))
    for field in FIELDS:
        with pytest.raises(AttributeError, match=field):
            config.make_config('resnetgan', dev='cpu', pin_memory=False, **{field: 1})
    for model in ('ProGAN', 'StyleGAN'):
        assert set(FIELDS) <= {row[0] for row in config._spec(model)}
    assert all(f in config.__doc__ for f in FIELDS)


@pytest.mark.parametrize('model', PROGRESSIVE)
def test_cli_round_trip(model, tmp_path, monkeypatch):
    from gan_lab_amd import config
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    common = [model, '--dev=cpu', '--pin_memory=false', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(common + ['--ppl_samples=256', '--ppl_space=Z', '--ppl_sampling=END', '--ppl_epsilon=1e-3', '--ppl_seed=11'])
    assert (c.ppl_samples, c.ppl_space, c.ppl_sampling, c.ppl_epsilon, c.ppl_seed) == (256, 'z', 'end', 1e-3, 11)
    c = config.main(common + ['--ppl_space=none'])
    assert (c.ppl_samples, c.ppl_space, c.ppl_sampling, c.ppl_epsilon, c.ppl_seed) == (1024, None, 'full', 1e-4, 0)


def test_validate_config_resolves_the_space_and_refuses_by_field():
    from gan_lab_amd import ppl
    assert ppl.validate_config(_ns()) == (1024, 'w', 'full', 1e-4, 0)
    assert ppl.validate_config(_ns(model='StyleGAN')) == (1024, 'w', 'full', 1e-4, 0)
    assert ppl.validate_config(_ns(model='ProGAN')) == (1024, 'z', 'full', 1e-4, 0)
    assert ppl.validate_config(_ns(model='StyleGAN', ppl_space='z', ppl_samples=2, ppl_sampling='end', ppl_epsilon=0.5,
                                   ppl_seed=2 ** 63 - 1, gen_metrics=['PPL'], disc_metrics=['fake realness'])) == \
        (2, 'z', 'end', 0.5, 2 ** 63 - 1)
    for bad in (1, 0, -4, 1024.0, True, None, '1024'):
        with pytest.raises(ValueError, match='ppl_samples'):
            ppl.validate_config(_ns(ppl_samples=bad))
    for bad in ('w+', 'W', 'x', 0, True):
        with pytest.raises(ValueError, match='ppl_space'):
            ppl.validate_config(_ns(ppl_space=bad))
    with pytest.raises(ValueError, match='ppl_space'):
        ppl.validate_config(_ns(model='ProGAN', ppl_space='w'))
    for bad in ('FULL', 'start', None, 1):
        with pytest.raises(ValueError, match='ppl_sampling'):
            ppl.validate_config(_ns(ppl_sampling=bad))
    for bad in (0.0, -1e-4, float('nan'), float('inf'), 1.0, None, 'x', True):
        with pytest.raises(ValueError, match='ppl_epsilon'):
            ppl.validate_config(_ns(ppl_epsilon=bad))
    for bad in (-1, 2 ** 63, 1.0, True, None):
        with pytest.raises(ValueError, match='ppl_seed'):
            ppl.validate_config(_ns(ppl_seed=bad))
    with pytest.raises(ValueError, match='generator metric'):
        ppl.validate_config(_ns(disc_metrics=['real realness', 'Ppl']))
    assert ppl.wanted(['generator loss', 'PPL']) and ppl.wanted(('ppl',))
    assert not ppl.wanted(['fd', 'pl']) and not ppl.wanted(None) and not ppl.wanted([])


def _learner(monkeypatch, kind, **kw):
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


@pytest.mark.parametrize('kind', PROGRESSIVE)
def test_learner_validates_the_fields_when_it_is_built(monkeypatch, kind):
    for field, bad in (('ppl_samples', 1), ('ppl_space', 'w+'), ('ppl_sampling', 'middle'), ('ppl_epsilon', 0.0),
                       ('ppl_seed', -1)):
        with pytest.raises(ValueError, match=field):
            _learner(monkeypatch, kind, **{field: bad})
    with pytest.raises(ValueError, match='generator metric'):
        _learner(monkeypatch, kind, disc_metrics=['ppl'])
    _learner(monkeypatch, kind, gen_metrics=['generator loss', 'ppl'], ppl_space='z')          # legal among the generator's
    if kind == 'progan':
        with pytest.raises(ValueError, match='ppl_space'):
            _learner(monkeypatch, kind, ppl_space='w')
    else:
        _learner(monkeypatch, kind, ppl_space='w')


def test_compute_metrics_refuses_ppl_for_the_critic(monkeypatch):
    L = _learner(monkeypatch, 'progan')
    with pytest.raises(ValueError, match='generator metric'):
        L.compute_metrics(['ppl'], 'Discriminator', None, None)


def test_reference_format_checkpoint_omits_the_fields_while_the_metric_is_off():
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    for model in PROGRESSIVE:
        off = make_config(model, dev='cpu', pin_memory=False)
        assert 'ppl_samples' in vars(off) and not [k for k in checkpoint.reference_config_fields(off) if k.startswith('ppl_')]
        on = make_config(model, dev='cpu', pin_memory=False, gen_metrics=['generator loss', 'PPL'], ppl_samples=8)
        kept = checkpoint.reference_config_fields(on)
        assert kept['ppl_samples'] == 8 and set(FIELDS) <= set(kept) and not [k for k in kept if k.startswith('kid_')]


def test_path_length_refuses_bad_arguments_before_touching_a_tensor():
    from gan_lab_amd import ppl
    z = torch.zeros(4, 8)
    for kw, name in ((dict(mode='nlerp'), 'mode'), (dict(sampling='mid'), 'sampling'), (dict(epsilon=0), 'epsilon'),
                     (dict(batch=0), 'batch'), (dict(trim=(99, 1)), 'trim'), (dict(trim=(1,)), 'trim'), (dict(seed=-1), 'seed')):
        with pytest.raises(ValueError, match=name):
            ppl.path_length(lambda x: x, z, z, **{'mode': 'lerp', **kw})
    with pytest.raises(TypeError, match='no CPU fallback'):
        ppl.path_length(lambda x: x, z, z, 'lerp')
    with pytest.raises(TypeError, match='learner or generator'):
        ppl.generator_path_length(object(), 8, 'z')


# ---- the reference against independent compositions ---------------------------------------------------------------------------
def test_reference_uniform_draw_is_a_prefix_and_in_range():
    short, long = ref.uniforms(12345, 7, 5), ref.uniforms(12345, 7, 257)
    assert np.array_equal(short, long[:5]) and np.array_equal(ref.uniforms(12345, 9, 3), long[2:5])
    assert (long >= 0).all() and (long < 1).all() and len(set(long.tolist())) == 257
    assert np.array_equal(long.astype(np.float32).astype(np.float64), long)                       # multiples of 2^-24
    assert 0.35 < long.mean() < 0.65
    assert not np.array_equal(ref.uniforms(12346, 7, 5), short)


def test_reference_slerp_on_known_angles():
    """3-D rows with known angles against torch.acos / sin composed by hand: orthogonal rows at t = 0.5 give the bisector."""
    a = torch.tensor([[2.0, 0, 0], [0, 3.0, 0], [1.0, 1.0, 0]], dtype=torch.float64)
    b = torch.tensor([[0, 5.0, 0], [0, 0, 0.5], [0, 0, 4.0]], dtype=torch.float64)
    out = ref.endpoints(a, b, [0.5, 0.25, 1.0], 0.125, 'slerp')
    r3, h = 3 ** 0.5, 0.5 ** 0.5
    assert torch.allclose(out[0, 0], torch.tensor([h * r3, h * r3, 0], dtype=torch.float64), atol=1e-15)
    for n, t in enumerate((0.5, 0.25, 1.0)):
        ah, bh = a[n] / a[n].norm(), b[n] / b[n].norm()
        omega = torch.acos((ah * bh).sum())                  # pi / 2 for every pair here
        assert abs(float(omega) - np.pi / 2) < 1e-15
        for e, tt in enumerate((t, t + 0.125)):
            want = (torch.sin((1 - tt) * omega) * ah + torch.sin(tt * omega) * bh) / torch.sin(omega) * r3      # Shoemake's form
            assert torch.allclose(out[e, n], want, atol=1e-14), (n, e)
            assert abs(float(out[e, n].norm()) - r3) < 1e-14
    # a non-right angle: 60 degrees between (1, 0, 0) and (1/2, sqrt(3)/2, 0); at t = 0.5 the point sits at 30 degrees
    a, b = torch.tensor([[1.0, 0, 0]], dtype=torch.float64), torch.tensor([[0.5, 0.75 ** 0.5, 0]], dtype=torch.float64)
    out = ref.endpoints(a, b, [0.5], 0.5, 'slerp')
    assert torch.allclose(out[0, 0], torch.tensor([0.75 ** 0.5 * r3, 0.5 * r3, 0], dtype=torch.float64), atol=1e-14)
    assert torch.allclose(out[1, 0], b[0] * r3, atol=1e-14)


def test_reference_slerp_fallback_rows_and_lerp():
    a = torch.tensor([[1.0, 2.0, 2.0], [1.0, 2.0, 2.0], [1.0, 2.0, 2.0], [0, 0, 0], [1.0, 2.0, 2.0]], dtype=torch.float64)
    b = torch.stack([a[0], -a[0], 2 * a[0], torch.tensor([1.0, 0, 0], dtype=torch.float64), torch.zeros(3, dtype=torch.float64)])
    for dtype in (torch.float64, torch.float32):
        out = ref.endpoints(a, b, [0.3] * 5, 1e-2, 'slerp', dtype)
        assert torch.isfinite(out).all() and torch.equal(out[0], out[1])
        want = a[0] / 3 * 3 ** 0.5
        for n in (0, 1, 2, 4):
            assert torch.allclose(out[0, n].double(), want, atol=1e-6 if dtype == torch.float32 else 1e-15)
        assert torch.equal(out[0, 3], torch.zeros(3, dtype=dtype))
    x, y = torch.tensor([[1.0, -2.0]], dtype=torch.float64), torch.tensor([[3.0, 2.0]], dtype=torch.float64)
    out = ref.endpoints(x, y, [0.25], 0.5, 'lerp')
    assert out[0, 0].tolist() == [1.5, -1.0] and out[1, 0].tolist() == [2.5, 1.0]
    assert ref.row_sqdist(x, y).tolist() == [20.0]


@pytest.mark.parametrize('q', [(0.01, 0.99), (0.0, 1.0), (0.25, 0.5), (0.1, 0.1)])
def test_reference_trimmed_mean_is_numpys_percentiles_and_a_masked_mean(q):
    rng = np.random.default_rng(3)
    sizes = list(range(1, 303)) + [1000, 1001, 4097, 2 ** 17 + 1]
    for n in sizes:
        v = rng.standard_normal(n).astype(np.float32)
        if n > 10:
            v[: n // 3] = np.round(v[: n // 3])                    # blocks of ties, some straddling a bound
        got = ref.trimmed_mean(v, *q)
        lo = np.percentile(v, 100 * q[0], method='lower')
        hi = np.percentile(v, 100 * q[1], method='higher')
        mask = (v >= lo) & (v <= hi)
        assert (got['lo'], got['hi'], got['kept'], got['nonfinite']) == (float(lo), float(hi), int(mask.sum()), 0), n
        assert abs(got['mean'] - v[mask].astype(np.float64).mean()) <= 1e-13 * max(1.0, abs(got['mean'])), n
    for bad in (np.nan, np.inf, -np.inf):
        got = ref.trimmed_mean(np.array([1.0, bad, 3.0], dtype=np.float32), *q)
        assert np.isnan(got['mean']) and got['nonfinite'] == 1


def test_reference_path_length_of_a_linear_map_is_its_closed_form():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(50, 12, generator=g, dtype=torch.float64), torch.randn(50, 12, generator=g, dtype=torch.float64)
    m = torch.randn(12, 192, generator=g, dtype=torch.float64)
    synth = lambda w: (w @ m).view(-1, 3, 8, 8)      # noqa: E731
    out = ref.path_length(synth, a, b, 'lerp', epsilon=2.0 ** -7, weights=(1.0,))
    want = (((b - a) @ m) ** 2).mean(1)
    assert torch.allclose(out['distances'] / 2.0 ** -14, want, rtol=1e-9)
    emb = ref.path_length(synth, a, b, 'lerp', epsilon=2.0 ** -7, embed=lambda x: x.flatten(1))
    assert torch.allclose(emb['distances'] / 2.0 ** -14, want * 192, rtol=1e-9)
    # 50 values: floor(0.01 * 49) = 0 and ceil(0.99 * 49) = 49, nothing is trimmed; the mean is over the fp32 distances
    mean = out['distances'].to(torch.float32).double().mean().item()
    assert out['kept'] == 50 and abs(out['ppl'] - mean / 2.0 ** -14) <= 1e-12 * out['ppl']
    # 'end' sampling: t = 0, the first end is a itself
    assert torch.equal(ref.endpoints(a, b, np.zeros(50), 0.5, 'lerp')[0], a)


# ---- the C surface ---------------------------------------------------------------------------------------------------------
NAMES = ('ganlab_ppl_endpoints_f32', 'ganlab_row_sqdist_f32', 'ganlab_trimmed_mean_workspace', 'ganlab_trimmed_mean_f32')


def test_entry_points_are_declared_bound_and_exported():
    from gan_lab_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'ganlab_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', code) and name in _lib.SIGNATURES and hasattr(handle, name), name
    assert re.search(r'\bppl\.hip\b', open(os.path.join(ROOT, 'gan_lab_amd', 'csrc', 'Makefile')).read())
    assert os.path.exists(os.path.join(ROOT, 'gan_lab_amd', 'csrc', 'ppl.hip'))


def test_entry_points_check_their_arguments_before_any_launch():
    from gan_lab_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    ends = L.ganlab_ppl_endpoints_f32
    assert ends(None, buf, buf, buf, 2, 4, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, None, buf, buf, 2, 4, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, None, buf, 2, 4, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, None, 2, 4, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 0, 4, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2 ** 31, 4, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2, 0, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2, 4097, 1e-4, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2, 4, 0.0, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2, 4, float('nan'), 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2, 4, 1.0, 0, 0, 0, 0, None) == -1
    assert ends(buf, buf, buf, buf, 2, 4, 1e-4, 2, 0, 0, 0, None) == -1              # mode
    assert ends(buf, buf, buf, buf, 2, 4, 1e-4, 0, 2, 0, 0, None) == -1              # sampling
    sq = L.ganlab_row_sqdist_f32
    assert sq(None, buf, buf, 2, 4, None) == -1 and sq(buf, None, buf, 2, 4, None) == -1 and sq(buf, buf, None, 2, 4, None) == -1
    assert sq(buf, buf, buf, 0, 4, None) == -1 and sq(buf, buf, buf, 2, 0, None) == -1 and sq(buf, buf, buf, 2 ** 31, 4, None) == -1
    assert L.ganlab_trimmed_mean_workspace(0) == 0 and L.ganlab_trimmed_mean_workspace(2 ** 31) == 0
    assert L.ganlab_trimmed_mean_workspace(1000) >= 4000          # the sorted copy alone (a long sort's size needs the device)
    tm = L.ganlab_trimmed_mean_f32
    assert tm(None, 8, 0.01, 0.99, buf, buf, 256, None) == -1
    assert tm(buf, 8, 0.01, 0.99, None, buf, 256, None) == -1
    assert tm(buf, 8, 0.01, 0.99, buf, None, 256, None) == -1
    assert tm(buf, 0, 0.01, 0.99, buf, buf, 256, None) == -1
    assert tm(buf, 8, -0.01, 0.99, buf, buf, 256, None) == -1
    assert tm(buf, 8, 0.01, 1.01, buf, buf, 256, None) == -1
    assert tm(buf, 8, 0.6, 0.4, buf, buf, 256, None) == -1
    assert tm(buf, 8, float('nan'), 0.99, buf, buf, 256, None) == -1
    assert tm(buf, 1000, 0.01, 0.99, buf, buf, 16, None) == -2                         # workspace too small


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from gan_lab_amd import ops
    z = torch.zeros(4, 8)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.ppl_endpoints(z, z, 1e-4, 'lerp')
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.row_sqdist(z, z)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.trimmed_mean(torch.zeros(8))
    for bad in (0, -1.0, float('nan'), float('inf'), 1.0, None, True):
        with pytest.raises(ValueError, match='epsilon'):
            ops.check_ppl_epsilon(bad)
    assert ops.check_ppl_epsilon(2.0 ** -7) == 2.0 ** -7
    assert (ops.PPL_MAX_DIM, ops.PPL_RECORD) == (4096, ('mean', 'lo', 'hi', 'kept', 'nonfinite'))
