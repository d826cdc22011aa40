"""Host-side tests of k-NN precision / recall / density / coverage (gan_lab_amd/prdc.py): the config options,
the evaluation object's bookkeeping (no GPU: GANLAB_HOST_LOGIC_ONLY=1), the float64 reference on closed-form cases, and the C
entry points' declarations and exports."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import prdc_reference as ref  # noqa: E402


# ---- the reference on closed-form cases ----------------------------------------------------------------------------------------
def test_reference_identical_sets_score_one():
    x = np.random.default_rng(0).standard_normal((40, 6))
    for k in (1, 3, 5):
        out = ref.prdc(x, x.copy(), k)
        assert out['precision'] == out['recall'] == out['coverage'] == 1.0
        # every generated row sits on a real row: it is inside that ball and inside the ball of every real that has it
        # among its k nearest
        assert out['density'] >= 1.0


def test_reference_far_apart_clusters_score_zero():
    rng = np.random.default_rng(1)
    real, fake = rng.standard_normal((30, 5)), rng.standard_normal((25, 5)) + 1000.0
    out = ref.prdc(real, fake, 4)
    assert out['precision'] == out['recall'] == out['density'] == out['coverage'] == 0.0


REAL5 = np.array([[0.], [1.], [3.], [6.], [30.]])
FAKE5 = np.array([[0.5], [2.], [5.], [100.], [2.]])        # rows 1 and 4 are duplicates: each is the other's nearest, at 0


def test_reference_hand_worked_five_points():
    """On a line.  Squared radii, k = 1: reals (1, 1, 4, 9, 576), fakes (2.25, 0, 9, 9025, 0); k = 2: reals (9, 4, 9, 25, 729),
    fakes (2.25, 2.25, 9, 9604, 2.25).  Fake 2 (at 5) is exactly on real 2's k = 1 boundary (4 <= 4: inside) and fake 1 (at 2)
    exactly on real 1's (1 <= 1).  Fake 3 (at 100) is inside no real ball but its own huge ball covers real 4: recall stays 1."""
    out, p = ref.prdc(REAL5, FAKE5, 1, parts=True)
    assert p['rad_r'].tolist() == [1, 1, 4, 9, 576] and p['rad_f'].tolist() == [2.25, 0, 9, 9025, 0]
    assert p['c_fr'].tolist() == [2, 2, 2, 0, 2]
    assert p['arg_fr'].tolist() == [0, 1, 3, 4, 1]              # ties at 0.25 (reals 0, 1) and 1 (reals 1, 2): the lowest index
    assert p['min_fr'].tolist() == [0.25, 1, 1, 4900, 1]
    assert (out['precision'], out['recall'], out['density'], out['coverage']) == (0.8, 1.0, 1.6, 0.8)
    out, p = ref.prdc(REAL5, FAKE5, 2, parts=True)
    assert p['rad_r'].tolist() == [9, 4, 9, 25, 729] and p['rad_f'].tolist() == [2.25, 2.25, 9, 9604, 2.25]
    assert p['lists_f'][1].tolist() == [0, 2.25]               # the duplicate at index 4 counts, the row itself does not
    assert p['c_fr'].tolist() == [3, 4, 3, 0, 4]
    assert (out['precision'], out['recall'], out['density'], out['coverage']) == (0.8, 1.0, 1.4, 1.0)
    assert (out['k'], out['n_real'], out['n_fake']) == (2, 5, 5)


# ---- config ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_defaults_and_overrides(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    c = make_config(model, **kw)
    assert (c.prdc_k, c.prdc_res) == (5, 32)
    assert 'prdc' not in [m.casefold() for m in c.gen_metrics]
    c = make_config(model, prdc_k=3, prdc_res=16, **kw)
    assert (c.prdc_k, c.prdc_res) == (3, 16)


def test_reference_format_checkpoint_omits_the_fields_while_the_metric_is_off():
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    for model in ('stylegan', 'progan'):
        off = make_config(model, dev='cpu', pin_memory=False)
        assert 'prdc_k' in vars(off) and not [k for k in checkpoint.reference_config_fields(off) if k.startswith('prdc')]
        on = make_config(model, dev='cpu', pin_memory=False, gen_metrics=['generator loss', 'PRDC'], prdc_k=3)
        kept = checkpoint.reference_config_fields(on)
        assert (kept['prdc_k'], kept['prdc_res']) == (3, 32)


def _ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def test_validate_config_bounds():
    from gan_lab_amd import prdc
    assert prdc.validate_config(_ns()) == (5, 32)
    assert prdc.validate_config(_ns(prdc_k=1, prdc_res=4)) == (1, 4)
    assert prdc.validate_config(_ns(prdc_k=16, prdc_res=1024, gen_metrics=['PRDC'], disc_metrics=['fake realness'])) == (16, 1024)
    for bad in (0, 17, -1, 2.0, True, None, '5'):
        with pytest.raises(ValueError, match='prdc_k'):
            prdc.validate_config(_ns(prdc_k=bad))
    for bad in (0, 2, 3, 24, 32.0, True, None):
        with pytest.raises(ValueError, match='prdc_res'):
            prdc.validate_config(_ns(prdc_res=bad))
    with pytest.raises(ValueError, match='generator metric'):
        prdc.validate_config(_ns(disc_metrics=['real realness', 'PRDC']))


def test_wanted():
    from gan_lab_amd import prdc
    assert prdc.wanted(['generator loss', 'PrDc']) and prdc.wanted(('prdc',))
    assert not prdc.wanted(['swd', 'precision']) and not prdc.wanted(None) and not prdc.wanted([])


def test_feature_dim():
    from gan_lab_amd import prdc
    assert prdc.feature_dim(3, 64, 32) == 3 * 32 * 32 and prdc.feature_dim(3, 8, 32) == 3 * 8 * 8
    assert prdc.feature_dim(3, 32, 4) == 48


def test_resnet_learner_refuses_prdc_among_the_critic_metrics(monkeypatch):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    kw = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4)
    with pytest.raises(ValueError, match='generator metric'):
        GANLearner(make_config('resnetgan', disc_metrics=['prdc'], **kw))
    with pytest.raises(ValueError, match='prdc_k'):
        GANLearner(make_config('resnetgan', prdc_k=17, **kw))


# ---- the evaluation object's bookkeeping -----------------------------------------------------------------------------------
def test_evaluator_needs_the_gpu_or_the_host_logic_switch(monkeypatch):
    from gan_lab_amd import prdc
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(TypeError, match='GPU only'):
        prdc.PRDC(8, 10, 10, device='cpu')


def test_evaluator_bookkeeping(monkeypatch):
    from gan_lab_amd import prdc
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    for bad in (dict(k=10), dict(k=12), dict(k=0), dict(k=17)):
        with pytest.raises(ValueError, match='k must be'):
            prdc.PRDC(8, 10, 20, device='cpu', **bad)           # k >= n_real
    with pytest.raises(ValueError, match='n_fake = 5'):
        prdc.PRDC(8, 10, 5, k=5, device='cpu')
    with pytest.raises(ValueError, match='dim'):
        prdc.PRDC(0, 10, 10, device='cpu')
    ev = prdc.PRDC(8, 10, 12, k=3, device='cpu')
    ev.feed_real(torch.zeros(4, 8))
    ev.feed_real(torch.zeros(6, 8))
    with pytest.raises(ValueError, match='declared with 10'):
        ev.feed_real(torch.zeros(1, 8))                         # overfeed
    with pytest.raises(ValueError, match=r'\(n, 8\) float32'):
        ev.feed_fake(torch.zeros(4, 7))                         # width mismatch
    with pytest.raises(ValueError, match='float32'):
        ev.feed_fake(torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match='float32'):
        ev.feed_fake(torch.zeros(4, 2, 4))
    ev.feed_fake(torch.zeros(8, 8))
    with pytest.raises(ValueError, match='12 fake rows were declared, 8 were fed'):
        ev.result()
    ev.feed_fake(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match='host logic only'):
        ev.result()
    ev.reset()
    ev.feed_fake(torch.zeros(12, 8))                            # the same buffers take the next evaluation
    with pytest.raises(ValueError, match='declared with 12'):
        ev.feed_fake(torch.zeros(1, 8))


# ---- the C surface ---------------------------------------------------------------------------------------------------------
NEW = ('ganlab_prdc_norms_f32', 'ganlab_prdc_knn_f32', 'ganlab_prdc_cross_f32')


def test_entry_points_are_declared_bound_and_exported():
    from gan_lab_amd import _lib, ops
    src = open(os.path.join(ROOT, 'include', 'ganlab_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', code), name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
    assert int(re.search(r'#define\s+GANLAB_PRDC_MAX_K\s+(\d+)', src).group(1)) == ops.PRDC_MAX_K == 16
    assert 'prdc.hip' in open(os.path.join(ROOT, 'gan_lab_amd', 'csrc', 'Makefile')).read()
    # argument checks of the entry points run before any launch: callable without a GPU
    L = _lib.lib()
    assert L.ganlab_prdc_norms_f32(None, None, 4, 4, None) == -1
    assert L.ganlab_prdc_knn_f32(None, None, None, 4, 4, 1, None) == -1


def test_wrappers_refuse_host_tensors():
    from gan_lab_amd import ops
    x = torch.zeros(8, 4)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.prdc_knn(x, 3)
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.prdc_cross(x, x, torch.zeros(8))
