"""Host-side tests of the Kernel Inception Distance (gan_lab_amd/kid.py): the float64 reference on closed-form
cases, the config options, the evaluation object's bookkeeping (no GPU: GANLAB_HOST_LOGIC_ONLY=1) and the C entry point's
declaration and export."""
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

import kid_reference as ref  # noqa: E402


# ---- the reference on closed-form cases ----------------------------------------------------------------------------------------
def test_reference_hand_worked_three_points():
    """On a line with gamma = 1, coef0 = 1: k(x, y) = (x y + 1)^3.  Reals (0, 1, 2), fakes (1, 1, 3):
    real-real off the diagonal 1, 1, 1, 27, 1, 27 = 58; fake-fake 8, 64, 8, 64, 64, 64 = 272; real-fake rows 3, 8 + 8 + 64 = 80,
    27 + 27 + 343 = 397, together 480.  mmd2 = 58 / 6 + 272 / 6 - 2 * 480 / 9."""
    real, fake = np.array([[0.], [1.], [2.]]), np.array([[1.], [1.], [3.]])
    s = ref.row_sums(real, fake, 1.0)
    assert s['real_real'].tolist() == [2, 28, 28] and s['fake_fake'].tolist() == [72, 72, 128]     # the duplicate counts
    assert s['real_fake'].tolist() == [3, 80, 397]
    assert ref.mmd2(real, fake, 1.0) == 58 / 6 + 272 / 6 - 2.0 * 480 / 9
    out = ref.kid(real, fake, block=2, gamma=1.0)
    assert (out['blocks'], out['block'], out['n_real'], out['n_fake'], out['kid_block_std']) == (1, 2, 3, 3, None)
    assert out['kid_block_mean'] == ref.mmd2(real[:2], fake[:2], 1.0) == 2 / 2 + 16 / 2 - 2.0 * 18 / 4


def test_reference_is_near_zero_for_one_distribution_and_positive_for_two():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((400, 16)), rng.standard_normal((400, 16))
    same, apart = ref.kid(a, b, block=100), ref.kid(a, b + 0.5, block=100)
    assert abs(same['kid']) < 0.02 < apart['kid']
    assert same['blocks'] == 4 and same['kid_block_std'] > 0 and abs(same['kid_block_mean']) < 3 * same['kid_block_std']


# ---- config ------------------------------------------------------------------------------------------------------------
def _ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def test_validate_config_bounds_and_wanted():
    from gan_lab_amd import kid
    assert kid.validate_config(_ns()) == (32, 1000)
    assert kid.validate_config(_ns(kid_res=4, kid_block=2, gen_metrics=['KID'], disc_metrics=['fake realness'])) == (4, 2)
    for bad in (0, 2, 3, 24, 32.0, True, None):
        with pytest.raises(ValueError, match='kid_res'):
            kid.validate_config(_ns(kid_res=bad))
    for bad in (1, 0, -5, 1000.0, True, None, '1000'):
        with pytest.raises(ValueError, match='kid_block'):
            kid.validate_config(_ns(kid_block=bad))
    with pytest.raises(ValueError, match='generator metric'):
        kid.validate_config(_ns(disc_metrics=['real realness', 'Kid']))
    assert kid.wanted(['generator loss', 'KID']) and kid.wanted(('kid',))
    assert not kid.wanted(['fd', 'mmd']) and not kid.wanted(None) and not kid.wanted([])


@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_overrides(model):
    from gan_lab_amd.config import make_config
    c = make_config(model, dev='cpu', pin_memory=False, kid_res=16, kid_block=50)
    assert (c.kid_res, c.kid_block) == (16, 50)


# ---- the evaluation object's bookkeeping -----------------------------------------------------------------------------------
def test_evaluator_needs_the_gpu_or_the_host_logic_switch(monkeypatch):
    from gan_lab_amd import kid
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(TypeError, match='GPU only'):
        kid.KID(8, 10, 10, device='cpu')


def test_evaluator_bookkeeping(monkeypatch):
    from gan_lab_amd import kid
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    for bad in (dict(n_real=1), dict(n_fake=1), dict(n_real=0), dict(n_fake=2.0)):
        with pytest.raises(ValueError, match='>= 2'):
            kid.KID(8, **{'n_real': 10, 'n_fake': 10, **bad}, device='cpu')          # fewer than 2 rows
    with pytest.raises(ValueError, match='dim'):
        kid.KID(0, 10, 10, device='cpu')
    for bad in (1, 0, 2.0, True):
        with pytest.raises(ValueError, match='block'):
            kid.KID(8, 10, 10, block=bad, device='cpu')
    with pytest.raises(ValueError, match='gamma'):
        kid.KID(8, 10, 10, gamma=float('nan'), device='cpu')
    ev = kid.KID(8, 10, 12, block=4, device='cpu')
    assert (ev.gamma, ev.coef0, ev.blocks, ev.block) == (1 / 8, 1.0, 2, 4)
    assert kid.KID(8, 10, 12, gamma=0.5, coef0=0.0, device='cpu').gamma == 0.5
    # B = min(n_real, n_fake) // block
    assert [kid.KID(8, n, m, block=b, device='cpu').blocks for n, m, b in
            ((10, 12, 1000), (10, 12, 11), (10, 12, 10), (12, 10, 5), (2000, 3999, 1000), (4000, 3999, 1000))] == [0, 0, 1, 2, 2, 3]
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
    with pytest.raises(ValueError, match='12 fake rows were declared, 8 were fed'):
        ev.row_sums()
    ev.feed_fake(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match='host logic only'):
        ev.result()
    ev.reset()
    ev.feed_fake(torch.zeros(12, 8))                            # the same object takes the next evaluation
    with pytest.raises(ValueError, match='declared with 12'):
        ev.feed_fake(torch.zeros(1, 8))


# ---- the C surface ---------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    from gan_lab_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'ganlab_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.SO_PATH)
    name = 'ganlab_kid_rowsums_f32'
    assert re.search(r'\bint\s+' + name + r'\s*\(', code) and name in _lib.SIGNATURES and hasattr(handle, name)
    assert 'kid.hip' in open(os.path.join(ROOT, 'gan_lab_amd', 'csrc', 'Makefile')).read()
    # argument checks of the entry point run before any launch: callable without a GPU
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.ganlab_kid_rowsums_f32(None, 4, None, 4, 4, 0.25, 1.0, 0, None, None) == -1
    assert L.ganlab_kid_rowsums_f32(buf, 4, buf, 5, 4, 0.25, 1.0, 1, buf, None) == -1            # exclude_diag with M != N
    assert L.ganlab_kid_rowsums_f32(buf, 4, buf, 4, 4, 0.25, 1.0, 2, buf, None) == -1
    assert L.ganlab_kid_rowsums_f32(buf, 0, buf, 4, 4, 0.25, 1.0, 0, buf, None) == -1
    assert L.ganlab_kid_rowsums_f32(buf, 4, buf, 4, 0, 0.25, 1.0, 0, buf, None) == -1
    assert L.ganlab_kid_rowsums_f32(buf, 4, buf, 2 ** 30 + 1, 4, 0.25, 1.0, 0, buf, None) == -1


def test_wrapper_refuses_host_tensors():
    from gan_lab_amd import ops
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.kid_rowsums(torch.zeros(8, 4), torch.zeros(8, 4), 0.25)
