"""Host-side tests of the Frechet distance (gan_lab_amd/frechet.py): the closed form ``distance`` (plain float64
torch, solved on the host) against the float64 numpy restatement and scipy's matrix square root, the config options, the
evaluation object's bookkeeping (no GPU: GANLAB_HOST_LOGIC_ONLY=1) and the C entry point's declaration and export."""
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

import frechet_reference as ref  # noqa: E402

CASES = {'full rank n=200 D=48': (200, 48), 'rank deficient n=40 D=96': (40, 96)}


def _two_sets(n, d):
    real = ref.offset_rows(n, d, seed=d)
    fake = ref.offset_rows(n, d, seed=d + 1, offset=100.5, scale=1.2)
    return ref.moments(real), ref.moments(fake)


# ---- the closed form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_distance_matches_the_reference_and_sqrtm(case):
    """Against the numpy restatement: both are float64 symmetric eigenproblems, whose eigenvalues carry an error of the order of
    2^-52 |A|, |A| <= |C_r| |C_f| (spectral norms).  At full rank that is 1e-12 of tr C_r + tr C_f after the square root.  With
    n rows and D > n - 1 columns, D - n + 1 eigenvalues are 0 in exact arithmetic and come out as that error, of either sign:
    each adds up to sqrt(2^-52 |C_r| |C_f|) to the sum of square roots, in either implementation, so the bar gains
    2 (D - n + 1) sqrt(2^-52 |C_r| |C_f|) - around 1e-8 of the distance here, the accuracy of this form for such sets.
    Against scipy.linalg.sqrtm (a Schur method for general matrices): 1e-10 relative at full rank, the same bar when rank
    deficient (there sqrtm returns a complex matrix; its real part is taken)."""
    from gan_lab_amd import frechet
    (mr, cr), (mf, cf) = _two_sets(*CASES[case])
    got, want = frechet.distance(mr, cr, mf, cf), ref.distance(mr, cr, mf, cf)
    assert set(got) == {'fd', 'mean_term', 'trace_term'} and all(isinstance(v, float) for v in got.values())
    scale = np.trace(cr) + np.trace(cf)
    print(f'{case}: fd {got["fd"]:.12g} (reference {want["fd"]:.12g}), difference {abs(got["fd"] - want["fd"]) / scale:.2e} of '
          f'tr C_r + tr C_f')
    assert got['mean_term'] == pytest.approx(want['mean_term'], rel=1e-14)
    n, d = CASES[case]
    null = max(d - (n - 1), 0)
    bar = 1e-12 * scale + 2 * null * np.sqrt(2.0 ** -52 * np.linalg.norm(cr, 2) * np.linalg.norm(cf, 2))
    assert abs(got['trace_term'] - want['trace_term']) <= bar
    assert abs(got['fd'] - want['fd']) <= bar
    assert got['fd'] > 0.01 * scale                     # a test of the inputs: the two sets are far apart
    linalg = pytest.importorskip('scipy.linalg')
    root = linalg.sqrtm(cr @ cf)
    fd_sqrtm = float((mr - mf) @ (mr - mf) + np.trace(cr) + np.trace(cf) - 2.0 * np.trace(root).real)
    print(f'{case}: against scipy.linalg.sqrtm {abs(got["fd"] - fd_sqrtm) / fd_sqrtm:.2e} relative')
    assert abs(got['fd'] - fd_sqrtm) <= 1e-10 * fd_sqrtm + 2 * bar


@pytest.mark.parametrize('case', sorted(CASES))
def test_identical_moments_give_zero_to_rounding(case):
    """fd of a set with itself is 0 up to the rounding of tr C - tr (C C)^(1/2); the bar is 10x what the float64 reference itself
    returns.  Measured: full rank, tr C 5.7e2: reference -3.7e-11, distance 4.5e-13; rank deficient, tr C 2.2e3: reference
    -7.3e-5, distance -2.1e-5 (the zero eigenvalues' rounding under a square root, see above).  Where the reference returns an
    exact 0 the bar is 10 units of 2^-53 tr C."""
    from gan_lab_amd import frechet
    (mr, cr), _ = _two_sets(*CASES[case])
    got, want = frechet.distance(mr, cr, mr, cr)['fd'], ref.distance(mr, cr, mr, cr)['fd']
    print(f'{case}: identical moments: distance {got:.3e}, reference {want:.3e}, tr C {np.trace(cr):.3e}')
    assert abs(got) <= 10 * max(abs(want), 2.0 ** -53 * np.trace(cr))


def test_isotropic_gaussians_closed_form():
    """N(m1, 4 I) and N(m2, 9 I) in D dimensions: |m1 - m2|^2 + D (2 - 3)^2, every intermediate an exact float."""
    from gan_lab_amd import frechet
    d = 12
    m1, m2 = np.arange(d, dtype=np.float64), np.arange(d, dtype=np.float64) + 2.0
    got = frechet.distance(m1, 4.0 * np.eye(d), m2, 9.0 * np.eye(d))
    assert got == {'fd': 4.0 * d + d, 'mean_term': 4.0 * d, 'trace_term': float(d)}
    assert ref.distance(m1, 4.0 * np.eye(d), m2, 9.0 * np.eye(d))['fd'] == 5.0 * d


def test_distance_accepts_tensors_and_checks_shapes():
    from gan_lab_amd import frechet
    c = torch.eye(3, dtype=torch.float64)
    assert frechet.distance(torch.zeros(3), c, torch.ones(3), c)['fd'] == 3.0
    with pytest.raises(ValueError, match='one width'):
        frechet.distance(torch.zeros(3), c, torch.zeros(4), c)
    with pytest.raises(ValueError, match='one width'):
        frechet.distance(torch.zeros(3), torch.eye(4), torch.zeros(3), c)


# ---- config ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_defaults_and_overrides(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    c = make_config(model, **kw)
    assert (c.fd_res, c.kid_res, c.kid_block) == (16, 32, 1000)
    assert not {'fd', 'kid'} & {m.casefold() for m in c.gen_metrics}
    c = make_config(model, fd_res=8, **kw)
    assert c.fd_res == 8


def _ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def test_validate_config_bounds_and_wanted():
    from gan_lab_amd import frechet
    assert frechet.validate_config(_ns()) == 16
    assert frechet.validate_config(_ns(fd_res=4, gen_metrics=['FD'], disc_metrics=['fake realness'])) == 4
    for bad in (0, 2, 3, 24, 16.0, True, None):
        with pytest.raises(ValueError, match='fd_res'):
            frechet.validate_config(_ns(fd_res=bad))
    with pytest.raises(ValueError, match='generator metric'):
        frechet.validate_config(_ns(disc_metrics=['real realness', 'Fd']))
    assert frechet.wanted(['generator loss', 'FD']) and frechet.wanted(('fd',))
    assert not frechet.wanted(['fid', 'kid']) and not frechet.wanted(None) and not frechet.wanted([])


def test_reference_format_checkpoint_omits_the_fields_while_the_metrics_are_off():
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    for model in ('stylegan', 'progan'):
        off = make_config(model, dev='cpu', pin_memory=False)
        assert 'fd_res' in vars(off) and not [k for k in checkpoint.reference_config_fields(off) if k.startswith(('fd_', 'kid_'))]
        on = make_config(model, dev='cpu', pin_memory=False, gen_metrics=['generator loss', 'FD'], fd_res=8)
        kept = checkpoint.reference_config_fields(on)
        assert kept['fd_res'] == 8 and not [k for k in kept if k.startswith('kid_')]
        on = make_config(model, dev='cpu', pin_memory=False, gen_metrics=['kid'], kid_block=10)
        kept = checkpoint.reference_config_fields(on)
        assert (kept['kid_res'], kept['kid_block']) == (32, 10) and 'fd_res' not in kept


def test_resnet_learner_refuses_the_names_among_the_critic_metrics(monkeypatch):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    kw = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4)
    for name in ('fd', 'kid'):
        with pytest.raises(ValueError, match='generator metric'):
            GANLearner(make_config('resnetgan', disc_metrics=[name], **kw))
    with pytest.raises(ValueError, match='fd_res'):
        GANLearner(make_config('resnetgan', fd_res=12, **kw))
    with pytest.raises(ValueError, match='kid_res'):
        GANLearner(make_config('resnetgan', kid_res=2, **kw))
    with pytest.raises(ValueError, match='kid_block'):
        GANLearner(make_config('resnetgan', kid_block=1, **kw))


# ---- the evaluation object's bookkeeping -----------------------------------------------------------------------------------
def test_evaluator_needs_the_gpu_or_the_host_logic_switch(monkeypatch):
    from gan_lab_amd import frechet
    monkeypatch.delenv('GANLAB_HOST_LOGIC_ONLY', raising=False)
    with pytest.raises(TypeError, match='GPU only'):
        frechet.Frechet(8, device='cpu')


def test_evaluator_bookkeeping(monkeypatch):
    from gan_lab_amd import frechet
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    for bad in (0, 4097, 8.0, True):
        with pytest.raises(ValueError, match='dim'):
            frechet.Frechet(bad, device='cpu')
    with pytest.raises(ValueError, match='pivot'):
        frechet.Frechet(8, device='cpu', pivot=torch.zeros(7))
    with pytest.raises(ValueError, match='pivot'):
        frechet.Frechet(8, device='cpu', pivot=torch.zeros(8, dtype=torch.float64))
    ev = frechet.Frechet(8, device='cpu')
    with pytest.raises(ValueError, match=r'\(n, 8\) float32'):
        ev.feed_real(torch.zeros(4, 7))                         # width mismatch
    with pytest.raises(ValueError, match='float32'):
        ev.feed_real(torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match='float32'):
        ev.feed_fake(torch.zeros(4, 2, 4))
    ev.feed_real(torch.zeros(1, 8))
    ev.feed_fake(torch.zeros(5, 8))
    with pytest.raises(ValueError, match='at least 2 real rows, 1 were fed'):
        ev.result()
    with pytest.raises(ValueError, match='at least 2 real rows'):
        ev.moments('real')
    with pytest.raises(ValueError, match="'real' or 'fake'"):
        ev.moments('both')
    ev.feed_real(torch.zeros(300, 8))                           # any number of rows, any number of feeds
    with pytest.raises(RuntimeError, match='host logic only'):
        ev.result()
    ev.reset()
    with pytest.raises(ValueError, match='at least 2 real rows, 0 were fed'):
        ev.result()


# ---- the C surface ---------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    from gan_lab_amd import _lib, ops
    src = open(os.path.join(ROOT, 'include', 'ganlab_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.SO_PATH)
    name = 'ganlab_moments_accum_f32'
    assert re.search(r'\bint\s+' + name + r'\s*\(', code) and name in _lib.SIGNATURES and hasattr(handle, name)
    assert 'frechet.hip' in open(os.path.join(ROOT, 'gan_lab_amd', 'csrc', 'Makefile')).read()
    assert ops.MOMENTS_MAX_DIM == 4096
    # argument checks of the entry point run before any launch: callable without a GPU
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.ganlab_moments_accum_f32(None, 4, 4, None, None, None, None) == -1
    for n, d in ((0, 4), (4, 0), (2 ** 30 + 1, 4), (4, 4097)):
        assert L.ganlab_moments_accum_f32(buf, n, d, buf, buf, buf, None) == -1, (n, d)


def test_wrapper_refuses_host_tensors():
    from gan_lab_amd import ops
    with pytest.raises(TypeError, match='no CPU fallback'):
        ops.moments_accum(torch.zeros(8, 4), torch.zeros(4), torch.zeros(4, dtype=torch.float64),
                          torch.zeros(4, 4, dtype=torch.float64))
