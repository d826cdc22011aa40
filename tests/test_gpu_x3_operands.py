"""The split-product (3 x bf16) conv kernels on the operands a training step feeds them (csrc/conv_x3*.hip).

tests/test_gpu_x3.py and tests/test_gpu_x3_persistent.py draw every operand from ``randn``: zero mean, unit scale, one binade
wide, no zeros.  Training feeds these kernels one-signed post-LeakyReLU activations, activations with a large common offset,
gradients that span many binades, planes with exact zeros and, now and then, a non-finite value - and each of these leans on
another part of the arithmetic: the exact three-way split h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), the three dropped
cross products, the hi*hi accumulator and its chains of 288 / 1024 terms, the InstanceNorm sums of the layer tail.

Every form of tests/x3_forms.py runs under every distribution there, three ways (split-product kernel, exact-fp32 kernel,
float64 on the CPU), at the bars of tests/test_gpu_x3.py:
  * max-relative error <= TOL = 2e-4 against float64 and against the exact kernel;
  * "fp32" = the rms error against float64 is at most 1.1 x the exact kernel's (weight gradients: or 2.5e-7, ATen's own level).
    The layer tail's mean and rstd take the first bar only, like tests/test_gpu_x3_persistent.py: they are 384 numbers at the
    rounding of their own fp32 result, where a ratio of two such errors says nothing.
A case whose split-product launch fell back to the exact kernel fails: both runs' launched symbols are asserted.
Measured ratios per distribution: DESIGN.md section 4.0."""
import pytest
import torch

import x3_forms as X
from util import assert_close, rel_err
from x3_forms import TOL, WGRAD_FLOOR, rms_rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gan_lab_amd import ops as _ops, _lib
    _lib.lib()
    return _ops


def check_dispatch(f, r):
    assert X.ran(f.symbol, r.launched_x3), (f.name, f.symbol, r.launched_x3)
    assert r.launched_exact and not X.ran(f.symbol, r.launched_exact), (f.name, f.symbol, r.launched_exact)


@pytest.mark.parametrize('dist', X.DISTS)
@pytest.mark.parametrize('form', list(X.FORMS))
def test_x3_form_on_training_like_operands(ops, form, dist):
    f = X.FORMS[form]
    r = X.run_three_ways(ops, f, X.draw(f, dist))
    check_dispatch(f, r)
    figures = []
    for name, y3, y1, yd in zip(r.names, r.x3, r.exact, r.f64):
        assert torch.isfinite(yd).all(), (form, dist, name)
        if dist in ('tiny', 'huge'):       # (util.rel_err floors its denominator at 1e-30)
            assert 1e-20 <= yd.pow(2).mean().sqrt().item() <= 1e20 and yd.abs().max().item() <= 1e20, (form, dist, name)
        e3, e1 = rms_rel(y3, yd), rms_rel(y1, yd)
        figures.append((name, e3, e1))
        print(f'X3OPERANDS {form} {dist} {name}: rms vs float64 x3 {e3:.3e} exact {e1:.3e} ratio {e3 / max(e1, 1e-300):.2f} | '
              f'max-rel x3 vs float64 {rel_err(y3, yd):.2e}, x3 vs exact {rel_err(y3, y1):.2e}, exact vs float64 {rel_err(y1, yd):.2e} | '
              f'launched {r.symbol}')
    for name, y3, y1, yd in zip(r.names, r.x3, r.exact, r.f64):
        assert torch.isfinite(y3).all(), (form, dist, name)
        assert_close(y3, yd, TOL, f'x3 {form} {dist} {name} vs float64')
        assert_close(y3, y1, TOL, f'x3 {form} {dist} {name} vs exact-fp32 kernel')
    # "fp32" means: no further from float64 than the exact-fp32 kernels (rms over the tensor)
    name, e3, e1 = figures[0]
    assert e3 <= (max(1.1 * e1, WGRAD_FLOOR) if f.role == 'wgrad' else 1.1 * e1), (form, dist, name, e3, e1)


def test_x3_layer_tail_near_constant_planes(ops):
    """|mean| / std of every output plane near 30 (a bias of ~30 standard deviations, either sign): the variance is what is left
    of E[y^2] - mean^2 after three digits cancel.  The epilogue sums 16 values per lane in fp32 and goes on in float64; that
    loses about 2^-24 * 30^2 = 5e-5 of the variance, inside TOL.  The split-product tail may be no worse than the exact one."""
    f = X.FORMS['fwd_aff_tail']
    T = X.tail_near_constant_operands(f)
    r = X.run_three_ways(ops, f, T)
    check_dispatch(f, r)
    (y3, m3, r3), (y1, m1, r1), (yd, md, rd) = r.x3, r.exact, r.f64
    ratio = md.abs() * rd
    assert 20.0 <= ratio.min().item() and ratio.max().item() <= 45.0, (ratio.min().item(), ratio.max().item())
    errs = {}
    for name, a3, a1, ad in (('y', y3, y1, yd), ('mean', m3, m1, md), ('rstd', r3, r1, rd)):
        errs[name] = (rel_err(a3, ad), rel_err(a1, ad))
        print(f'X3OPERANDS tail near-constant {name}: max-rel vs float64 x3 {errs[name][0]:.3e} exact {errs[name][1]:.3e} '
              f'(|mean|/std {ratio.min().item():.1f}..{ratio.max().item():.1f})')
    for name, a3, ad in (('y', y3, yd), ('mean', m3, md), ('rstd', r3, rd)):
        assert_close(a3, ad, TOL, f'x3 layer tail, near-constant planes: {name} vs float64')
    for name in ('mean', 'rstd'):
        e3, e1 = errs[name]
        assert e3 <= max(1.1 * e1, 1e-5), (name, e3, e1)


# ---- non-finite values stay where linear algebra puts them ---------------------------------------------------------------------------
# One +inf / NaN in image 0 at a pixel in the last row and column of a tile (16 x 16 pixels; 8 x 16 low-resolution pixels in
# the stride-2 kernels, so (15, 31) of a pooled layer's input), so the halo carries it into the neighbouring tiles.  The
# affected set is where the float64 result of the same input is non-finite.  (The split turns inf into NaN - inf - inf in
# v - h - so the kind of non-finite value is not compared: DESIGN.md section 4.0.)
# form, (N, Cin, Cout, H, W), pixel
NONFINITE = [('fwd', (2, 64, 64, 16, 32), (7, 15)), ('dgrad', (2, 64, 64, 16, 32), (7, 15)),
             ('up_fwd', (2, 64, 64, 16, 32), (7, 15)), ('pool_fwd', (2, 64, 128, 16, 32), (15, 31)),
             ('wgrad', (2, 64, 64, 16, 32), (7, 15)), ('s2_wgrad_pool', (2, 32, 64, 8, 32), (7, 15)),
             ('s2_wgrad_up', (2, 64, 32, 8, 32), (7, 15))]
POISON_CHANNEL = 5


@pytest.mark.parametrize('value', [float('inf'), float('nan')], ids=['inf', 'nan'])
@pytest.mark.parametrize('form,shape,pixel', NONFINITE, ids=[c[0] for c in NONFINITE])
def test_x3_non_finite_stays_where_linear_algebra_puts_it(ops, form, shape, pixel, value):
    f = X.FORMS[form].at(shape)
    clean = X.draw(f, 'randn')
    which = 'gy' if f.role == 'dgrad' else 'x'
    v = getattr(clean, which).clone()
    assert v.shape[2] > pixel[0] and v.shape[3] > pixel[1] + 1
    v[0, POISON_CHANNEL, pixel[0], pixel[1]] = value
    bad = clean._replace(**{which: v})
    ref, = f.ref(f, X.to_f64(bad))
    affected = ~torch.isfinite(ref)
    if f.role == 'wgrad':       # the rows of the poisoned input channel, and nothing else
        want = torch.zeros_like(affected)
        want[:, POISON_CHANNEL] = True
        assert torch.equal(affected, want)
    else:                       # a neighbourhood of the pixel in image 0, in every channel
        assert affected[0].any() and not affected[1].any() and affected.sum().item() < 64 * affected.shape[1]
    (y_clean,), l3 = X.run_x3(ops, f, X.to_gpu(clean))
    assert X.ran(f.symbol, l3), (form, l3)
    (y_bad,), l3 = X.run_x3(ops, f, X.to_gpu(bad))
    assert X.ran(f.symbol, l3), (form, l3)
    y_clean, y_bad = y_clean.cpu(), y_bad.cpu()
    assert torch.isfinite(y_clean).all()
    got = ~torch.isfinite(y_bad)
    print(f'X3OPERANDS non-finite {form} {value}: reference non-finite at {int(affected.sum())} elements, kernel at {int(got.sum())}; '
          f'NaN among them {int(torch.isnan(y_bad).sum())}')
    assert torch.equal(got, affected), (int(got.sum()), int(affected.sum()), int((got ^ affected).sum()))
    assert torch.equal(y_bad[~affected], y_clean[~affected])
