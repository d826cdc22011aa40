"""The exact-fp32 convolution kernels by name against float64 (tests/exact_forms.py: one row per kernel per edge).

Every row, on ``randn`` operands with the split-product kernels off:
  * the launches contain the row's kernel symbol, and every (symbol, workgroups) pair of the row's restated plan in order -
    the grid is what proves that the geometry reached the edge the row is for;
  * every output is within TOL = 2e-4 of float64 (max error over the tensor's maximum, ``util.assert_close``);
  * the rms error against float64 is at most ``row.factor`` (2) x that of fp32 ATen on the CPU - the layer's definition run in
    fp32 on the same operands; weight gradients: or x3_forms.WGRAD_FLOOR.  The factor allows a sequential fp32 chain over
    9 * Cin terms against ATen's blocked sums.  InstanceNorm mean / rstd of the tail forms take the TOL bar only: a few hundred
    numbers at the rounding of their own fp32 result, where a ratio of two such errors says nothing
    (tests/test_gpu_x3_operands.py).
The rows marked ``dists`` - one per kernel, its most edge-laden geometry - run again under every distribution of
x3_forms.DISTS at the same bars.  One +inf / NaN: tests/test_gpu_x3_operands.py's test of the same name, on the exact kernels.
Measured worst ratios per kernel: DESIGN.md section 4.0."""
import pytest
import torch

import exact_forms as E
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


def run_gpu(ops, f, T):
    """E.run; a HIP error ends the whole session - nothing more is started on a device that has faulted"""
    try:
        return E.run(ops, f, T)
    except RuntimeError as e:
        if 'HIP' in str(e) or 'hip' in str(e):
            pytest.exit(f'{f.name}: {e}', returncode=3)
        raise


def check_row(ops, name, dist):
    f = E.ROWS[name]
    T = X.draw(f, dist)
    got, launches = run_gpu(ops, f, T)
    print(f'EXACT {name} {dist}: launched {launches}')
    assert any(E.norm(f.symbol) in k for k, _ in launches), (name, f.symbol, launches)
    assert E.plan_found(f.plan, launches), (name, f.plan, launches)
    want = tuple(v.detach() for v in f.ref(f, X.to_f64(T)))
    aten = tuple(v.detach() for v in f.define(f, T))
    figures = []
    for out, y, yd, ya in zip(f.outs, got, want, aten):
        assert ya.dtype == torch.float32 and torch.isfinite(yd).all(), (name, dist, out)
        if dist in ('tiny', 'huge'):       # (util.rel_err floors its denominator at 1e-30)
            assert 1e-20 <= yd.pow(2).mean().sqrt().item() <= 1e20 and yd.abs().max().item() <= 1e20, (name, dist, out)
        ek, ea = rms_rel(y, yd), rms_rel(ya, yd)
        figures.append((out, ek, ea))
        print(f'EXACT {name} {dist} {out}: rms vs float64 kernel {ek:.3e} ATen {ea:.3e} ratio {ek / max(ea, 1e-300):.2f} | '
              f'max-rel vs float64 {rel_err(y, yd):.2e} | launched {f.symbol}')
    for out, y, yd in zip(f.outs, got, want):
        assert torch.isfinite(y).all(), (name, dist, out)
        assert_close(y, yd, TOL, f'{name} {dist} {out} vs float64')
    for out, ek, ea in figures:
        if out in ('mean', 'rstd'):
            continue
        bar = max(f.factor * ea, WGRAD_FLOOR) if f.role == 'wgrad' else f.factor * ea
        assert ek <= bar, (name, dist, out, ek, ea, f.factor)


@pytest.mark.parametrize('name', list(E.ROWS))
def test_exact_kernel_row(ops, name):
    check_row(ops, name, 'randn')


@pytest.mark.parametrize('dist', X.DISTS)
@pytest.mark.parametrize('name', [n for n, r in E.ROWS.items() if r.dists])
def test_exact_kernel_on_training_like_operands(ops, name, dist):
    check_row(ops, name, dist)


# ---- non-finite values stay where linear algebra puts them ---------------------------------------------------------------------------
# One +inf / NaN in image 0 of the streamed operand (gy of an input gradient, else x), at a pixel in the last row and column of
# a tile, so the halo carries it into the neighbouring tiles.  The affected SET is where the float64 result of the same operands
# is non-finite; the kind is not compared - a folded 4x4 stride-2 kernel sums weights before it multiplies, so inf - inf turns
# up at other places than in the composed reference.
POISON_CHANNEL = 1


@pytest.mark.parametrize('value', [float('inf'), float('nan')], ids=['inf', 'nan'])
@pytest.mark.parametrize('name,pixel', E.NONFINITE, ids=[c[0] for c in E.NONFINITE])
def test_exact_non_finite_stays_where_linear_algebra_puts_it(ops, name, pixel, value):
    f = E.ROWS[name]
    clean = X.draw(f, 'randn')
    which = 'gy' if f.role == 'dgrad' else 'x'
    v = getattr(clean, which).clone()
    assert v.shape[0] >= 2 and v.shape[2] > pixel[0] and v.shape[3] > pixel[1]
    v[0, POISON_CHANNEL, pixel[0], pixel[1]] = value
    bad = clean._replace(**{which: v})
    ref, = f.ref(f, X.to_f64(bad))
    affected = ~torch.isfinite(ref)
    if f.role == 'wgrad':       # the rows of the poisoned input channel, and nothing else
        want = torch.zeros_like(affected)
        want[:, POISON_CHANNEL] = True
        assert torch.equal(affected, want)
    else:                       # a neighbourhood of the pixel in image 0, in every channel
        assert affected[0].any() and not affected[1:].any() and affected.sum().item() <= 64 * affected.shape[1]
    (y_clean,), l0 = run_gpu(ops, f, clean)
    (y_bad,), l1 = run_gpu(ops, f, bad)
    assert E.plan_found(f.plan, l0) and E.plan_found(f.plan, l1), (name, l0, l1)
    assert torch.isfinite(y_clean).all()
    got = ~torch.isfinite(y_bad)
    print(f'EXACT non-finite {name} {value}: reference non-finite at {int(affected.sum())} elements, kernel at {int(got.sum())}; '
          f'NaN among them {int(torch.isnan(y_bad).sum())} | launched {f.symbol}')
    assert torch.equal(got, affected), (int(got.sum()), int(affected.sum()), int((got ^ affected).sum()))
    if f.role != 'wgrad':
        assert torch.isfinite(y_bad[1:]).all()
    assert torch.equal(y_bad[~affected], y_clean[~affected])
