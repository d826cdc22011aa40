"""CPU tests of tests/norm_reference.py, the float64 judge of tests/test_gpu_norm.py: it equals torch's own BatchNorm2d /
LayerNorm in float64 (outputs, first-order gradients, the penalty's second-order gradients, running statistics), every shape
of the GPU tests reaches the launch branch it is listed for, and with a fused activation the float32 evaluation of the
reference agrees with the float64 one on every sign - so the kernel's sign pattern, which the GPU tests hand to the
reference, cannot hide an error that float32 itself would not make."""
import pytest
import torch
import torch.nn.functional as F

import norm_reference as ref
from util import rel_err

F64 = torch.float64
EXACT = 1e-12      # float64 against float64: the same formula in another order of operations


def _torch_bn(x, weight, bias, gy, slope):
    c = x.shape[1]
    bn = torch.nn.BatchNorm2d(c, affine=True).double().train()
    with torch.no_grad():
        bn.weight.copy_(weight.double() if weight is not None else torch.ones(c))
        bn.bias.copy_(bias.double() if bias is not None else torch.zeros(c))
    xl = x.double().clone().requires_grad_(True)
    z = bn(xl)
    y = z if slope is None else F.leaky_relu(z, slope)
    gx, gw, gb = torch.autograd.grad(y, (xl, bn.weight, bn.bias), gy.double())
    return z.detach(), y.detach(), gx, gw, gb


@pytest.mark.parametrize('slope', ref.SLOPES)
@pytest.mark.parametrize('params', ['wb', 'w', 'b', ''])
def test_batch_norm_reference_equals_torch(params, slope):
    shape = (3, 4, 36, 40)
    x, weight, bias, gy = ref.bn_inputs(shape, params, 0.5, 2.0)
    z, y, gx, gw, gb, mean, var = ref.batch_norm_with_grads(x, weight, bias, gy, F64, act_slope=slope)
    tz, ty, tgx, tgw, tgb = _torch_bn(x, weight, bias, gy, slope)
    for nm, a, b in (('z', z, tz), ('y', y, ty), ('gx', gx, tgx), ('gw', gw, tgw), ('gb', gb, tgb)):
        if a is None:
            assert nm[1] not in params
            continue
        assert rel_err(a, b) <= EXACT, nm
    assert rel_err(mean, x.double().mean(dim=(0, 2, 3))) <= EXACT
    assert rel_err(var, x.double().var(dim=(0, 2, 3), unbiased=False)) <= EXACT
    assert z.dtype == F64 and ref.batch_norm_with_grads(x, weight, bias, gy, torch.float32)[0].dtype == torch.float32


@pytest.mark.parametrize('momentum', [0.1, 0.3])
def test_running_update_and_eval_equal_torch(momentum):
    shape = (5, 6, 9, 11)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(*shape, generator=g) * (1 + i) + 0.5 * i for i in range(3)]
    bn = torch.nn.BatchNorm2d(6, momentum=momentum).double().train()
    for x in xs:
        bn(x.double())
    rm, rv, cnt = ref.running_update(xs, momentum, F64)
    assert cnt == int(bn.num_batches_tracked) == 3
    assert rel_err(rm, bn.running_mean) <= EXACT and rel_err(rv, bn.running_var) <= EXACT
    _, weight, bias, _ = ref.bn_inputs(shape, 'wb', 0.5, 2.0)
    bn.eval()
    with torch.no_grad():
        bn.weight.copy_(weight.double())
        bn.bias.copy_(bias.double())
    for slope in ref.SLOPES:
        want = bn(xs[0].double()) if slope is None else F.leaky_relu(bn(xs[0].double()), slope)
        got = ref.batch_norm_eval(xs[0], weight, bias, rm, rv, bn.eps, F64, act_slope=slope)
        assert rel_err(got, want) <= EXACT, slope
    plain = ref.batch_norm_eval(xs[0], None, None, rm, rv, bn.eps, F64)
    assert rel_err(plain, F.batch_norm(xs[0].double(), rm, rv, None, None, False, 0.0, bn.eps)) <= EXACT


def _torch_ln(x, weight, bias, cot, w2, slope, functional):
    m = x.shape[1]
    xl = x.double().clone().requires_grad_(True)
    leaves = [xl]
    if functional:
        wl = weight.double().clone().requires_grad_(True) if weight is not None else None
        bl = bias.double().clone().requires_grad_(True) if bias is not None else None
        leaves += [t for t in (wl, bl) if t is not None]
        z = F.layer_norm(xl, (m,), wl, bl, ref.EPS)
    else:
        ln = torch.nn.LayerNorm(m, eps=ref.EPS).double()
        with torch.no_grad():
            ln.weight.copy_(weight.double())
            ln.bias.copy_(bias.double())
        leaves += [ln.weight, ln.bias]
        z = ln(xl)
    y = z if slope is None else F.leaky_relu(z, slope)
    out = (y * cot.double()).sum()
    gx, = torch.autograd.grad(out, xl, create_graph=True)
    pen = ((gx * w2.double()) ** 2).sum() + out
    return (z.detach(), y.detach(), gx.detach()) + tuple(torch.autograd.grad(pen, leaves))


@pytest.mark.parametrize('slope', ref.SLOPES)
@pytest.mark.parametrize('params', ['wb', 'w', ''])
def test_layer_norm_reference_equals_torch(params, slope):
    shape = (3, 4101)
    x, weight, bias, cot, w2 = ref.ln_inputs(shape, params, 0.2, 1.5)
    got = ref.layer_norm_with_grads(x, weight, bias, cot, w2, F64, act_slope=slope)
    wants = [_torch_ln(x, weight, bias, cot, w2, slope, True)]
    if params == 'wb':
        wants.append(_torch_ln(x, weight, bias, cot, w2, slope, False))        # nn.LayerNorm as well
    assert len(got) == 4 + len(params)           # gradients of absent parameters are left out
    for want in wants:
        assert len(want) == len(got)
        for nm, a, b in zip(('z', 'y', 'gx', 'd pen/dx', 'd pen/d p1', 'd pen/d p2'), got, want):
            assert rel_err(a, b) <= EXACT, nm


def test_given_mask_replaces_the_references_own_sign():
    x, weight, bias, gy = ref.bn_inputs((5, 6, 9, 11), 'wb', 0.5, 2.0)
    z, y, gx = ref.batch_norm_with_grads(x, weight, bias, gy, F64, act_slope=0.2)[:3]
    same = ref.batch_norm_with_grads(x, weight, bias, gy, F64, act_slope=0.2, mask=z > 0)
    assert torch.equal(same[1], y) and torch.equal(same[2], gx)
    flipped = ref.batch_norm_with_grads(x, weight, bias, gy, F64, act_slope=0.2, mask=torch.zeros_like(z, dtype=torch.bool))
    assert torch.equal(flipped[1], z * 0.2)


# ---- which branch each GPU shape reaches --------------------------------------------------------------------------------------
def test_batch_norm_shapes_reach_their_branches():
    plan = {s: ref.rowsum_plan(s[0] * s[2] * s[3]) for s in ref.BN_SHAPES}
    assert plan == ref.BN_SHAPES
    facts = {}
    for (n, c, h, w), (S, length) in plan.items():
        hw, L = h * w, n * h * w
        facts[(n, c, h, w)] = dict(ragged=L % length != 0, cuts_segments=length % hw != 0 and S > 1, scalar=hw % 4 != 0,
                                   apply2=ref.second_pass(n * c * hw // 4 if hw % 4 == 0 else n * c * hw),
                                   project2=ref.second_pass(n * c * hw))
    f = facts[(5, 6, 9, 11)]
    assert plan[(5, 6, 9, 11)][0] == 1 and f['scalar'] and not f['apply2']
    f = facts[(8, 3, 32, 32)]                     # two full slices, each four whole segments
    assert plan[(8, 3, 32, 32)] == (2, 4 * 32 * 32) and not f['ragged'] and not f['cuts_segments'] and not f['scalar']
    f = facts[(3, 4, 36, 40)]
    assert plan[(3, 4, 36, 40)][0] == 2 and f['ragged'] and f['cuts_segments'] and not f['scalar']
    f = facts[(4, 8, 264, 260)]                   # the cap: ceil(L / 4096) > 64, so len > 4096
    assert -(-4 * 264 * 260 // 4096) > ref.ROWSUM_MAX_SPLIT and plan[(4, 8, 264, 260)] == (64, 4352)
    assert f['cuts_segments'] and not f['scalar'] and f['apply2'] and f['project2']
    f = facts[(3, 2, 295, 297)]
    assert f['scalar'] and f['apply2'] and f['project2'] and plan[(3, 2, 295, 297)][1] > 4096 and f['cuts_segments']
    assert 3 * 2 * 295 * 297 > 524288
    assert plan[(1, 4, 4, 4)][0] == 1
    for s in ((8, 3, 32, 32), (3, 4, 36, 40)):    # the operand combinations run where the rows are split
        assert {p for sh, p, _, _ in ref.BN_CASES if sh == s} == {'wb', 'w', 'b', ''}


def test_layer_norm_shapes_reach_their_branches():
    got = {s: (ref.row_stats_regime(s[1]), ref.row_stats_chunks(s[1]), ref.rowsum_plan(s[1])) for s in ref.LN_SHAPES}
    assert got == ref.LN_SHAPES
    regimes = [v[0] for v in got.values()]
    assert {'wave64', 'block256', 'chunked'} == set(regimes)
    assert got[(5, 1028)][0] == 'block256' and 1028 % 4 == 0 and 1028 >= 1024          # vector loads, >= 1024 template
    assert got[(4, 1020)][0] == 'wave64' and 1020 % 4 == 0 and 1020 < 1024
    assert 4101 % 4 != 0 and got[(3, 4101)][2][0] == 2 and 4101 % got[(3, 4101)][2][1] != 0   # scalar loads; ragged slice
    assert got[(2, 8192)][1] == 1 and got[(2, 8196)][1] == 2                           # either side of the chunk threshold
    assert 8192 == 2 * got[(2, 8192)][2][1]                                            # two full row-sum slices
    assert got[(2, 269120)][1] == 33 and got[(2, 269120)][2][1] == 4352 and -(-269120 // 4096) > 64
    assert ref.second_pass(2 * 269120) and 2 * 269120 > 524288
    assert got[(1, 528392)][1] == 64 and -(-(528392 // 4) // 2048) > 64 and got[(1, 528392)][2][1] == 8448
    assert ref.second_pass(528392)
    for s in ((3, 4101), (2, 8192)):
        assert {p for sh, p, _, _ in ref.LN_CASES if sh == s} == {'wb', 'w', ''}


# ---- float32 and float64 agree on every sign of the pre-activation ------------------------------------------------------------
@pytest.mark.parametrize('case', ref.BN_CASES, ids=ref.case_id)
def test_batch_norm_float32_has_no_sign_flip(case):
    x, weight, bias, gy = ref.bn_inputs(*case)
    z64 = ref.batch_norm_with_grads(x, weight, bias, gy, F64)[0]
    z32 = ref.batch_norm_with_grads(x, weight, bias, gy, torch.float32)[0]
    assert int(((z32 > 0) != (z64 > 0)).sum()) == 0


@pytest.mark.parametrize('case', ref.LN_CASES, ids=ref.case_id)
def test_layer_norm_float32_has_no_sign_flip(case):
    x, weight, bias, cot, w2 = ref.ln_inputs(*case)
    z64 = ref.layer_norm_with_grads(x, weight, bias, cot, w2, F64)[0]
    z32 = ref.layer_norm_with_grads(x, weight, bias, cot, w2, torch.float32)[0]
    assert int(((z32 > 0) != (z64 > 0)).sum()) == 0
