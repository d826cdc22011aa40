"""GPU tests of the normalisation kernels (csrc/norm.hip, the row statistics of csrc/pointwise.hip) through ``ops.batch_norm``
/ ``ops.layer_norm`` and through the C ABI, at the shapes where the launch code splits: several row-sum slices (full, ragged,
across BatchNorm's segment boundaries, at the cap of 64), a second pass of the element-wise grid-stride loops, the scalar
BatchNorm apply, the three regimes of the row statistics, absent operands.  tests/test_norm_host.py proves which branch each
shape reaches.

Bound, per tensor (the rule of tests/test_gpu_cond.py): ``rel_err(gpu, float64) <= max(1e-5, 16 * e_cpu)`` with ``e_cpu`` the
error of norm_reference.py evaluated in float32 on the CPU against its own float64 run on the same inputs.

Fused activation: the reference's gradients are formed with the kernel's own sign pattern (``y_gpu > 0``), under the condition
that at most 2 elements per case disagree with the float64 sign and that each of them has ``|z64| <= bound * max|z64|``
(``bound``: the forward bound).  The float32 reference itself has no disagreement (test_norm_host.py), so the mask cannot hide
an error of the kernels.

Every test prints ``norm | case | tensor | e | e_cpu`` before it asserts; DESIGN.md 4.18 holds the largest e / e_cpu seen.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import norm_reference as ref
from util import rel_err

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
BN_NAMES = ('y', 'gx', 'gw', 'gb', 'mean', 'var')
LN_NAMES = ('y', 'gx', 'dpen/dx', 'dpen/dp1', 'dpen/dp2')
BN_BY_ID = {ref.case_id(c): c for c in ref.BN_CASES}
LN_BY_ID = {ref.case_id(c): c for c in ref.LN_CASES}


def _limit(c):
    return max(1e-5, 16 * c)


def _judge(tag, names, got, want, cpu):
    """Print e / e_cpu of every tensor, then assert the bound; an absent gradient is absent on both sides."""
    rows = []
    for nm, a, b, c in zip(names, got, want, cpu):
        if b is None:
            assert a is None, f'{tag} {nm}: a gradient without its parameter'
            continue
        assert a is not None and tuple(a.shape) == tuple(b.shape), f'{tag} {nm}'
        rows.append((nm, rel_err(a, b), rel_err(c, b)))
    for nm, e, c in rows:
        print(f'norm | {tag} | {nm} | {e:.2e} | {c:.2e}')
    for nm, e, c in rows:
        assert e <= _limit(c), f'{tag} {nm}: {e:.3e} > max(1e-5, 16 * {c:.3e})'


def _sign_condition(tag, y_gpu, z64, z32):
    """The condition that goes with the kernel's mask: few disagreements, each at a pre-activation within the forward bound."""
    mask = y_gpu.cpu() > 0
    flips = mask != (z64 > 0)
    n = int(flips.sum())
    worst = float(z64[flips].abs().max()) if n else 0.0
    allowed = _limit(rel_err(z32, z64)) * float(z64.abs().max())
    print(f'norm | {tag} | sign flips {n} | worst |z64| {worst:.2e} | allowed {allowed:.2e}')
    assert n <= 2, f'{tag}: {n} signs differ from float64'
    assert worst <= allowed, f'{tag}: a sign differs at |z64| = {worst:.3e} > {allowed:.3e}'
    return mask


def _offset_view(t):
    """A contiguous CUDA copy of ``t`` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_case(case):
    """Inputs (CPU fp32) and the reference without activation in float64 and float32; computed once, never modified."""
    inputs = ref.bn_inputs(*case)
    return inputs, ref.batch_norm_with_grads(*inputs, F64), ref.batch_norm_with_grads(*inputs, F32)


def _bn_gpu(x, weight, bias, gy, slope, buffers=True, input_grad_only=False, offset=False):
    from gan_lab_amd import ops
    place = _offset_view if offset else (lambda t: t.cuda())
    xg, gyg = place(x).requires_grad_(True), place(gy)
    wg, bg = (t.cuda().requires_grad_(True) if t is not None else None for t in (weight, bias))
    c = x.shape[1]
    rm, rv, cnt = (torch.zeros(c).cuda(), torch.ones(c).cuda(), torch.zeros((), dtype=torch.int64).cuda()) if buffers \
        else (None, None, None)
    y, mean, var = ops._BatchNormTrain.apply(xg, wg, bg, ref.EPS, rm, rv, 0.1, cnt, slope)
    leaves = [t for t in (xg, wg, bg) if t is not None]
    if input_grad_only:
        with ops.input_grad_only():
            grads = list(torch.autograd.grad(y, leaves, gyg, allow_unused=True))
    else:
        grads = list(torch.autograd.grad(y, leaves, gyg))
    gx = grads.pop(0)
    gw = grads.pop(0) if weight is not None else None
    gb = grads.pop(0) if bias is not None else None
    return y.detach(), gx, gw, gb, mean, var


def _bn_reference(case, slope, y_gpu):
    """(want, cpu) for the GPU result ``y_gpu``: the cached pair, or with a fused activation the pair under the kernel's mask."""
    inputs, want, cpu = _bn_case(case)
    if slope is None:
        return want, cpu
    mask = _sign_condition(f'bn {ref.case_id(case)} slope {slope}', y_gpu, want[0], cpu[0])
    return (ref.batch_norm_with_grads(*inputs, F64, act_slope=slope, mask=mask),
            ref.batch_norm_with_grads(*inputs, F32, act_slope=slope, mask=mask))


@pytest.mark.parametrize('slope', ref.SLOPES)
@pytest.mark.parametrize('case', ref.BN_CASES, ids=ref.case_id)
def test_batch_norm_against_float64(case, slope):
    inputs = _bn_case(case)[0]
    got = _bn_gpu(*inputs, slope)
    want, cpu = _bn_reference(case, slope, got[0])
    _judge(f'bn {ref.case_id(case)} slope {slope}', BN_NAMES, got, want[1:], cpu[1:])


@pytest.mark.parametrize('slope', [None, 0.2])
@pytest.mark.parametrize('cid', ['8x3x32x32-wb', '3x2x295x297-wb'])
def test_batch_norm_input_gradient_only(cid, slope):
    """Under ops.input_grad_only() the parameter gradients are absent and gx is the same, bit for bit."""
    inputs = _bn_case(BN_BY_ID[cid])[0]
    full = _bn_gpu(*inputs, slope)
    only = _bn_gpu(*inputs, slope, input_grad_only=True)
    assert only[2] is None and only[3] is None and full[2] is not None and full[3] is not None
    assert torch.equal(only[1], full[1]) and torch.equal(only[0], full[0])


def _bn_eval_gpu(x, weight, bias, gy, rm, rv, slope, offset=False, **kw):
    """Eval-mode (y, gx, gw, gb) on the GPU; ``offset``: x and the cotangent as views 4 bytes past a 16-byte boundary."""
    from gan_lab_amd import ops
    place = _offset_view if offset else (lambda t: t.cuda())
    xg, wg, bg = place(x).requires_grad_(True), weight.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    yg = ops.batch_norm(xg, wg, bg, rm, rv, False, eps=ref.EPS, act_slope=slope, **kw)
    return (yg.detach(),) + torch.autograd.grad(yg, (xg, wg, bg), place(gy))


def _bn_eval_reference(tag, x, weight, bias, gy, rm, rv, slope, y_gpu):
    """(want, cpu): eval-mode (y, gx, gw, gb) of the reference in float64 / float32, under the kernel's mask when fused."""
    pre = [ref.batch_norm_eval(x, weight, bias, rm, rv, ref.EPS, dt) for dt in (F64, F32)]
    mask = None if slope is None else _sign_condition(tag, y_gpu, *pre)
    res = []
    for dt in (F64, F32):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in (x, weight, bias)]
        yr = ref.batch_norm_eval(*leaves, rm, rv, ref.EPS, dt, act_slope=slope, mask=mask)
        res.append((yr.detach(),) + torch.autograd.grad(yr, leaves, gy.to(dt)))
    return res


@pytest.mark.parametrize('momentum', [0.1, 0.3])
@pytest.mark.parametrize('shape', [(8, 3, 32, 32), (5, 6, 9, 11)], ids=['8x3x32x32', '5x6x9x11'])
def test_batch_norm_running_statistics_and_eval(shape, momentum):
    from gan_lab_amd import ops
    tag = f'bn state {"x".join(map(str, shape))} momentum {momentum}'
    x0, weight, bias, gy = _bn_case((shape, 'wb', 0.5, 2.0))[0]
    g = torch.Generator().manual_seed(11)
    xs = [x0] + [torch.randn(*shape, generator=g) * (0.7 + i) - 0.4 * i for i in (1, 2)]
    c = shape[1]
    rm, rv, cnt = torch.zeros(c).cuda(), torch.ones(c).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    for x in xs:
        y = ops.batch_norm(x.cuda(), weight.cuda(), bias.cuda(), rm, rv, True, momentum=momentum, eps=ref.EPS, batches=cnt)
    none = ops.batch_norm(xs[-1].cuda(), weight.cuda(), bias.cuda(), None, None, True, momentum=momentum, eps=ref.EPS)
    assert torch.equal(none, y)                      # no buffers, no counter: the same training output
    want, cpu = ref.running_update(xs, momentum, F64), ref.running_update(xs, momentum, F32)
    assert int(cnt) == want[2] == 3
    _judge(tag, ('running_mean', 'running_var'), (rm, rv), want[:2], cpu[:2])
    # eval mode: the running statistics as constants, buffers and counter untouched
    before = rm.clone(), rv.clone()
    for slope in ref.SLOPES:
        got = _bn_eval_gpu(x0, weight, bias, gy, rm, rv, slope, momentum=momentum, batches=cnt)
        res = _bn_eval_reference(f'{tag} eval slope {slope}', x0, weight, bias, gy, rm, rv, slope, got[0])
        _judge(f'{tag} eval slope {slope}', ('y', 'gx', 'gw', 'gb'), got, *res)
    plain = ops.batch_norm(x0.cuda(), None, None, rm, rv, False, eps=ref.EPS)
    _judge(f'{tag} eval no affine', ('y',), (plain,), *[(ref.batch_norm_eval(x0, None, None, rm, rv, ref.EPS, dt),)
                                                         for dt in (F64, F32)])
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and int(cnt) == 3


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_case(case):
    inputs = ref.ln_inputs(*case)
    return inputs, ref.layer_norm_with_grads(*inputs, F64), ref.layer_norm_with_grads(*inputs, F32)


def _ln_gpu(x, weight, bias, cot, w2, slope, input_grad_only=False, offset=False):
    """First and second order on the GPU: (y, gx, d pen/dx[, d pen/dw][, d pen/db]) of norm_reference's penalty."""
    from gan_lab_amd import ops
    place = _offset_view if offset else (lambda t: t.cuda())
    xg, cg, w2g = place(x).requires_grad_(True), place(cot), place(w2)
    leaves = [xg] + [t.cuda().requires_grad_(True) for t in (weight, bias) if t is not None]
    wg = leaves[1] if weight is not None else None
    bg = leaves[-1] if bias is not None else None
    y = ops.layer_norm(xg, wg, bg, eps=ref.EPS, act_slope=slope)
    out = (y * cg).sum()
    if input_grad_only:                              # the gradient-penalty pass of the learner: ln_project instead of ln_bwd_cols
        with ops.input_grad_only():
            gx, = torch.autograd.grad(out, xg, create_graph=True)
    else:
        gx, = torch.autograd.grad(out, xg, create_graph=True)
    pen = ((gx * w2g) ** 2).sum() + out
    return (y.detach(), gx.detach()) + torch.autograd.grad(pen, leaves)


def _ln_reference(case, slope, y_gpu):
    inputs, want, cpu = _ln_case(case)
    if slope is None:
        return want, cpu
    mask = _sign_condition(f'ln {ref.case_id(case)} slope {slope}', y_gpu, want[0], cpu[0])
    return (ref.layer_norm_with_grads(*inputs, F64, act_slope=slope, mask=mask),
            ref.layer_norm_with_grads(*inputs, F32, act_slope=slope, mask=mask))


@pytest.mark.parametrize('slope', ref.SLOPES)
@pytest.mark.parametrize('case', ref.LN_CASES, ids=ref.case_id)
def test_layer_norm_first_and_second_order_against_float64(case, slope):
    inputs = _ln_case(case)[0]
    got = _ln_gpu(*inputs, slope)
    want, cpu = _ln_reference(case, slope, got[0])
    assert len(got) == len(want) - 1 == 3 + len(case[1])
    _judge(f'ln {ref.case_id(case)} slope {slope}', LN_NAMES, got, want[1:], cpu[1:])


@pytest.mark.parametrize('slope', [None, 0.2])
@pytest.mark.parametrize('cid', ['3x4101-wb', '2x269120-wb'])
def test_layer_norm_penalty_pass_without_parameter_gradients(cid, slope):
    """ops.input_grad_only() around the differentiable first backward, as the learner's gradient penalty runs it: the input
    gradient comes from ln_project with the weight folded in, and every result stays within the same bound."""
    case = LN_BY_ID[cid]
    inputs = _ln_case(case)[0]
    got = _ln_gpu(*inputs, slope, input_grad_only=True)
    want, cpu = _ln_reference(case, slope, got[0])
    assert len(got) == len(want) - 1 == 3 + len(case[1])
    _judge(f'ln {cid} slope {slope} input-grad-only', LN_NAMES, got, want[1:], cpu[1:])


def test_layer_norm_of_one_element_rows():
    """M = 1: x equals its mean, so y = bias exactly and the input gradient is exactly zero."""
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(4, 1, generator=g) * 3 + 1).cuda().requires_grad_(True)
    w = (torch.randn(1, generator=g) + 2).cuda().requires_grad_(True)
    b = torch.randn(1, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(4, 1, generator=g).cuda()
    y = ops.layer_norm(x, w, b)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), cot)
    print(f'norm | ln 4x1 | max |gx| {float(gx.abs().max()):.2e} | gw {float(gw):.2e}')
    assert torch.equal(y, b.detach().expand(4, 1))
    assert torch.equal(gx, torch.zeros_like(gx))
    assert float(gw) == 0.0
    # gb: four float32 additions, each within 2^-24 of the running sum
    assert abs(float(gb) - float(cot.double().sum())) <= 4 * 2.0 ** -24 * float(cot.double().abs().sum())


# ---- determinism, offset views ------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    """norm.hip promises fixed-order reductions: at the largest cases two runs on the same inputs agree in every output."""
    bn = _bn_case(BN_BY_ID['4x8x264x260-wb'])[0]
    ln = _ln_case(LN_BY_ID['2x269120-wb'])[0]
    for run, inputs in ((_bn_gpu, bn), (_ln_gpu, ln)):
        for slope in (None, 0.2):
            a, b = run(*inputs, slope), run(*inputs, slope)
            assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b)), (run.__name__, slope)


@pytest.mark.parametrize('slope', [None, 0.2])
def test_offset_views_take_the_scalar_paths(slope):
    """x, the cotangent and w2 contiguous but 4 bytes past a 16-byte boundary: the host functions must keep such a tensor away
    from every float4 access (bn_apply, the row statistics, the per-channel affine, sums and activation backward of eval
    mode) - the same bounds, and the results of the aligned run.  Where the two runs reduce in a different order (row
    statistics and channel sums: float4 loads add (a + b) + (c + d), scalar loads add in sequence) the equality rests on the
    fp64 partial sums, whose difference is ~1e-16 relative and disappears in the rounding to float32 - not on identical
    arithmetic."""
    case = BN_BY_ID['8x3x32x32-wb']
    inputs = _bn_case(case)[0]
    got, aligned = _bn_gpu(*inputs, slope, offset=True), _bn_gpu(*inputs, slope)
    want, cpu = _bn_reference(case, slope, got[0])
    _judge(f'bn offset view slope {slope}', BN_NAMES, got, want[1:], cpu[1:])
    assert all(torch.equal(p, q) for p, q in zip(got, aligned))
    # eval mode, forward and gradients: chan_affine on the offset x, and on the offset cotangent chan_affine, channel_sum
    # (gw, gb) and - with an activation - act_bwd
    from gan_lab_amd import ops
    x, weight, bias, gy = inputs
    rm, rv = (x.mean(dim=(0, 2, 3)) * 0.9).cuda(), (x.var(dim=(0, 2, 3)) * 1.1).cuda()
    got, aligned = (_bn_eval_gpu(x, weight, bias, gy, rm, rv, slope, offset=o) for o in (True, False))
    res = _bn_eval_reference(f'bn eval offset view slope {slope}', x, weight, bias, gy, rm, rv, slope, got[0])
    _judge(f'bn eval offset view slope {slope}', ('y', 'gx', 'gw', 'gb'), got, *res)
    assert all(torch.equal(p, q) for p, q in zip(got, aligned))
    # bias_act itself on an offset view (in batch_norm its input is always a fresh allocation)
    ba = [ops.bias_act(xe, bias.cuda(), act='lrelu', slope=0.2 if slope is None else slope) for xe in (_offset_view(x), x.cuda())]
    assert torch.equal(ba[0], ba[1])
    want_ba = torch.nn.functional.leaky_relu(x.double() + bias.double().view(1, -1, 1, 1), 0.2 if slope is None else slope)
    assert rel_err(ba[0], want_ba) <= 1e-5
    case = LN_BY_ID['2x8192-wb']
    inputs = _ln_case(case)[0]
    got, aligned = _ln_gpu(*inputs, slope, offset=True), _ln_gpu(*inputs, slope)
    want, cpu = _ln_reference(case, slope, got[0])
    _judge(f'ln offset view slope {slope}', LN_NAMES, got, want[1:], cpu[1:])
    assert all(torch.equal(p, q) for p, q in zip(got, aligned))
    # a row long enough for the chunked statistics: the misaligned row falls back to one block per row
    case = LN_BY_ID['2x8196-wb']
    inputs = _ln_case(case)[0]
    got = _ln_gpu(*inputs, slope, offset=True)
    want, cpu = _ln_reference(case, slope, got[0])
    _judge(f'ln offset view 2x8196 slope {slope}', LN_NAMES, got, want[1:], cpu[1:])


# ---- the C ABI directly: branches that ops never selects ----------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@functools.lru_cache(maxsize=None)
def _abi_operands():
    """(3, 4101) operands as float64 numpy arrays whose values are float32 numbers."""
    n, m = 3, 4101
    r = np.random.RandomState(7)
    r32 = lambda v: v.astype(np.float32).astype(np.float64)               # noqa: E731
    x = r32(r.randn(n, m) * 1.5 + 0.2)
    mean, rstd = r32(x.mean(1)), r32(1.0 / np.sqrt(x.var(1) + ref.EPS))
    return dict(a=r32(r.randn(n, m)), x=x, mean=mean, rstd=rstd, w=r32(r.randn(m) * 0.3 + 1.0),
                wo=r32(r.randn(m) * 0.3 + 1.0), sums=r32(r.randn(n, 3) * 50.0))


def _abi_formulas(o, dt):
    """The five operations in numpy at dtype ``dt``."""
    a, x, mean, rstd, w, wo, sums = (o[k].astype(dt) for k in ('a', 'x', 'mean', 'rstd', 'w', 'wo', 'sums'))
    m = dt(x.shape[1])
    xhat = (x - mean[:, None]) * rstd[:, None]
    return dict(
        coldot_stats=(a * xhat).sum(0), coldot_o2=a.sum(0), coldot_plain=(a * x).sum(0),
        project=wo * rstd[:, None] * (a * w - sums[:, :1] / m - xhat * sums[:, 1:2] / m),
        colscale=a * w, affine=xhat * w)


def test_c_abi_branches_against_float64():
    from gan_lab_amd import _lib
    L = _lib.lib()
    o = _abi_operands()
    n, m = o['x'].shape
    d = {k: torch.from_numpy(v).float().cuda() for k, v in o.items()}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    new = lambda *s: torch.full(s, float('nan'), device='cuda')            # noqa: E731
    got = dict(coldot_stats=new(m), coldot_o2=new(m), coldot_plain=new(m), project=new(n, m), colscale=new(n, m),
               affine=new(n, m))
    rcs = [
        L.ganlab_coldot_f32(_ptr(d['a']), _ptr(d['x']), _ptr(d['mean']), _ptr(d['rstd']), _ptr(got['coldot_stats']),
                            _ptr(got['coldot_o2']), n, m, st),
        L.ganlab_coldot_f32(_ptr(d['a']), _ptr(d['x']), None, None, _ptr(got['coldot_plain']), None, n, m, st),
        L.ganlab_ln_project_f32(_ptr(d['a']), _ptr(d['w']), _ptr(d['x']), _ptr(d['mean']), _ptr(d['rstd']), _ptr(d['sums']),
                                _ptr(d['wo']), _ptr(got['project']), n, m, st),
        L.ganlab_colscale_f32(_ptr(d['a']), _ptr(d['w']), _ptr(got['colscale']), n, m, st),
        L.ganlab_ln_affine_fwd_f32(_ptr(d['x']), _ptr(d['mean']), _ptr(d['rstd']), _ptr(d['w']), None, _ptr(got['affine']), n, m,
                                   _lib.ACT_NONE, 1.0, st)]
    assert rcs == [0] * 5, rcs
    want, cpu = _abi_formulas(o, np.float64), _abi_formulas(o, np.float32)
    names = sorted(want)
    _judge('abi 3x4101', names, [got[k] for k in names], [torch.from_numpy(want[k]) for k in names],
           [torch.from_numpy(cpu[k]) for k in names])


def test_c_abi_argument_checks_launch_nothing():
    from gan_lab_amd import _lib
    L = _lib.lib()
    EINVAL, EWORKSPACE = -1, -2
    n, m = 3, 4101
    x = torch.randn(n, m).cuda()
    a, mean, rstd = torch.randn(n, m).cuda(), torch.zeros(n).cuda(), torch.ones(n).cuda()
    out, o1 = torch.zeros(n, 3).cuda(), torch.zeros(m).cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    count = L.ganlab_launch_count()
    need = L.ganlab_ln_rowsums_workspace(n, m)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64).cuda()
    assert need > 0
    assert L.ganlab_ln_rowsums_f32(_ptr(a), None, _ptr(x), _ptr(mean), _ptr(rstd), None, None, _ptr(out), n, m, _ptr(ws), need - 1,
                                   None, None, 1.0, st) == EWORKSPACE
    x4 = torch.randn(2, 3, 8, 8).cuda()
    need = L.ganlab_ln_rowsums_workspace(3, 2 * 64)
    assert L.ganlab_bn_stats_f32(_ptr(x4), _ptr(out), 2, 3, 64, _ptr(ws), need - 1, st) == EWORKSPACE
    assert L.ganlab_ln_rowsums_f32(_ptr(a), None, _ptr(x), _ptr(mean), _ptr(rstd), None, None, _ptr(out), n, m, _ptr(ws),
                                   ws.numel() * 8, _ptr(x), None, 0.2, st) == EINVAL            # yact without gz
    assert L.ganlab_coldot_f32(_ptr(a), _ptr(x), _ptr(mean), None, _ptr(o1), None, n, m, st) == EINVAL
    assert L.ganlab_launch_count() == count
    assert bool((out == 0).all()) and bool((o1 == 0).all())
