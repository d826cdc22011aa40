"""GPU tests of class conditioning (csrc/cond.hip; gan_lab_amd/conditional.py): ``ops.cond_batch_norm``, the projection family
``ops.class_projection``, the conditional ResNet networks and the learner with ``config.cgan='projection'``.

Op bound, per tensor: ``rel_err <= max(1e-5, 16 * e_cpu)`` where ``e_cpu`` is the error of the reference (cond_reference.py) run
in fp32 on the CPU against its own float64 run on the same inputs - the rule and headroom of tests/test_gpu_attn.py and
tests/test_gpu_sn.py.  Network bound: TOL = 1e-3 of tests/test_gpu_resnet.py.  The fused activation is never judged against
float64 (a ReLU tie would hide a failure or fake one): its forward is compared bitwise, its gradients within the op bound, with
the unfused composition on the GPU.

Measured errors: not recorded yet; every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import cond_reference as ref
from util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3
CBN_NAMES = ('y', 'gx', 'dweight', 'dbias')
# (N, C, H, W, K), labels (None: drawn)
CBN_CASES = [((3, 5, 7, 7, 3), None), ((4, 8, 8, 8, 3), (2, 0, 2, 2)), ((2, 64, 32, 32, 10), None), ((1, 4, 4, 4, 2), None)]
PROJ_CASES = [((5, 37, 4), None), ((8, 8192, 10), None), ((1, 128, 2), (1,))]
_ids = lambda cases: ['x'.join(map(str, s)) for s, _ in cases]      # noqa: E731


def _bound(name, e, c):
    assert e <= max(1e-5, 16 * c), f'{name}: {e:.3e} > max(1e-5, 16 * {c:.3e})'


@functools.lru_cache(maxsize=None)
def _cbn_case(shape, labels):
    """Inputs (CPU fp32), the float64 reference and e_cpu of every tensor; computed once, never modified."""
    n, c, h, w, k = shape
    g = torch.Generator().manual_seed(100 * c + h)
    x = torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3
    weight, bias = torch.randn(k, c, generator=g) * 0.5 + 1.0, torch.randn(k, c, generator=g) * 0.5
    gy = torch.randn(n, c, h, w, generator=g)
    labels = torch.tensor(labels, dtype=torch.int32) if labels is not None else \
        torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    want = ref.cond_batch_norm_with_grads(x, weight, bias, labels, gy, torch.float64)
    cpu = ref.cond_batch_norm_with_grads(x, weight, bias, labels, gy, torch.float32)
    return (x, weight, bias, labels, gy), want, [rel_err(a, b) for a, b in zip(cpu, want)]


def _cbn_gpu(x, weight, bias, labels, gy, act_slope=None, fused=True):
    from gan_lab_amd import ops
    x, weight, bias = (t.cuda().requires_grad_(True) for t in (x, weight, bias))
    c = x.shape[1]
    rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
    y = ops.cond_batch_norm(x, weight, bias, labels.cuda(), rm, rv, True, act_slope=act_slope if fused else None)
    if act_slope is not None and not fused:
        y = ops.bias_act(y, act='lrelu', slope=act_slope)
    gx, gw, gb = torch.autograd.grad(y, (x, weight, bias), gy.cuda())
    return y.detach(), gx, gw, gb


@pytest.mark.parametrize('shape,labels', CBN_CASES, ids=_ids(CBN_CASES))
def test_cond_batch_norm_against_float64(shape, labels):
    inputs, want, e_cpu = _cbn_case(shape, labels)
    got = _cbn_gpu(*inputs)
    errs = [rel_err(a, b) for a, b in zip(got, want)]
    print(f'cbn {shape}: ' + ' '.join(f'{nm} gpu {e:.2e} cpu {c:.2e}' for nm, e, c in zip(CBN_NAMES, errs, e_cpu)))
    for nm, e, c in zip(CBN_NAMES, errs, e_cpu):
        _bound(nm, e, c)
    present = set(inputs[3].tolist())
    for k in range(shape[4]):
        if k not in present:                         # a class absent from the batch: rows of exact zeros, written
            assert bool((got[2][k] == 0).all()) and bool((got[3][k] == 0).all()), k
    if labels is not None:
        assert 1 not in present                      # the case that has one


def test_running_statistics_follow_batchnorm_and_eval_mode():
    from gan_lab_amd import ops
    (x, weight, bias, labels, _), _, e_cpu = _cbn_case((4, 8, 8, 8, 3), (2, 0, 2, 2))
    g = torch.Generator().manual_seed(3)
    x2 = torch.randn(*x.shape, generator=g) * 0.7 - 0.2
    bn = torch.nn.BatchNorm2d(8).double().train()
    bn(x.double())
    bn(x2.double())
    rm, rv, cnt = torch.zeros(8).cuda(), torch.ones(8).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    for xi in (x, x2):
        ops.cond_batch_norm(xi.cuda(), weight.cuda(), bias.cuda(), labels.cuda(), rm, rv, True, momentum=bn.momentum, eps=bn.eps,
                            batches=cnt)
    errs = rel_err(rm, bn.running_mean), rel_err(rv, bn.running_var)
    print(f'running mean {errs[0]:.2e} var {errs[1]:.2e} (e_cpu y {e_cpu[0]:.2e})')
    assert int(cnt) == int(bn.num_batches_tracked) == 2
    for nm, e in zip(('running_mean', 'running_var'), errs):
        _bound(nm, e, e_cpu[0])
    # eval mode: the running statistics, no update of them
    before = rm.clone(), rv.clone()
    want = ref.cond_batch_norm_eval(x, weight, bias, labels, rm.cpu(), rv.cpu(), bn.eps, torch.float64)
    cpu = ref.cond_batch_norm_eval(x, weight, bias, labels, rm.cpu(), rv.cpu(), bn.eps, torch.float32)
    got = ops.cond_batch_norm(x.cuda(), weight.cuda(), bias.cuda(), labels.cuda(), rm, rv, False, eps=bn.eps, batches=cnt)
    e, c = rel_err(got, want), rel_err(cpu, want)
    print(f'eval y gpu {e:.2e} cpu {c:.2e}')
    _bound('eval y', e, c)
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and int(cnt) == 2
    # eval-mode gradients: mean / rstd are constants
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, weight, bias))
    gy = torch.randn(*x.shape, generator=g)
    got_g = torch.autograd.grad(ops.cond_batch_norm(xg, wg, bg, labels.cuda(), rm, rv, False, eps=bn.eps), (xg, wg, bg), gy.cuda())
    leaves = [t.double().clone().requires_grad_(True) for t in (x, weight, bias)]
    want_g = torch.autograd.grad(ref.cond_batch_norm_eval(*leaves, labels, rm.cpu().double(), rv.cpu().double(), bn.eps), leaves,
                                 gy.double())
    for nm, a, b, c in zip(CBN_NAMES[1:], got_g, want_g, e_cpu[1:]):
        print(f'eval {nm} {rel_err(a, b):.2e}')
        _bound('eval ' + nm, rel_err(a, b), c)


@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('shape,labels', CBN_CASES[:2], ids=_ids(CBN_CASES[:2]))
def test_fused_activation_equals_the_unfused_composition(shape, labels, slope):
    inputs, _, e_cpu = _cbn_case(shape, labels)
    fused, unfused = _cbn_gpu(*inputs, act_slope=slope), _cbn_gpu(*inputs, act_slope=slope, fused=False)
    assert torch.equal(fused[0], unfused[0])
    errs = [rel_err(a, b) for a, b in zip(fused[1:], unfused[1:])]
    print(f'cbn {shape} slope {slope}: ' + ' '.join(f'{nm} {e:.2e}' for nm, e in zip(CBN_NAMES[1:], errs)))
    for nm, e, c in zip(CBN_NAMES[1:], errs, e_cpu[1:]):
        _bound(nm, e, c)


@pytest.mark.parametrize('shape,labels', CBN_CASES[:3], ids=_ids(CBN_CASES[:3]))
def test_equal_rows_reproduce_batch_norm(shape, labels):
    from gan_lab_amd import ops
    (x, weight, bias, lab, gy), _, e_cpu = _cbn_case(shape, labels)
    n, c, h, w, k = shape
    w1, b1 = weight[0].clone(), bias[0].clone()
    for slope in (None, 0.0, 0.2):
        xb, wb, bb = (t.cuda().requires_grad_(True) for t in (x, w1, b1))
        yb = ops.batch_norm(xb, wb, bb, torch.zeros(c).cuda(), torch.ones(c).cuda(), True, act_slope=slope)
        want = torch.autograd.grad(yb, (xb, wb, bb), gy.cuda())
        got = _cbn_gpu(x, w1.expand(k, c).contiguous(), b1.expand(k, c).contiguous(), lab, gy, act_slope=slope)
        assert torch.equal(got[0], yb.detach()), slope                   # bit for bit
        errs = [rel_err(got[1], want[0]), rel_err(got[2].sum(0), want[1]), rel_err(got[3].sum(0), want[2])]
        print(f'equal rows {shape} slope {slope}: ' + ' '.join(f'{nm} {e:.2e}' for nm, e in zip(CBN_NAMES[1:], errs)))
        for nm, e, cc in zip(CBN_NAMES[1:], errs, e_cpu[1:]):
            _bound(nm, e, cc)


def test_cond_batch_norm_arguments():
    from gan_lab_amd import ops
    x, w, b = torch.randn(2, 3, 4, 4).cuda(), torch.ones(2, 3).cuda(), torch.zeros(2, 3).cuda()
    rm, rv = torch.zeros(3).cuda(), torch.ones(3).cuda()
    l32 = torch.tensor([1, 0], dtype=torch.int32).cuda()
    y = ops.cond_batch_norm(x, w, b, l32, rm, rv, True)
    assert torch.equal(y, ops.cond_batch_norm(x, w, b, l32.long(), rm, rv, True))          # int64 is accepted
    with pytest.raises(TypeError):
        ops.cond_batch_norm(x, w, b, l32.cpu(), rm, rv, True)
    with pytest.raises(TypeError):
        ops.cond_batch_norm(x, w, b, l32.float(), rm, rv, True)
    with pytest.raises(ValueError):
        ops.cond_batch_norm(x, w, b, l32[:1], rm, rv, True)
    with pytest.raises(ValueError):
        ops.cond_batch_norm(x, w[:, :2].contiguous(), b[:, :2].contiguous(), l32, rm, rv, True)
    # a label outside [0, K) is clamped by the kernels, never an index outside the tables
    w2 = torch.tensor([[1., 1., 1.], [2., 2., 2.]]).cuda()
    wild = torch.tensor([7, -3], dtype=torch.int32).cuda()
    assert torch.equal(ops.cond_batch_norm(x, w2, b, wild, rm, rv, True), ops.cond_batch_norm(x, w2, b, l32, rm, rv, True))


# ---- projection ---------------------------------------------------------------------------------------------------------------
PROJ_NAMES = ('P', 'G', 'S', 'dbase')


@functools.lru_cache(maxsize=None)
def _proj_case(shape, labels):
    n, nf, k = shape
    g = torch.Generator().manual_seed(nf + n)
    f, W = torch.randn(n, nf, generator=g), torch.randn(k, nf, generator=g) / nf ** 0.5
    base, cot = torch.randn(n, generator=g), torch.randn(n, generator=g)
    labels = torch.tensor(labels, dtype=torch.int32) if labels is not None else \
        torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    want = ref.projection_with_grads(f, W, labels, base, cot, torch.float64)
    cpu = ref.projection_with_grads(f, W, labels, base, cot, torch.float32)
    return (f, W, labels, base, cot), want, [rel_err(a, b) for a, b in zip(cpu, want)]


def _proj_gpu(f, W, labels, base, cot):
    from gan_lab_amd import ops
    f, W, base = (t.cuda().requires_grad_(True) for t in (f, W, base))
    out = ops.class_projection(f, W, labels.cuda(), base)
    gf, gw, gbase = torch.autograd.grad(out, (f, W, base), cot.cuda())
    return out.detach(), gf, gw, gbase


@pytest.mark.parametrize('shape,labels', PROJ_CASES, ids=_ids(PROJ_CASES))
def test_projection_against_float64(shape, labels):
    from gan_lab_amd import ops
    inputs, want, e_cpu = _proj_case(shape, labels)
    got = _proj_gpu(*inputs)
    errs = [rel_err(a, b) for a, b in zip(got, want)]
    print(f'proj {shape}: ' + ' '.join(f'{nm} gpu {e:.2e} cpu {c:.2e}' for nm, e, c in zip(PROJ_NAMES, errs, e_cpu)))
    for nm, e, c in zip(PROJ_NAMES, errs, e_cpu):
        _bound(nm, e, c)
    f, W, lab, base, cot = inputs
    assert torch.equal(got[3].cpu(), cot)                                # base is passed through, and so is its gradient
    zero = ops.class_projection(f.cuda(), torch.zeros_like(W).cuda(), lab.cuda(), base.cuda())
    assert torch.equal(zero.cpu(), base)                                 # weight = 0: out == base, bit for bit
    nobase = ops.class_projection(f.cuda(), W.cuda(), lab.cuda())
    assert rel_err(nobase, ref.projection(f, W, lab, None, torch.float64)) <= max(1e-5, 16 * e_cpu[0])
    present = set(lab.tolist())
    for k in range(shape[2]):
        if k not in present:
            assert bool((got[2][k] == 0).all()), k
    if labels is not None:
        assert 0 not in present


@pytest.mark.parametrize('shape,labels', PROJ_CASES[:1] + PROJ_CASES[2:], ids=_ids(PROJ_CASES[:1] + PROJ_CASES[2:]))
def test_projection_second_order(shape, labels):
    """The family closes: gradients of gradients through P, G and S against float64 autograd on the reference."""
    from gan_lab_amd import ops
    (x, W, lab, _, _), _, _ = _proj_case(shape, labels)
    want = ref.projection_second_order(x, W, lab, torch.float64)
    cpu = ref.projection_second_order(x, W, lab, torch.float32)
    xg, wg = x.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
    got = ref.second_order_scalars(lambda f, w, l: ops.class_projection(f, w, l), xg, wg, lab.cuda())
    for nm, a, b, c in zip(('dW of |g|^2', 'dx of the mixed scalar', 'dx through S'), got, want, cpu):
        e, ec = rel_err(a, b), rel_err(c, b)
        print(f'proj {shape} second order, {nm}: gpu {e:.2e} cpu {ec:.2e}')
        _bound(nm, e, ec)


def test_input_grad_only_skips_the_weight_gradient():
    from gan_lab_amd import ops
    (f, W, lab, base, cot), _, _ = _proj_case((5, 37, 4), None)
    f, W = f.cuda().requires_grad_(True), W.cuda().requires_grad_(True)
    out = ops.class_projection(f, W, lab.cuda(), base.cuda())
    with ops.input_grad_only():
        gf, gw = torch.autograd.grad(out, (f, W), cot.cuda(), retain_graph=True, allow_unused=True)
    assert gw is None and gf is not None                                 # no S launch: nothing was computed for W
    gf2, gw2 = torch.autograd.grad(out, (f, W), cot.cuda())
    assert gw2 is not None and torch.equal(gf, gf2)
    with pytest.raises(TypeError):
        ops.class_projection(f.detach().cpu(), W.detach().cpu(), lab, base)
    with pytest.raises(TypeError):
        ops.class_projection(f, W, lab, base.cuda())                     # labels on the host
    wild = torch.tensor([9, -1, 2, 3, 0], dtype=torch.int64).cuda()      # clamped: rows 3, 0, 2, 3, 0
    assert torch.equal(ops.class_projection(f, W, wild), ops.class_projection(f, W, torch.tensor([3, 0, 2, 3, 0]).cuda()))


# ---- hygiene ------------------------------------------------------------------------------------------------------------------
def _poisoned(sizes, gap=61):
    buf = torch.full((sum(sizes.values()) + gap * (len(sizes) + 1),), float('nan'), device='cuda')
    views, inside, off = {}, torch.zeros(buf.numel(), dtype=torch.bool, device='cuda'), gap
    for name, size in sizes.items():
        off = (off + 3) // 4 * 4                         # 16-byte aligned views: the float4 paths are the ones under test
        views[name] = buf[off:off + size]
        inside[off:off + size] = True
        off += size + gap
    return buf, views, inside


def test_tails_stay_inside_their_buffers():
    """Outputs live inside NaN-poisoned buffers with gaps: the kernels write their tensors and nothing else."""
    from gan_lab_amd import _lib, ops
    L, p, st = _lib.lib(), ops._p, ops._st()
    (x, weight, bias, lab, gy), _, _ = _cbn_case((4, 8, 8, 8, 3), (2, 0, 2, 2))
    n, c, h, w, k = 4, 8, 8, 8, 3
    x, weight, bias, lab, gy = (t.cuda() for t in (x, weight, bias, lab, gy))
    mean, rstd = x.mean((0, 2, 3)), torch.rsqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)
    sizes = dict(y=x.numel(), gz=x.numel(), gx=x.numel(), gw=k * c, gb=k * c, sums=2 * c, ws=n * c * 2 * 2 + 2)
    buf, v, inside = _poisoned(sizes)
    ws = v['ws'][(-(v['ws'].data_ptr() // 4) % 2):]        # fp64 partials: 8-byte aligned
    _lib.check(L.ganlab_cbn_apply_f32(p(x), p(mean), p(rstd), p(weight), p(bias), p(lab), p(v['y']), n, c, h * w, k,
                                      _lib.ACT_LRELU, 0.2, st), 'cbn_apply')
    _lib.check(L.ganlab_cbn_bwd_f32(p(gy), p(x), p(mean), p(rstd), p(weight), p(lab), p(v['y']), p(v['gz']), p(v['gx']),
                                    p(v['gw']), p(v['gb']), p(v['sums']), n, c, h * w, k, 1, 0.2, p(ws), n * c * 2 * 8, st),
               'cbn_bwd')
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[~inside]).all())
    for name in ('y', 'gz', 'gx', 'gw', 'gb', 'sums'):
        assert not bool(torch.isnan(v[name]).any()), name
    assert not bool(torch.isnan(ws[:n * c * 2 * 2]).any())
    assert bool((v['gw'].view(k, c)[1] == 0).all())
    # the scalar paths: odd plane size
    (x, weight, bias, lab, gy), _, _ = _cbn_case((3, 5, 7, 7, 3), None)
    n, c, h, w, k = 3, 5, 7, 7, 3
    x, weight, bias, lab, gy = (t.cuda() for t in (x, weight, bias, lab, gy))
    mean, rstd = x.mean((0, 2, 3)), torch.rsqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)
    sizes = dict(y=x.numel(), gx=x.numel(), gw=k * c, gb=k * c, sums=2 * c, ws=n * c * 2 * 2 + 2)
    buf, v, inside = _poisoned(sizes)
    ws = v['ws'][(-(v['ws'].data_ptr() // 4) % 2):]
    _lib.check(L.ganlab_cbn_apply_f32(p(x), p(mean), p(rstd), p(weight), p(bias), p(lab), p(v['y']), n, c, h * w, k,
                                      _lib.ACT_NONE, 1.0, st), 'cbn_apply')
    _lib.check(L.ganlab_cbn_bwd_f32(p(gy), p(x), p(mean), p(rstd), p(weight), p(lab), None, None, p(v['gx']), p(v['gw']),
                                    p(v['gb']), p(v['sums']), n, c, h * w, k, 1, 1.0, p(ws), n * c * 2 * 8, st), 'cbn_bwd')
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[~inside]).all())
    for name in ('y', 'gx', 'gw', 'gb', 'sums'):
        assert not bool(torch.isnan(v[name]).any()), name
    # the projection family
    (f, W, lab, base, cot), _, _ = _proj_case((5, 37, 4), None)
    n, nf, k = 5, 37, 4
    f, W, lab, base, cot = (t.cuda() for t in (f, W, lab, base, cot))
    buf, v, inside = _poisoned(dict(out=n, gf=n * nf, gw=k * nf))
    _lib.check(L.ganlab_proj_fwd_f32(p(f), p(W), p(lab), p(base), p(v['out']), n, nf, k, st), 'proj_fwd')
    _lib.check(L.ganlab_proj_dfeat_f32(p(cot), p(W), p(lab), p(v['gf']), n, nf, k, st), 'proj_dfeat')
    _lib.check(L.ganlab_proj_dweight_f32(p(cot), p(f), p(lab), p(v['gw']), n, nf, k, st), 'proj_dweight')
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[~inside]).all()) and not bool(torch.isnan(buf[inside]).any())
    got = _proj_gpu(*(t.cpu() for t in (f, W, lab, base, cot)))
    for name, t in (('out', got[0]), ('gf', got[1]), ('gw', got[2])):
        assert torch.equal(v[name], t.reshape(-1)), name


def test_two_runs_are_bit_equal():
    for slope in (None, 0.2):
        inputs, _, _ = _cbn_case((4, 8, 8, 8, 3), (2, 0, 2, 2))
        a, b = _cbn_gpu(*inputs, act_slope=slope), _cbn_gpu(*inputs, act_slope=slope)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    inputs, _, _ = _cbn_case((2, 64, 32, 32, 10), None)
    assert all(torch.equal(s, t) for s, t in zip(_cbn_gpu(*inputs), _cbn_gpu(*inputs)))
    for shape, labels in PROJ_CASES[:2]:
        inputs, _, _ = _proj_case(shape, labels)
        assert all(torch.equal(s, t) for s, t in zip(_proj_gpu(*inputs), _proj_gpu(*inputs)))


def test_forward_and_backward_replay_from_a_graph():
    """No host readback, no upload: forward + backward captured with torch.cuda.graph replays to the bits of the eager run."""
    from gan_lab_amd import ops
    (x, weight, bias, lab, gy), _, _ = _cbn_case((4, 8, 8, 8, 3), (2, 0, 2, 2))
    (f, W, plab, base, cot), _, _ = _proj_case((5, 37, 4), None)
    x, weight, bias, f, W, base = (t.cuda().requires_grad_(True) for t in (x, weight, bias, f, W, base))
    lab, gy, plab, cot = lab.cuda(), gy.cuda(), plab.cuda(), cot.cuda()
    rm, rv, cnt = torch.zeros(8).cuda(), torch.ones(8).cuda(), torch.zeros((), dtype=torch.int64).cuda()

    def run():
        y = ops.cond_batch_norm(x, weight, bias, lab, rm, rv, True, batches=cnt, act_slope=0.2)
        out = ops.class_projection(f, W, plab, base)
        return (y, out) + torch.autograd.grad(y, (x, weight, bias), gy) + torch.autograd.grad(out, (f, W, base), cot)

    eager = [t.detach().clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        if t.data_ptr() != cot.data_ptr():
            t.detach().zero_()              # a capture records, it does not run
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b.detach())
    assert int(cnt) == 2                    # the eager run and the replay; the capture itself counted nothing


# ---- the networks -------------------------------------------------------------------------------------------------------------
NETS = [('Generator64PixResnet', dict(fmap=16, len_latent=32), (3, 32)),
        ('Discriminator64PixResnet', dict(fmap=16), (3, 3, 64, 64)),
        ('Generator32PixResnet', dict(fmap=32, len_latent=32), (3, 32)),
        ('Discriminator32PixResnet', dict(fmap=32), (3, 3, 32, 32))]
K = 4


def _net_pair(name, kw, seed):
    """An unconditional network with non-trivial norm affines, and the conditional one carrying its weights: norm rows
    broadcast, the projection zero."""
    from gan_lab_amd.resnetgan import architectures as A
    torch.manual_seed(seed)
    off = getattr(A, name)(**kw)
    on = getattr(A, name)(cgan=True, num_classes=K, **kw)
    sd, sd_on = off.state_dict(), on.state_dict()
    with torch.no_grad():
        for k_, v in sd.items():
            if k_.endswith(('norm.weight', 'norm.bias')) and name.startswith('Generator'):
                v.add_(0.3 * torch.randn_like(v))
    load = {}
    for k_, v in sd_on.items():
        if k_ == 'proj.linear.weight':
            load[k_] = torch.zeros_like(v)
        elif v.shape != sd[k_].shape:
            assert v.shape == (K,) + tuple(sd[k_].shape), k_
            load[k_] = sd[k_].expand(K, -1).clone()
        else:
            load[k_] = sd[k_].clone()
    off.load_state_dict(sd)
    on.load_state_dict(load)
    return off.cuda().train(), on.cuda().train()


@pytest.mark.parametrize('name,kw,in_shape', NETS, ids=[n for n, _, _ in NETS])
def test_networks_carry_an_unconditional_networks_weights(name, kw, in_shape):
    off, on = _net_pair(name, kw, 21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*in_shape, generator=g).cuda()
    labels = torch.tensor([3, 0, 2], dtype=torch.int32).cuda()
    y_off = off(x)
    cot = torch.randn(*y_off.shape, generator=g).cuda()
    y_off.backward(cot)
    y_on = on(x, labels)
    y_on.backward(cot)
    assert torch.equal(y_on.detach(), y_off.detach())                       # bit for bit, for any labels
    assert torch.equal(on(x, torch.tensor([1, 1, 0]).cuda()).detach(), y_off.detach())
    shared = dict(off.named_parameters())
    worst = 0.0
    for k_, p in on.named_parameters():
        if k_.endswith(('conv2d.weight', 'linear.weight')) and k_ in shared:
            worst = max(worst, rel_err(p.grad, shared[k_].grad))
    print(f'{name}: worst conv / linear weight gradient difference {worst:.2e}')
    assert worst <= TOL
    with pytest.raises(TypeError, match='labels'):
        on(x)
    with pytest.raises(TypeError, match='labels'):
        off(x, labels)
    if name.startswith('Generator'):
        assert all(m.labels is None for m in on._cond_norms)                # cleared after the forward


@pytest.mark.parametrize('name,kw,in_shape', NETS, ids=[n for n, _, _ in NETS])
def test_a_label_moves_its_own_sample_only(name, kw, in_shape):
    _, on = _net_pair(name, kw, 23)
    gen = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for k_, p in on.named_parameters():
            if k_.endswith(('norm.weight', 'norm.bias')) and p.dim() == 2 and p.shape[0] == K:
                p.add_(0.5 * torch.randn(*p.shape, generator=gen).cuda())
            elif k_ == 'proj.linear.weight':
                p.copy_(torch.randn(*p.shape, generator=gen).cuda())
    x = torch.randn(*in_shape, generator=gen).cuda()
    a, b = torch.tensor([0, 1, 2], dtype=torch.int32).cuda(), torch.tensor([0, 3, 2], dtype=torch.int32).cuda()
    if name.startswith('Generator'):
        on(x, a)                                   # one training-mode pass fills the running statistics
        on.eval()                                  # batch statistics couple the samples; the running ones do not
    with torch.no_grad():
        ya, yb = on(x, a), on(x, b)
    assert torch.equal(ya[0], yb[0]) and torch.equal(ya[2], yb[2])
    assert not torch.equal(ya[1], yb[1])
    if name.startswith('Disc'):
        assert torch.equal(on.features(x), on.features(x))                   # label-free


# ---- the learner --------------------------------------------------------------------------------------------------------------
def _learner(**kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    kw.setdefault('random_seed', 7)
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=2, len_latent=32, num_classes=3,
                      cgan='projection', **kw)
    cfg.fmap_g, cfg.fmap_d = 32, 32
    torch.manual_seed(7)
    return GANLearner(cfg)


def _batches(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).cuda() for _ in range(n)], \
        [torch.randn(4, 32, generator=g).cuda() for _ in range(n)], \
        [torch.tensor([0, 2, 2, 0] if i % 2 == 0 else [2, 2, 0, 2]) for i in range(n)]      # labels from {0, 2}, on the host


def _iteration(L, reals, zs, labels):
    """One main iteration: generator step, then two critic steps."""
    L.set_requires_grad_disc(False)
    losses = [L.g_step(zb=zs[0], labels=labels[0])]
    L.set_requires_grad_disc(True)
    for i in range(2):
        losses.append(L.d_step(reals[i], zb=zs[1 + i], labels=labels[1 + i]))
    return [float(v) for v in losses]


def _tables(L):
    out = {'g.' + k_: p for k_, p in L.gen_model.named_parameters() if k_.endswith(('norm.weight', 'norm.bias'))}
    out['d.proj.linear.weight'] = L.disc_model.proj.linear.weight
    return out


def test_learner_default_loss_and_penalty():
    """wgan + wgan-gp (the double backward runs through the projection), labels from {0, 2} only: finite losses, rows 0 and 2 of
    every table move, row 1 - zero gradient, zero Adam moments, no weight decay - keeps its bits."""
    L = _learner(wd=0.)
    assert L.gradient_penalty == 'wgan-gp' and L.loss == 'wgan' and L.sn is None
    before = {k_: p.detach().clone() for k_, p in _tables(L).items()}
    assert len(before) == 15
    reals, zs, labels = _batches(9)
    for it in range(3):
        losses = _iteration(L, reals[2 * it:2 * it + 2], zs[3 * it:3 * it + 3], labels[3 * it:3 * it + 3])
        print('iteration', it, losses)
        assert all(np.isfinite(losses)), losses
    gp = float(L.calc_gp(reals[0], reals[1], labels=labels[0].int().cuda()))
    print('penalty', gp)
    assert np.isfinite(gp)
    for k_, p in _tables(L).items():
        assert torch.equal(p.detach()[1], before[k_][1]), k_
        assert not torch.equal(p.detach()[0], before[k_][0]) and not torch.equal(p.detach()[2], before[k_][2]), k_


SAGAN = dict(self_attention='gd', spectral_norm=True, loss='hinge', gradient_penalty=None)


def test_learner_sagan_recipe(tmp_path):
    L = _learner(**SAGAN)
    assert 'proj.linear.weight' in L.sn.names
    assert 'proj.linear.weight_u' in L.disc_model.state_dict()
    assert L.disc_model.proj.weight_override is not None
    reals, zs, labels = _batches(12)
    for it in range(2):
        losses = _iteration(L, reals[2 * it:2 * it + 2], zs[3 * it:3 * it + 3], labels[3 * it:3 * it + 3])
        assert all(np.isfinite(losses)), losses
    L.not_trained_yet = False
    path = tmp_path / 'resnetgan_model.tar'
    L.save_model(path)
    with pytest.raises(ValueError, match='reference_format'):
        L.save_model(path, reference_format=True)
    from gan_lab_amd import checkpoint
    assert checkpoint.load_checkpoint(path, 'cpu')['config']['cgan'] == 'projection'
    L2 = _learner(**SAGAN)
    L2.load_model(path)
    L2.gen_model.train()
    L2.disc_model.train()
    for m, m2 in ((L.gen_model, L2.gen_model), (L.disc_model, L2.disc_model)):
        sd, sd2 = m.state_dict(), m2.state_dict()
        assert list(sd.keys()) == list(sd2.keys())
        for k_ in sd:
            assert torch.equal(sd[k_].cpu(), sd2[k_].cpu()), k_
    a = _iteration(L, reals[6:8], zs[9:12], labels[9:12])
    b = _iteration(L2, reals[6:8], zs[9:12], labels[9:12])
    assert a == b, (a, b)
    for (k_, p), (_, p2) in zip(list(L.gen_model.named_parameters()) + list(L.disc_model.named_parameters()),
                                list(L2.gen_model.named_parameters()) + list(L2.disc_model.named_parameters())):
        assert torch.equal(p.detach(), p2.detach()), k_


def test_learner_labels_are_required_drawn_and_reproducible():
    from gan_lab_amd import rng
    reals, zs, labels = _batches(3)
    runs = []
    for _ in range(2):
        L = _learner(random_seed=11)
        with pytest.raises(ValueError, match='labels'):
            L.d_step(reals[0], zb=zs[0])
        with pytest.raises(ValueError, match='labels'):
            L.d_step(reals[0], zb=zs[0], labels=torch.tensor([0, 1, 2, 3]))       # out of range, on the host
        pos = rng._STATE['offset']
        drawn = rng.randint(64, 3, 'cuda')
        assert drawn.dtype == torch.int32 and rng._STATE['offset'] == pos + 16
        assert set(drawn.tolist()) == {0, 1, 2}
        L.set_requires_grad_disc(False)
        losses = [float(L.g_step())]                                              # latents and labels both drawn
        L.set_requires_grad_disc(True)
        losses += [float(L.d_step(reals[i], labels=labels[i])) for i in range(2)]
        runs.append((drawn.cpu(), losses, [p.detach().clone() for p in L.gen_model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert all(torch.equal(p, q) for p, q in zip(runs[0][2], runs[1][2]))


def test_paired_and_separate_critic_passes_agree(monkeypatch):
    reals, zs, labels = _batches(1)
    losses = []
    for pair in ('0', '1'):
        monkeypatch.setenv('GANLAB_RESNET_PAIR', pair)
        L = _learner()
        with torch.no_grad():
            L.disc_model.proj.linear.weight.mul_(4.0)                             # a class term that matters
        L.set_requires_grad_disc(True)
        losses.append(float(L.d_step(reals[0], zb=zs[0], eps_interp=torch.full((4,), 0.3).cuda(), labels=labels[0])))
    monkeypatch.delenv('GANLAB_RESNET_PAIR')
    L = _learner()
    with torch.no_grad():
        L.disc_model.proj.linear.weight.mul_(4.0)
    L.set_requires_grad_disc(True)
    losses.append(float(L.d_step(reals[0], zb=zs[0], eps_interp=torch.full((4,), 0.3).cuda(), labels=labels[0])))
    print('D loss, separate / paired / default:', losses)
    assert abs(losses[0] - losses[1]) <= TOL * max(abs(losses[0]), 1e-30)
    assert losses[1] == losses[2]


def test_learner_without_the_option_is_untouched():
    from gan_lab_amd import rng
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=2, len_latent=32, random_seed=7)
    cfg.fmap_g, cfg.fmap_d = 32, 32
    L = GANLearner(cfg)
    assert L.cgan is False and L.disc_model.proj is None and not L.gen_model._cond_norms
    assert not any('proj' in k_ for k_ in L.disc_model.state_dict())
    pos = rng._STATE['offset']
    L.set_requires_grad_disc(False)
    L.g_step()
    assert rng._STATE['offset'] == pos + (4 * 32 + 3) // 4                       # the latents, and nothing else, were drawn
    with pytest.raises(ValueError, match='not class-conditional'):
        L.g_step(labels=torch.zeros(4, dtype=torch.int32).cuda())


def test_train_reads_the_labels_from_the_loader():
    from gan_lab_amd.utils.data_utils import DeviceImageLoader
    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (8, 32, 32, 3), generator=g, dtype=torch.uint8)
    L = _learner()
    before = L.disc_model.proj.linear.weight.detach().clone()
    L.train(DeviceImageLoader(images, 4, 32, labels=torch.tensor([0, 1, 2, 0, 1, 2, 0, 1]), seed=1), num_main_iters=1)
    assert np.isfinite(float(L.last_losses.get('loss_d', 0.0) or 0.0))
    assert not torch.equal(L.disc_model.proj.linear.weight.detach(), before)
    with pytest.raises(ValueError, match='labels'):             # refused on the host, from inside train()
        L.train(DeviceImageLoader(images, 4, 32, labels=torch.tensor([0, 1, 2, 3, 1, 2, 0, 1]), shuffle=False), num_main_iters=1)
