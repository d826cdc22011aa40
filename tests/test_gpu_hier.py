"""GPU tests of BigGAN's generator conditioning (csrc/hier.hip; gan_lab_amd/hier_latent.py): the batched modulation
(``ops.hier_modulate``), the modulated BatchNorm (``ops.mod_batch_norm``), the generators with ``hier_latent`` / ``shared_embed``
and the learner.

Op bound, per tensor: ``rel_err <= max(1e-5, 16 * e_cpu)`` where ``e_cpu`` is the error of the reference (hier_reference.py) run in
fp32 on the CPU against its own float64 run on the same inputs - the rule of tests/test_gpu_cond.py.  Network bound: TOL = 1e-3 of
tests/test_gpu_resnet.py.  The fused activation is never judged against float64 (a ReLU tie would hide a failure or fake one): its
forward is compared bitwise, its gradients within the op bound, with the unfused composition on the GPU.

Measured errors (MI355X): at most 7.6e-8 for the modulation family, 1.6e-7 for the norm; every test prints its
figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import hier_reference as ref
from util import rel_err, resnet_zero_grad_key

pytestmark = pytest.mark.gpu

TOL = 1e-3


def _bound(name, e, c):
    assert e <= max(1e-5, 16 * c), f'{name}: {e:.3e} > max(1e-5, 16 * {c:.3e})'


# ---- the modulation family -------------------------------------------------------------------------------------------------
# (N, Cs: one norm (a gain and a shift job) per entry, Lz, chunks per norm (offset, width), E); K = 4, class 1 absent
K = 4
MOD_CASES = {
    'hier_d7': (3, (5, 8, 64), 16, ((2, 7), (9, 7), (9, 7)), 0),
    'hier_d1_n1': (1, (5, 8, 64), 4, ((1, 1), (2, 1), (3, 1)), 0),
    'shared_only': (5, (5, 8, 64), 6, ((0, 0), (0, 0), (0, 0)), 7),
    'both_d153': (5, (5, 8, 64, 130), 128, ((28, 25), (28, 25), (53, 25), (103, 25)), 128),
    'both_nine_jobs': (3, (5, 8, 64, 3, 70), 11, ((1, 2), (1, 2), (3, 4), (7, 4), (7, 4)), 1),
}


@functools.lru_cache(maxsize=None)
def _mod_case(name):
    """Inputs (CPU fp32), the float64 reference and e_cpu of every tensor; computed once, never modified."""
    n, cs, lz, chunks, e = MOD_CASES[name]
    g = torch.Generator().manual_seed(len(name) + 10 * n)
    z = torch.randn(n, lz, generator=g)
    shared = torch.randn(K, e, generator=g) if e else None
    labels = torch.tensor([(0, 2, 3, 3, 0)[i] for i in range(n)], dtype=torch.int32)
    jobs = []
    for c, (zo, zl) in zip(cs, chunks):
        for one in (1.0, 0.0):
            jobs.append((torch.randn(c, zl + e, generator=g) * 0.3, zo, zl, 0.5 + 0.25 * len(jobs), one))
    cot = torch.randn(n, 2 * sum(cs), generator=g)
    want = ref.modulation_with_grads(z, jobs, shared, labels, cot, torch.float64)
    cpu = ref.modulation_with_grads(z, jobs, shared, labels, cot, torch.float32)
    e_cpu = [None if a is None else rel_err(a, b) for a, b in zip(cpu, want)]
    return (z, jobs, shared, labels, cot), want, e_cpu


def _mod_gpu(z, jobs, shared, labels, cot):
    from gan_lab_amd import ops
    z = z.cuda().requires_grad_(True)
    shared = shared.cuda().requires_grad_(True) if shared is not None else None
    Ws = [W.cuda().requires_grad_(True) for W, *_ in jobs]
    table = ops.HierTable([dict(w=W, z_off=j[1], z_len=j[2], scale=j[3], one=j[4]) for W, j in zip(Ws, jobs)], z.shape[1], shared)
    out = ops.hier_modulate(table, z, labels.cuda() if shared is not None else None)
    leaves = [z] + ([shared] if shared is not None else []) + Ws
    grads = list(torch.autograd.grad(out, leaves, cot.cuda()))
    dz = grads.pop(0)
    dshared = grads.pop(0) if shared is not None else None
    return [out.detach(), dz, dshared] + grads, table


@pytest.mark.parametrize('name', list(MOD_CASES))
def test_modulation_against_float64(name):
    inputs, want, e_cpu = _mod_case(name)
    got, table = _mod_gpu(*inputs)
    assert table.n == 2 * len(MOD_CASES[name][1]) and table.T == want[0].shape[1]
    names = ['out', 'dz', 'dshared'] + [f'dW{j}' for j in range(table.n)]
    for nm, a, b, c in zip(names, got, want, e_cpu):
        if b is None:
            assert a is None, nm
            continue
        if b.abs().max() == 0:                       # a width-0 chunk has no dz at all: exact zeros
            assert bool((a == 0).all()), nm
            continue
        e = rel_err(a, b)
        print(f'mod {name} {nm}: gpu {e:.2e} cpu {c:.2e}')
        _bound(nm, e, c)
    # no job reads the first chunk (or anything outside the chunks): exact zeros, written
    z, jobs = inputs[0], inputs[1]
    read = torch.zeros(z.shape[1], dtype=torch.bool)
    for _, zo, zl, _, _ in jobs:
        read[zo:zo + zl] = True
    assert bool((got[1][:, ~read.cuda()] == 0).all())
    if inputs[2] is not None:                        # class 1 is absent from every batch: a row of exact zeros, written
        assert 1 not in set(inputs[3].tolist())
        assert bool((got[2][1] == 0).all()) and bool((got[2][0] != 0).any())


class _LaunchCount(object):
    """Kernels launched by the two modulation entry points while active.  The library counts per calling thread and the autograd
    engine launches the backward from a thread of its own, so each entry point is wrapped and the count read around the call, on
    the thread that makes it."""
    NAMES = ('ganlab_hier_fwd_f32', 'ganlab_hier_bwd_f32')

    def __enter__(self):
        from gan_lab_amd import _lib
        self.L, self.saved, self.seen = _lib.lib(), {}, {n: 0 for n in self.NAMES}
        count = self.L.ganlab_launch_count
        for name in self.NAMES:
            fn = self.saved[name] = getattr(self.L, name)

            def wrapped(*a, _fn=fn, _name=name):
                before = int(count())
                rc = _fn(*a)
                self.seen[_name] += int(count()) - before
                return rc
            setattr(self.L, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.L, name, fn)
        return False


def test_modulation_launch_count_does_not_depend_on_the_jobs():
    from gan_lab_amd import ops
    counts = {}
    for name in ('shared_only', 'both_nine_jobs'):
        inputs, _, _ = _mod_case(name)
        z, jobs, shared, labels, cot = inputs
        for jobs_ in (jobs[:2], jobs):
            zc, sc = z.cuda().requires_grad_(True), shared.cuda().requires_grad_(True)
            Ws = [W.cuda().requires_grad_(True) for W, *_ in jobs_]
            table = ops.HierTable([dict(w=W, z_off=j[1], z_len=j[2], scale=j[3], one=j[4]) for W, j in zip(Ws, jobs_)],
                                  z.shape[1], sc)
            t = sum(W.shape[0] for W in Ws)
            with _LaunchCount() as census:
                out = ops.hier_modulate(table, zc, labels.cuda())
                torch.autograd.grad(out, [zc, sc] + Ws, cot[:, :t].contiguous().cuda())
                torch.cuda.synchronize()
            counts[(name, len(jobs_))] = (census.seen['ganlab_hier_fwd_f32'], census.seen['ganlab_hier_bwd_f32'])
    print(counts)
    assert len(MOD_CASES['both_nine_jobs'][1]) * 2 >= 9
    assert set(counts.values()) == {(1, 3)}          # forward 1, backward 3 (weights; dz and d embedding; d shared): 2 jobs or 10


def test_modulation_arguments():
    from gan_lab_amd import ops
    W = torch.randn(4, 3).cuda()
    with pytest.raises(ValueError, match='leaves the latent'):
        ops.HierTable([dict(w=W, z_off=6, z_len=3, scale=1.0, one=1.0)], 8)
    with pytest.raises(ValueError, match=r'\(C, 5\)'):
        ops.HierTable([dict(w=W, z_off=0, z_len=5, scale=1.0, one=1.0)], 8)
    table = ops.HierTable([dict(w=W, z_off=1, z_len=1, scale=1.0, one=1.0)], 8, torch.randn(3, 2).cuda())
    with pytest.raises(TypeError, match='labels'):
        ops.hier_modulate(table, torch.randn(2, 8).cuda())
    with pytest.raises(ValueError, match=r'\(N, 8\)'):
        ops.hier_modulate(table, torch.randn(2, 7).cuda(), torch.zeros(2, dtype=torch.int32).cuda())
    with pytest.raises(TypeError, match='GPU'):
        ops.hier_modulate(table, torch.randn(2, 8), torch.zeros(2, dtype=torch.int32).cuda())
    # labels outside [0, K) are clamped, as in cond.hip
    z = torch.randn(2, 8).cuda()
    a = ops.hier_modulate(table, z, torch.tensor([-5, 9], dtype=torch.int32).cuda())
    b = ops.hier_modulate(table, z, torch.tensor([0, 2], dtype=torch.int32).cuda())
    assert torch.equal(a, b)


# ---- the modulated BatchNorm ----------------------------------------------------------------------------------------------
MBN_NAMES = ('y', 'gx', 'dgain', 'dshift')
MBN_CASES = [(3, 5, 7, 7), (4, 8, 8, 8), (2, 64, 32, 32), (1, 4, 4, 4)]
_ids = ['x'.join(map(str, s)) for s in MBN_CASES]
PAD = 3            # columns of the flat buffer in front of, between and behind the gain and the shift block


@functools.lru_cache(maxsize=None)
def _mbn_case(shape):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(100 * c + h)
    x = torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3
    flat = torch.randn(n, 2 * c + 3 * PAD, generator=g) * 0.5
    flat[:, PAD:PAD + c] += 1.0
    gy = torch.randn(n, c, h, w, generator=g)
    gain, shift = flat[:, PAD:PAD + c], flat[:, 2 * PAD + c:2 * PAD + 2 * c]
    want = ref.mod_batch_norm_with_grads(x, gain, shift, gy, torch.float64)
    cpu = ref.mod_batch_norm_with_grads(x, gain, shift, gy, torch.float32)
    return (x, flat, gy), want, [rel_err(a, b) for a, b in zip(cpu, want)]


def _mbn_gpu(x, flat, gy, act_slope=None, fused=True, training=True, stats=None):
    """gain / shift: strided views of ONE flat buffer; the gradients are read from that buffer's own gradient."""
    from gan_lab_amd import ops
    x, flat = x.cuda().requires_grad_(True), flat.cuda().requires_grad_(True)
    c = x.shape[1]
    gain, shift = flat[:, PAD:PAD + c], flat[:, 2 * PAD + c:2 * PAD + 2 * c]
    assert gain.stride(0) == flat.shape[1] and (x.shape[0] == 1 or not gain.is_contiguous())
    rm, rv = stats if stats is not None else (torch.zeros(c).cuda(), torch.ones(c).cuda())
    y = ops.mod_batch_norm(x, gain, shift, rm, rv, training, act_slope=act_slope if fused else None)
    if act_slope is not None and not fused:
        y = ops.bias_act(y, act='lrelu', slope=act_slope)
    gx, gflat = torch.autograd.grad(y, (x, flat), gy.cuda())
    pads = torch.cat((gflat[:, :PAD], gflat[:, PAD + c:2 * PAD + c], gflat[:, 2 * PAD + 2 * c:]), dim=1)
    assert bool((pads == 0).all())
    return y.detach(), gx, gflat[:, PAD:PAD + c], gflat[:, 2 * PAD + c:2 * PAD + 2 * c]


@pytest.mark.parametrize('shape', MBN_CASES, ids=_ids)
def test_mod_batch_norm_against_float64(shape):
    inputs, want, e_cpu = _mbn_case(shape)
    got = _mbn_gpu(*inputs)
    errs = [rel_err(a, b) for a, b in zip(got, want)]
    print(f'mbn {shape}: ' + ' '.join(f'{nm} gpu {e:.2e} cpu {c:.2e}' for nm, e, c in zip(MBN_NAMES, errs, e_cpu)))
    for nm, e, c in zip(MBN_NAMES, errs, e_cpu):
        _bound(nm, e, c)


def test_running_statistics_follow_batchnorm_and_eval_mode():
    from gan_lab_amd import ops
    (x, flat, _), _, e_cpu = _mbn_case((4, 8, 8, 8))
    g = torch.Generator().manual_seed(3)
    x2 = torch.randn(*x.shape, generator=g) * 0.7 - 0.2
    bn = torch.nn.BatchNorm2d(8).double().train()
    bn(x.double())
    bn(x2.double())
    rm, rv, cnt = torch.zeros(8).cuda(), torch.ones(8).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    fl = flat.cuda()
    gain, shift = fl[:, PAD:PAD + 8], fl[:, 2 * PAD + 8:2 * PAD + 16]
    for xi in (x, x2):
        ops.mod_batch_norm(xi.cuda(), gain, shift, rm, rv, True, momentum=bn.momentum, eps=bn.eps, batches=cnt)
    errs = rel_err(rm, bn.running_mean), rel_err(rv, bn.running_var)
    print(f'running mean {errs[0]:.2e} var {errs[1]:.2e} (e_cpu y {e_cpu[0]:.2e})')
    assert int(cnt) == int(bn.num_batches_tracked) == 2
    for nm, e in zip(('running_mean', 'running_var'), errs):
        _bound(nm, e, e_cpu[0])
    # eval mode: the running statistics, no update of them; its gradients: mean / rstd are constants
    before = rm.clone(), rv.clone()
    gy = torch.randn(*x.shape, generator=g)
    leaves = [t.double().clone().requires_grad_(True) for t in (x, flat[:, PAD:PAD + 8], flat[:, 2 * PAD + 8:2 * PAD + 16])]
    want = ref.mod_batch_norm_eval(*leaves, rm.cpu().double(), rv.cpu().double(), bn.eps)
    want = (want.detach(),) + torch.autograd.grad(want, leaves, gy.double())
    l32 = [t.detach().float().requires_grad_(True) for t in leaves]
    cpu = ref.mod_batch_norm_eval(*l32, rm.cpu(), rv.cpu(), bn.eps)
    cpu = (cpu.detach(),) + torch.autograd.grad(cpu, l32, gy)
    got = _mbn_gpu(x, flat, gy, training=False, stats=(rm, rv))
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and int(cnt) == 2
    for nm, a, b, c in zip(MBN_NAMES, got, want, cpu):
        e, ec = rel_err(a, b), rel_err(c, b)
        print(f'eval {nm} gpu {e:.2e} cpu {ec:.2e}')
        _bound('eval ' + nm, e, ec)


@pytest.mark.parametrize('shape', MBN_CASES[:3], ids=_ids[:3])
def test_equal_rows_reproduce_batch_norm(shape):
    from gan_lab_amd import ops
    (x, flat, gy), _, e_cpu = _mbn_case(shape)
    n, c, h, w = shape
    eq = flat[:1].expand(n, -1).contiguous()
    w1, b1 = eq[0, PAD:PAD + c].clone(), eq[0, 2 * PAD + c:2 * PAD + 2 * c].clone()
    g = torch.Generator().manual_seed(9)
    stats = (torch.randn(c, generator=g).cuda(), (torch.rand(c, generator=g) + 0.5).cuda())
    for training in (True, False):
        for slope in (None, 0.0, 0.2):
            xb, wb, bb = (t.cuda().requires_grad_(True) for t in (x, w1, b1))
            rm, rv = (torch.zeros(c).cuda(), torch.ones(c).cuda()) if training else stats
            yb = ops.batch_norm(xb, wb, bb, rm.clone(), rv.clone(), training, act_slope=slope)
            want = torch.autograd.grad(yb, (xb, wb, bb), gy.cuda())
            got = _mbn_gpu(x, eq, gy, act_slope=slope, training=training, stats=None if training else stats)
            assert torch.equal(got[0], yb.detach()), (training, slope)              # bit for bit
            errs = [rel_err(got[1], want[0]), rel_err(got[2].sum(0), want[1]), rel_err(got[3].sum(0), want[2])]
            print(f'equal rows {shape} training {training} slope {slope}: ' +
                  ' '.join(f'{nm} {e:.2e}' for nm, e in zip(MBN_NAMES[1:], errs)))
            for nm, e, cc in zip(MBN_NAMES[1:], errs, e_cpu[1:]):
                _bound(nm, e, cc)


@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('shape', MBN_CASES[:2], ids=_ids[:2])
def test_fused_activation_equals_the_unfused_composition(shape, slope):
    inputs, _, e_cpu = _mbn_case(shape)
    fused, unfused = _mbn_gpu(*inputs, act_slope=slope), _mbn_gpu(*inputs, act_slope=slope, fused=False)
    assert torch.equal(fused[0], unfused[0])
    errs = [rel_err(a, b) for a, b in zip(fused[1:], unfused[1:])]
    print(f'mbn {shape} slope {slope}: ' + ' '.join(f'{nm} {e:.2e}' for nm, e in zip(MBN_NAMES[1:], errs)))
    for nm, e, c in zip(MBN_NAMES[1:], errs, e_cpu[1:]):
        _bound(nm, e, c)


def test_mod_batch_norm_is_first_order_and_checks_its_arguments():
    from gan_lab_amd import ops
    x = torch.randn(2, 3, 4, 4).cuda().requires_grad_(True)
    gain, shift = torch.ones(2, 3).cuda().requires_grad_(True), torch.zeros(2, 3).cuda()
    rm, rv = torch.zeros(3).cuda(), torch.ones(3).cuda()
    y = ops.mod_batch_norm(x, gain, shift, rm, rv, True)
    gx, = torch.autograd.grad(y.square().sum(), x, create_graph=True)      # a head whose cotangent depends on x
    with pytest.raises((NotImplementedError, RuntimeError), match='differentiate|once_differentiable|second'):
        torch.autograd.grad(gx.sum(), x)
    with pytest.raises(ValueError, match='gain'):
        ops.mod_batch_norm(x, torch.ones(3, 3).cuda(), shift, rm, rv, True)
    with pytest.raises(ValueError, match='shift'):
        ops.mod_batch_norm(x, gain, torch.zeros(3, 2).cuda().t(), rm, rv, True)
    with pytest.raises(TypeError, match='GPU'):
        ops.mod_batch_norm(x, gain.cpu(), shift, rm, rv, True)


def test_two_runs_are_bit_equal():
    for slope in (None, 0.2):
        inputs, _, _ = _mbn_case((4, 8, 8, 8))
        a, b = _mbn_gpu(*inputs, act_slope=slope), _mbn_gpu(*inputs, act_slope=slope)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    inputs, _, _ = _mbn_case((2, 64, 32, 32))
    assert all(torch.equal(s, t) for s, t in zip(_mbn_gpu(*inputs), _mbn_gpu(*inputs)))
    for name in ('both_d153', 'both_nine_jobs'):
        inputs, _, _ = _mod_case(name)
        a, b = _mod_gpu(*inputs)[0], _mod_gpu(*inputs)[0]
        assert all(torch.equal(s, t) for s, t in zip(a, b) if s is not None)


# ---- the networks ----------------------------------------------------------------------------------------------------------
NETS = [('Generator64PixResnet', dict(fmap=8, len_latent=21)), ('Generator32PixResnet', dict(fmap=16, len_latent=13))]
KN = 3


def _net(name, kw, seed, **opts):
    from gan_lab_amd.resnetgan import architectures as A
    torch.manual_seed(seed)
    net = getattr(A, name)(cgan=True, num_classes=KN, hier_latent=True, shared_embed=8, **opts, **kw)
    with torch.no_grad():                            # non-trivial affines of the last norm
        for k_, p in net.named_parameters():
            if k_.endswith(('norm.weight', 'norm.bias')):
                p.add_(0.3 * torch.randn_like(p))
    return net.cuda().train()


@pytest.mark.parametrize('name,kw', NETS, ids=[n for n, _ in NETS])
def test_networks_against_the_reference_composition(name, kw):
    net = _net(name, kw, 31)
    g = torch.Generator().manual_seed(32)
    z = torch.randn(3, kw['len_latent'], generator=g).cuda().requires_grad_(True)
    labels = torch.tensor([2, 0, 2], dtype=torch.int32).cuda()
    y = net(z, labels)
    cot = torch.randn(*y.shape, generator=g).cuda()
    y.backward(cot)
    got = {k_: p.grad.clone() for k_, p in net.named_parameters()}
    got_z = z.grad.clone()
    assert all(m.mod is None for m, _, _ in net.hier.norms)                 # cleared after the forward
    # the reference composition in float64 on the same parameters
    ref_net = _net(name, kw, 31).double()
    ref_net.load_state_dict({k_: v.double() for k_, v in net.state_dict().items()})
    zr = z.detach().double().requires_grad_(True)
    yr = ref.generator(ref_net, zr, labels)
    yr.backward(cot.double())
    e = rel_err(y.detach(), yr.detach())
    print(f'{name}: image {e:.2e}')
    assert e <= TOL
    # the measure of tests/test_gpu_resnet.py (_cmp_grads): a block's conv biases sit in front of a BatchNorm, their exact
    # gradient is zero and what either side holds there is rounding noise - judged against the largest gradient of the network
    gmax = max(float(p.grad.abs().max()) for p in ref_net.parameters())
    worst = ('', 0.0)
    for k_, p in ref_net.named_parameters():
        den = gmax if resnet_zero_grad_key(k_) else max(float(p.grad.abs().max()), 1e-4 * gmax)
        e = float((got[k_].double() - p.grad).abs().max()) / den
        worst = max(worst, (k_, e), key=lambda t: t[1])
        assert e <= TOL, (k_, e)
    print(f'{name}: worst parameter gradient {worst[0]} {worst[1]:.2e}; z {rel_err(got_z, zr.grad):.2e}')
    assert rel_err(got_z, zr.grad) <= TOL
    first, chunks = ref.chunk_layout(kw['len_latent'], len(net.hier.norms) // 2)
    for lo, n_ in [(0, first)] + chunks:                                   # the latent reaches every consumer
        assert bool((got_z[:, lo:lo + n_] != 0).any()), lo
    assert bool((got['shared.weight'][1] == 0).all()) and bool((got['shared.weight'][0] != 0).any())      # class 1 is absent
    with pytest.raises(TypeError, match='labels'):
        net(z)
    # eval mode, and a label moves its own sample only
    net.eval()
    with torch.no_grad():
        ya, yb = net(z, labels), net(z, torch.tensor([2, 1, 2], dtype=torch.int32).cuda())
    assert torch.equal(ya[0], yb[0]) and torch.equal(ya[2], yb[2]) and not torch.equal(ya[1], yb[1])


def test_generator_forward_and_backward_replay_from_a_graph():
    """No host readback, no upload: forward + backward of a modulated generator captured with torch.cuda.graph replay to the bits
    of the eager run (the job table was uploaded by the eager run)."""
    name, kw = NETS[1]
    net = _net(name, kw, 41)
    g = torch.Generator().manual_seed(42)
    z = torch.randn(3, kw['len_latent'], generator=g).cuda().requires_grad_(True)
    labels = torch.tensor([2, 0, 1], dtype=torch.int32).cuda()
    params = [p for p in net.parameters()]
    cot = torch.randn(3, 3, 32, 32, generator=g).cuda()
    counters = [b for k_, b in net.named_buffers() if k_.endswith('num_batches_tracked')]

    def run():
        y = net(z, labels)
        return (y,) + torch.autograd.grad(y, [z] + params, cot)

    eager = [t.detach().clone() for t in run()]
    state = {k_: v.clone() for k_, v in net.state_dict().items()}
    net.load_state_dict(_net(name, kw, 41).state_dict())                     # the running statistics back to their start
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.detach().zero_()                       # a capture records, it does not run
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b.detach())
    for k_, v in net.state_dict().items():
        assert torch.equal(v, state[k_]), k_
    assert all(int(c) == 1 for c in counters)


# ---- the learner -----------------------------------------------------------------------------------------------------------
BIGGAN = dict(cgan='projection', num_classes=3, shared_embed=8, hier_latent=True, spectral_norm=True, loss='hinge',
              gradient_penalty=None, ortho_reg=1e-4)


def _learner(**kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    kw.setdefault('random_seed', 7)
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=1, len_latent=32, **kw)
    cfg.fmap_g, cfg.fmap_d = 16, 16
    torch.manual_seed(7)
    return GANLearner(cfg)


def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).cuda(), torch.randn(4, 32, generator=g).cuda(), \
        torch.randn(4, 32, generator=g).cuda(), torch.tensor([0, 2, 2, 0])


def _mod_params(L):
    return {k_: p for k_, p in L.gen_model.named_parameters() if '.gain.' in k_ or '.shift.' in k_ or k_ == 'shared.weight'}


def _steps(L, seed=0):
    real, zd, zg, labels = _batch(seed)
    lab = labels if L.cgan else None
    L.set_requires_grad_disc(True)
    ld = L.d_step(real, zb=zd, labels=lab)
    L.set_requires_grad_disc(False)
    lg = L.g_step(zb=zg, labels=lab)
    L.set_requires_grad_disc(True)
    return float(ld), float(lg)


def test_learner_biggan_recipe(tmp_path):
    L = _learner(**BIGGAN)
    assert L.gen_model.hier.table is not None and L.gen_model.hier.table.in_arena        # uploaded with the arena
    assert len(_mod_params(L)) == 13 and 'shared.weight' not in L.ortho_g.names
    assert sum('.gain.' in k_ or '.shift.' in k_ for k_ in L.ortho_g.names) == 12
    before = {k_: p.detach().clone() for k_, p in _mod_params(L).items()}
    real, zd, zg, labels = _batch(0)
    L.set_requires_grad_disc(False)
    lg = float(L.g_step(zb=zg, labels=labels))
    grads = {k_: p.grad.detach().clone() for k_, p in _mod_params(L).items()}
    L.set_requires_grad_disc(True)
    ld = float(L.d_step(real, zb=zd, labels=labels))
    print('losses', lg, ld)
    assert np.isfinite(lg) and np.isfinite(ld)
    for k_, p in _mod_params(L).items():
        assert bool((grads[k_] != 0).any()), k_                              # received a gradient ...
        assert not torch.equal(p.detach(), before[k_]), k_                   # ... and moved
    assert bool((grads['shared.weight'][1] == 0).all())                      # class 1 is absent from the batch
    # save / load restores the embedding and the modulation weights bitwise, and training goes on identically
    L.not_trained_yet = False
    path = tmp_path / 'resnetgan_model.tar'
    L.save_model(path)
    with pytest.raises(ValueError, match='reference_format'):
        L.save_model(path, reference_format=True)
    L2 = _learner(**BIGGAN)
    L2.load_model(path)
    L2.gen_model.train()
    L2.disc_model.train()
    for (k_, p), (_, p2) in zip(L.gen_model.state_dict().items(), L2.gen_model.state_dict().items()):
        assert torch.equal(p, p2), k_
    assert L2.gen_model.hier.table.is_current() and L2.gen_model.hier.table.in_arena
    a, b = _steps(L, 1), _steps(L2, 1)
    assert a == b, (a, b)
    for (k_, p), (_, p2) in zip(L.gen_model.named_parameters(), L2.gen_model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), k_


def test_learner_generator_step_replays_from_a_graph():
    """The generator step - forward, backward into the arena, ortho_reg, Adam - captured with torch.cuda.graph on one learner
    ends bitwise where the eager step of an identically built learner ends (default queue settings, no overrides)."""
    La, Lb = _learner(**BIGGAN), _learner(**BIGGAN)
    _, _, zg, labels = _batch(0)
    lab = labels.int().cuda()
    for L in (La, Lb):
        L.set_requires_grad_disc(False)
        L.g_step(zb=zg, labels=lab)              # the first step (packs weights, builds Adam's state) runs eagerly on both
    _, _, zg2, _ = _batch(1)
    La.g_step(zb=zg2, labels=lab)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Lb.g_step(zb=zg2, labels=lab)
    graph.replay()
    torch.cuda.synchronize()
    for (k_, p), (_, p2) in zip(La.gen_model.state_dict().items(), Lb.gen_model.state_dict().items()):
        if not k_.endswith('num_batches_tracked'):
            assert torch.equal(p, p2), k_
    assert torch.equal(La.arena_g.gflat, Lb.arena_g.gflat)


def test_learner_self_modulation_takes_a_step():
    """hier_latent without labels (Chen et al. 2019): the unconditional pair, default loss and penalty."""
    L = _learner(hier_latent=True)
    assert L.cgan is False and L.gen_model.shared_embed == 0
    before = {k_: p.detach().clone() for k_, p in _mod_params(L).items()}
    assert len(before) == 12
    losses = _steps(L)
    print('losses', losses)
    assert all(np.isfinite(losses))
    for k_, p in _mod_params(L).items():
        assert not torch.equal(p.detach(), before[k_]), k_
    with pytest.raises(TypeError, match='labels'):
        L.gen_model(torch.randn(4, 32).cuda(), torch.zeros(4, dtype=torch.int32).cuda())
