"""GPU tests of BigGAN's orthogonal regulariser (csrc/ortho.hip, gan_lab_amd/ortho_reg.py): the batched kernels against the
float64 reference (tests/ortho_reference.py) on a job table with awkward shapes, the diagonal mask, the scaling with beta,
bitwise reproducibility, graph capture, and the learner's generator / critic steps with and without the option.

Bounds.  Gradient: max|err| / max|ref| <= 1e-5 per layer; penalty: relative error <= 1e-5 per layer and for the total.  A CPU
fp32 restatement of both forms on exactly these shapes (ATen CPU, seed 0), in the form each shape uses, stays below 7.8e-7 on
the gradient (worst: (2048, 128), column form) and below 2.1e-7 on the penalty, so 1e-5 leaves ~13x for another summation
order while a wrong tail, mask, offset or form is O(1) - the margin of tests/test_gpu_sn.py."""
import pytest
import torch

import ortho_reference as ref
from util import rel_err

pytestmark = pytest.mark.gpu
BOUND = 1e-5
BETA = 1e-2
# (R, K): skipped | one partial tile (x2) | the generator's last conv | column form, K % 4 != 0 | both tails | column form |
# row form | many tiles, longest contraction | column form, R / K = 16
SHAPES = [(1, 64), (2, 3), (5, 7), (3, 576), (64, 27), (33, 130), (128, 64), (128, 576), (512, 4608), (2048, 128)]
GAP = 8       # floats between two slots (keeps them 16-byte aligned)
OUTSIDE = 40  # a slot of the arena that belongs to no regularised layer (a bias, say)


class _Table(object):
    """A job table over a hand-made parameter / gradient arena: NaN between the slots of the parameters, random values in
    the whole gradient arena (the kernels accumulate, and must leave everything outside their slots alone)."""

    def __init__(self, shapes, seed=0, weights=None):
        from gan_lab_amd import ops
        g = torch.Generator().manual_seed(seed)
        self.shapes = shapes
        self.off = []
        o = GAP + OUTSIDE + GAP
        for r, k in shapes:
            self.off.append(o)
            o += (r * k + 3) // 4 * 4 + GAP
        self.W = torch.full((o,), float('nan'), device='cuda')
        self.gW = torch.empty(o, device='cuda')
        self.inside = torch.zeros(o, dtype=torch.bool)
        self.W0 = [(weights[i].float() if weights is not None else torch.randn(r, k, generator=g) * (2.0 / k) ** 0.5)
                   for i, (r, k) in enumerate(shapes)]
        self.G0 = torch.randn(o, generator=g)
        self.jobs = []
        for (r, k), of in zip(shapes, self.off):
            self.inside[of:of + r * k] = True
            self.jobs.append(dict(w=self.W[of:of + r * k].view(r, k), gw=self.gW[of:of + r * k]))
        self.reset()
        self.table = ops.OrthoTable(self.jobs)

    def reset(self, zero=False):
        for j, w in zip(self.jobs, self.W0):
            j['w'].copy_(w)
        self.gW.zero_() if zero else self.gW.copy_(self.G0)
        if hasattr(self, 'table'):          # every result a kernel owes is poisoned; a skipped layer's penalty stays 0
            self.table.penalties.fill_(float('nan'))
            for i, e in enumerate(self.table.plan):
                if e is None:
                    self.table.penalties[i] = 0.

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone().view(torch.int32) for b in (self.gW, self.table.penalties, self.W)]


@pytest.fixture(scope='module')
def table():
    return _Table(SHAPES)


@pytest.fixture(scope='module')
def reference(table):
    """[(penalty, gradient)] in float64 by autograd of the literal penalty, computed once."""
    return [ref.gradient(w, BETA) for w in table.W0]


def _cmp(what, a, b):
    e = rel_err(a, b)
    print(f'{what}: rel err {e:.3e}')
    assert e <= BOUND, f'{what}: rel err {e:.3e} > {BOUND:.0e}'


def _cmp_scalar(what, got, want):
    e = abs(float(got) - float(want)) / abs(float(want))
    print(f'{what}: rel err {e:.3e}')
    assert e <= BOUND, f'{what}: {float(got)!r} vs {float(want)!r}: rel err {e:.3e} > {BOUND:.0e}'


def test_batched_apply(table, reference):
    """One apply into a gradient arena pre-filled with random values.  What the arena then holds is compared with (pre-fill +
    float64 gradient): the bound is the gradient's 1e-5 * max|ref| plus one fp32 rounding (2^-24 relative) of the largest sum,
    which the accumulation into O(1) values costs whatever the kernel does - the learner test's rule (1e-5 * max|arena|) is the
    looser one.  test_gradient_into_a_zeroed_arena asserts the plain 1e-5 on the gradient alone."""
    from gan_lab_amd import _lib, ops
    T = table
    T.reset()
    w_before = T.W.clone().view(torch.int32)
    n0 = _lib.launch_count()
    ops.ortho_apply(T.table, BETA)
    assert _lib.launch_count() - n0 == 3          # whatever the number of layers
    syms = [s or '' for s, _ in _lib.launches_since(n0)]
    assert all('ortho_' in s for s in syms), syms
    torch.cuda.synchronize()
    gW = T.gW.cpu()
    total = 0.0
    for i, ((r, k), of, (pen, grad)) in enumerate(zip(SHAPES, T.off, reference)):
        if r == 1:
            assert T.table.plan[i] is None
            assert torch.equal(gW[of:of + r * k], T.G0[of:of + r * k]), 'a one-row layer has no gradient: exactly 0'
            assert T.table.penalties[i].item() == 0.0
            continue
        want_sum = T.G0[of:of + r * k].view(r, k).double() + grad
        err = (gW[of:of + r * k].view(r, k).double() - want_sum).abs().max().item()
        slack = 2.0 ** -24 * want_sum.abs().max().item()
        print(f'gW += {r}x{k}: err {err:.3e} (|grad| {grad.abs().max().item():.3e})')
        assert err <= BOUND * grad.abs().max().item() + slack, (r, k, err)
        _cmp_scalar(f'penalty {r}x{k}', T.table.penalties[i], pen)
        total += pen.item()
    _cmp_scalar('total penalty', T.table.total, total)
    # everything outside the regularised slots - the gaps, the slot of another parameter - keeps its bits; so do the weights
    assert torch.equal(gW[~T.inside].view(torch.int32), T.G0[~T.inside].view(torch.int32))
    assert torch.equal(T.W.view(torch.int32), w_before)


def test_gradient_into_a_zeroed_arena(table, reference):
    """The gradient alone, against float64: max|err| / max|ref| <= 1e-5 per layer."""
    from gan_lab_amd import ops
    T = table
    T.reset(zero=True)
    ops.ortho_apply(T.table, BETA)
    for (r, k), j, (_, grad) in zip(SHAPES, T.jobs, reference):
        if r == 1:
            assert not j['gw'].any()
        else:
            _cmp(f'gW {r}x{k}', j['gw'].view(r, k), grad)


def test_diagonal_is_masked():
    """Orthogonal rows of unequal norms: Wm Wm^T is diagonal and not a multiple of I - the gradient and the penalty are exactly 0
    only if the diagonal is really left out.  (8, 16) takes the row form (the mask at the store); (16, 8) with eight more rows
    of zeros the column form (the q terms)."""
    from gan_lab_amd import ops
    W = torch.zeros(8, 16)
    W[:, :8] = torch.diag(torch.arange(1., 9.))
    T = _Table([(8, 16)], weights=[W])
    T.reset(zero=True)
    ops.ortho_apply(T.table, 0.5)
    torch.cuda.synchronize()
    assert not T.gW.any() and T.table.penalties[0].item() == 0.0 and T.table.total.item() == 0.0
    W2 = torch.zeros(16, 8)
    W2[:8] = torch.diag(torch.arange(1., 9.))
    T2 = _Table([(16, 8)], weights=[W2])
    T2.reset(zero=True)
    ops.ortho_apply(T2.table, 0.5)
    torch.cuda.synchronize()
    assert not T2.gW.any() and T2.table.penalties[0].item() == 0.0      # small integers: Wm S - q o Wm cancels exactly


def test_beta_scales_exactly(table):
    from gan_lab_amd import ops
    T = table
    out = []
    for beta in (BETA, 2 * BETA):
        T.reset(zero=True)
        ops.ortho_apply(T.table, beta)
        torch.cuda.synchronize()
        out.append((T.gW.clone(), T.table.penalties.clone()))
    (g1, p1), (g2, p2) = out
    assert torch.equal((2 * g1).view(torch.int32), g2.view(torch.int32))
    assert torch.equal((2 * p1).view(torch.int32), p2.view(torch.int32))
    assert float(g1.abs().max()) > 0 and float(p1[-1]) > 0


def test_bitwise_reproducible(table):
    from gan_lab_amd import ops
    T = table
    runs = []
    for _ in range(2):
        T.reset()
        ops.ortho_apply(T.table, BETA)
        runs.append(T.snapshot())
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_apply_replays_from_a_graph(table):
    """Everything is device-resident (no host read, no allocation, no upload): a captured apply replays to the bits of the
    eager call."""
    from gan_lab_amd import ops
    T = table
    T.reset()
    ops.ortho_apply(T.table, BETA)
    eager = T.snapshot()
    T.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ortho_apply(T.table, BETA)
    T.reset()               # a capture records, it does not run
    graph.replay()
    for a, b in zip(eager, T.snapshot()):
        assert torch.equal(a, b)


def test_argument_checks(table):
    from gan_lab_amd import ops
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='beta'):
            ops.ortho_apply(table.table, bad)
    with pytest.raises(TypeError, match='GPU'):
        ops.OrthoTable([dict(w=torch.zeros(4, 4), gw=torch.zeros(16))])
    with pytest.raises(ValueError, match='16-byte'):
        buf = torch.zeros(64, device='cuda')
        ops.OrthoTable([dict(w=buf[1:17].view(4, 4), gw=buf[32:48])])


# ---------------------------------------------------------------------------------------------------------------------- #
def _learner(**kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=2, random_seed=7, len_latent=32,
                      cgan='projection', num_classes=3, self_attention='g', **kw)
    cfg.fmap_g, cfg.fmap_d = 32, 32
    torch.manual_seed(7)
    L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    return L


def _inputs():
    g = torch.Generator().manual_seed(3)
    real = (torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).cuda()
    z = torch.randn(4, 32, generator=g).cuda()
    labels = torch.tensor([0, 2, 1, 2], dtype=torch.int32).cuda()
    return real, z, labels


def _step(L, which):
    """One step of a fresh learner.  -> (parameter arena before the step, gradient arena after it), both on the CPU."""
    real, z, labels = _inputs()
    arena = L.arena_g if which == 'g' else L.arena_d
    before = arena.flat.detach().cpu().clone()
    L.set_requires_grad_disc(which == 'd')
    if which == 'g':
        L.g_step(zb=z, labels=labels)
    else:
        L.d_step(real, zb=z, labels=labels)
    torch.cuda.synchronize()
    return before, arena.gflat.detach().cpu().clone()


@pytest.mark.parametrize('which', ['g', 'd'])
def test_learner_step_adds_the_reference_gradient(which):
    """Two learners with identical seeds, one with the regulariser: the gradient arenas after one step on the same inputs differ
    by the float64 gradient of the weights the step started from (the raw W under spectral normalisation) on every regularised
    key, and by exactly nothing on every other key."""
    beta = 1e-2
    kw = {} if which == 'g' else dict(spectral_norm=True, loss='hinge', gradient_penalty=None)
    field, attr = ('ortho_reg', 'ortho_g') if which == 'g' else ('ortho_reg_d', 'ortho_d')
    A = _learner(**{field: beta}, **kw)
    reg = getattr(A, attr)
    assert reg is not None and getattr(A, 'ortho_d' if which == 'g' else 'ortho_g') is None
    before_a, g_a = _step(A, which)
    logged = A.last_losses[attr]
    assert isinstance(logged, torch.Tensor) and logged.is_cuda and logged.numel() == 1
    arena = A.arena_g if which == 'g' else A.arena_d
    B = _learner(**kw)
    before_b, g_b = _step(B, which)
    assert torch.equal(before_a, before_b), 'the two learners did not start from the same weights'
    named = dict((A.gen_model if which == 'g' else A.disc_model).named_parameters())
    assert set(reg.names) == {k for k in named if k.endswith(('conv2d.weight', 'linear.weight'))}
    total, per_layer = 0.0, reg.per_layer()
    for k, off, n in zip(arena.names, arena.offsets, arena.sizes):
        diff = g_a[off:off + n].double() - g_b[off:off + n].double()
        if k not in reg.names:
            assert not diff.any(), f'{k}: not regularised, but its gradient changed'
            continue
        pen, grad = ref.gradient(before_a[off:off + n].view(named[k].shape), beta)
        tol = BOUND * g_a[off:off + n].abs().max().item()
        err = (diff - grad.reshape(-1)).abs().max().item()
        print(f'{k} {tuple(named[k].shape)}: err {err:.3e} tol {tol:.3e} |grad| {grad.abs().max().item():.3e}')
        assert err <= tol, f'{k}: {err:.3e} > {tol:.3e}'
        if pen.item() > 0:
            _cmp_scalar(f'penalty {k}', per_layer[k], pen)
        else:
            assert per_layer[k].item() == 0.0
        total += pen.item()
    _cmp_scalar('logged penalty', logged, total)
    assert total > 0


def test_default_learner_is_untouched():
    """Both strengths 0 (the default): no manager, and a generator and a critic step launch nothing of ortho.hip."""
    from gan_lab_amd import _lib
    L = _learner()
    assert L.ortho_g is None and L.ortho_d is None
    handle, calls, seen = _lib.lib(), [], []
    saved = {name: getattr(handle, name) for name in _lib.SIGNATURES
             if name not in ('ganlab_last_launch', 'ganlab_launch_count', 'ganlab_launch_history')}
    count = handle.ganlab_launch_count

    def wrap(name, fn):
        def wrapped(*a):
            before = int(count())
            rc = fn(*a)
            calls.append(name)
            seen.extend(s or '' for s, _ in _lib.launches_since(before))
            return rc
        return wrapped

    for name, fn in saved.items():
        setattr(handle, name, wrap(name, fn))
    try:
        _step(L, 'g')
        _step(L, 'd')
    finally:
        for name, fn in saved.items():
            setattr(handle, name, fn)
    assert len(calls) > 20 and len(seen) > 20          # the observer saw the step
    assert 'ganlab_ortho_apply' not in calls
    assert not [s for s in seen if 'ortho' in s]
    assert 'ortho_g' not in L.last_losses and 'ortho_d' not in L.last_losses


def test_manager_refuses_a_detached_arena():
    from gan_lab_amd.optim import ParamArena
    from gan_lab_amd.ortho_reg import OrthoReg
    from gan_lab_amd.resnetgan.architectures import Generator32PixResnet
    torch.manual_seed(1)
    g = Generator32PixResnet(fmap=32, len_latent=32).cuda()
    arena = ParamArena(g.named_parameters(), 'cuda')
    reg = OrthoReg(g, arena, 1e-3)
    reg.apply()
    assert float(reg.penalty) > 0 and set(reg.per_layer()) == set(reg.names)
    with pytest.raises(ValueError, match='arena'):
        OrthoReg(g, ParamArena(Generator32PixResnet(fmap=32, len_latent=32).cuda().named_parameters(), 'cuda'), 1e-3)
    p = next(g.parameters())
    p.data = p.data.clone()                 # what model.to('cpu') and back does
    with pytest.raises(RuntimeError, match='OrthoReg'):
        reg.apply()
