"""GPU tests of the classifier-based class conditioning (csrc/cond_loss.hip; gan_lab_amd/conditional.py):
``ops.class_cross_entropy``, ``ops.class_contrastive`` in both modes, the learner with ``config.cgan`` = 'contra' / 'reacgan', and
a critic with AC-GAN's head on its own (``config.cgan='acgan'`` is still refused, so no learner runs it).

Op bound, per tensor: ``rel_err <= max(1e-5, 16 * e_cpu)`` where ``e_cpu`` is the error of the reference (cc_reference.py) run in
fp32 on the CPU against its own float64 run on the same inputs - the rule of tests/test_gpu_cond.py.  Network bound: TOL = 1e-3
of tests/test_gpu_resnet.py, with its denominator (the reference's largest magnitude, floored at 1e-4 of the network's largest
gradient).  Clamp kinks are never judged: every D2D-CE case asserts on its float64 reference that no similarity lies within
1e-4 of a margin (the seeds were picked on the CPU so that it holds; a violated condition fails, it does not skip).

Measured errors: DESIGN.md 4.20; every test prints its figures before it asserts.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import cc_reference as ref
from util import rel_err, resnet_zero_grad_key

pytestmark = pytest.mark.gpu

TOL = 1e-3
G_OUT = 0.7                 # the cotangent of the loss
KINK = 1e-4
# (N, K), labels (None: drawn)
CE_CASES = [((1, 2), None), ((7, 3), (0, 2, 2, 0, 2, 0, 0)), ((64, 10), None), ((33, 1000), None)]
# (N, E, K), labels (None: drawn), {mode: seed} - seeds for which the D2D-CE case is clear of its kinks (checked by the test)
CL_CASES = [((1, 8, 2), None, {'2c': 0, 'd2d': 0}),
            ((7, 12, 3), (0, 2, 2, 0, 2, 0, 0), {'2c': 0, 'd2d': 0}),
            ((64, 256, 10), None, {'2c': 0, 'd2d': 273}),
            ((130, 40, 4), None, {'2c': 0, 'd2d': 30}),
            ((65, 1024, 5), None, {'2c': 0, 'd2d': 299})]
MARGINS = dict(margin_pos=0.98, margin_neg=0.02)
SPREAD = ((130, 8, 4), dict(margin_pos=0.1, margin_neg=0.05), 13)       # shape, margins, seed: every clamp state occurs
_ids = lambda cases: ['x'.join(map(str, c[0])) for c in cases]      # noqa: E731


def _bound(name, e, c):
    assert e <= max(1e-5, 16 * c), f'{name}: {e:.3e} > max(1e-5, 16 * {c:.3e})'


def make_inputs(shape, labels, seed):
    """(h, proxy, labels) on the CPU in fp32: embeddings that lean towards their class's proxy."""
    n, e, k = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + e)
    proxy = torch.randn(k, e, generator=g)
    labels = torch.tensor(labels, dtype=torch.int32) if labels is not None else \
        torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    h = (torch.randn(n, e, generator=g) + 0.7 * proxy[labels.long()]) * 1.3
    return h, proxy, labels


def kink_distance(h, proxy, labels, margin_pos, margin_neg):
    """Smallest distance of an off-diagonal similarity from m_n and of a proxy similarity from m_p, in float64."""
    s, S = ref.similarities(h, proxy, labels, torch.float64)
    off = ~torch.eye(len(s), dtype=torch.bool)
    d_n = float((S[off] - margin_neg).abs().min()) if len(s) > 1 else float('inf')
    return min(d_n, float((s - margin_pos).abs().min()))


@functools.lru_cache(maxsize=None)
def _cl_case(shape, labels, mode, seed, margins=tuple(MARGINS.items()), temperature=0.5):
    """Inputs (CPU fp32), the float64 reference (loss, rows, dh, dproxy) and e_cpu of each; computed once, never modified."""
    h, proxy, lab = make_inputs(shape, labels, seed)
    kw = dict(mode=mode, temperature=temperature, **dict(margins))
    want = ref.contrastive_with_grads(h, proxy, lab, G_OUT, torch.float64, **kw)
    cpu = ref.contrastive_with_grads(h, proxy, lab, G_OUT, torch.float32, **kw)
    return (h, proxy, lab), kw, want, [rel_err(a, b) for a, b in zip(cpu, want)]


def _cl_gpu(h, proxy, lab, kw, scale=1.0):
    from gan_lab_amd import ops
    h, proxy = (h * scale).cuda().requires_grad_(True), proxy.cuda().requires_grad_(True)
    loss, rows = ops.class_contrastive(h, proxy, lab.cuda(), return_rows=True, **kw)
    dh, dp = torch.autograd.grad(loss * G_OUT, (h, proxy))
    return loss.detach(), rows, dh, dp


def _assert_clear_of_kinks(inputs, kw):
    d = kink_distance(*inputs, kw['margin_pos'], kw['margin_neg'])
    print(f'distance from the nearest clamp kink {d:.2e}')
    assert d >= KINK, f'this case sits {d:.2e} from a clamp kink: pick another seed'


NAMES = ('loss', 'rows', 'dh', 'dproxy')


def _check_against_float64(shape, labels, mode, seed, **case_kw):
    inputs, kw, want, e_cpu = _cl_case(shape, labels, mode, seed, **case_kw)
    if mode == 'd2d':
        _assert_clear_of_kinks(inputs, kw)
    got = _cl_gpu(*inputs, kw)
    errs = [rel_err(a, b) for a, b in zip(got, want)]
    print(f'{mode} {shape}: ' + ' '.join(f'{nm} gpu {e:.2e} cpu {c:.2e}' for nm, e, c in zip(NAMES, errs, e_cpu)))
    for nm, e, c in zip(NAMES, errs, e_cpu):
        _bound(nm, e, c)
    present = set(inputs[2].tolist())
    for k in range(shape[2]):
        if k not in present:                         # a class absent from the batch: a row of exact zeros, written
            assert bool((got[3][k] == 0).all()), k
    return inputs, kw, want, e_cpu, got


# ---- cross-entropy ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ce_case(shape, labels):
    n, k = shape
    g = torch.Generator().manual_seed(31 * n + k)
    z = torch.randn(n, k, generator=g) * 3.0
    labels = torch.tensor(labels, dtype=torch.int32) if labels is not None else \
        torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    want = ref.cross_entropy_with_grads(z, labels, G_OUT, torch.float64)
    cpu = ref.cross_entropy_with_grads(z, labels, G_OUT, torch.float32)
    return (z, labels), want, [rel_err(a, b) for a, b in zip(cpu, want)]


def _ce_gpu(z, labels):
    from gan_lab_amd import ops
    z = z.cuda().requires_grad_(True)
    loss = ops.class_cross_entropy(z, labels.cuda())
    dz, = torch.autograd.grad(loss * G_OUT, z)
    return loss.detach(), dz


@pytest.mark.parametrize('shape,labels', CE_CASES, ids=_ids(CE_CASES))
def test_cross_entropy_against_float64(shape, labels):
    inputs, want, e_cpu = _ce_case(shape, labels)
    loss, dz = _ce_gpu(*inputs)
    errs = [rel_err(loss, want[0]), rel_err(dz, want[2])]
    print(f'ce {shape}: loss gpu {errs[0]:.2e} cpu {e_cpu[0]:.2e}  dz gpu {errs[1]:.2e} cpu {e_cpu[2]:.2e}')
    _bound('loss', errs[0], e_cpu[0])
    _bound('dz', errs[1], e_cpu[2])
    assert torch.equal(loss, _ce_gpu(*inputs)[0]) and torch.equal(dz, _ce_gpu(*inputs)[1])      # two runs, the same bits
    if labels is not None:
        assert 1 not in set(inputs[1].tolist())      # the case with an absent class
        assert bool((dz[:, 1] > 0).all())            # ... whose column is pure softmax mass


def test_cross_entropy_is_first_order_and_checks_its_arguments():
    from gan_lab_amd import ops
    (z, labels), _, _ = _ce_case((7, 3), (0, 2, 2, 0, 2, 0, 0))
    z = z.cuda().requires_grad_(True)
    g, = torch.autograd.grad(ops.class_cross_entropy(z, labels.cuda()), z, create_graph=True)
    with pytest.raises(RuntimeError, match='first order'):
        g.sum().backward()
    with pytest.raises(ValueError):
        ops.class_cross_entropy(torch.zeros(4, 1).cuda(), torch.zeros(4, dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        ops.class_cross_entropy(torch.zeros(4, 3).cuda(), torch.zeros(5, dtype=torch.int32).cuda())


# ---- contrastive ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['2c', 'd2d'])
@pytest.mark.parametrize('shape,labels,seeds', CL_CASES, ids=_ids(CL_CASES))
def test_contrastive_against_float64(shape, labels, seeds, mode):
    inputs, kw, want, e_cpu, got = _check_against_float64(shape, labels, mode, seeds[mode])
    if labels is not None:
        assert 1 not in set(inputs[2].tolist())      # the case with an absent class
    again = _cl_gpu(*inputs, kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again))      # two runs, the same bits
    # h -> 3 h: the loss stays, dh is divided by 3
    scaled = _cl_gpu(*inputs, kw, scale=3.0)
    e_loss, e_dh = rel_err(scaled[0], want[0]), rel_err(scaled[2], want[2] / 3.0)
    print(f'3h: loss {e_loss:.2e} dh {e_dh:.2e}')
    _bound('loss of 3h', e_loss, e_cpu[0])
    _bound('dh of 3h', e_dh, e_cpu[2])


def test_d2d_with_every_clamp_state():
    shape, margins, seed = SPREAD
    inputs, kw, _, _, _ = _check_against_float64(shape, None, 'd2d', seed, margins=tuple(margins.items()))
    s, S = ref.similarities(*inputs, torch.float64)
    y = inputs[2].long()
    neg = S[y[:, None] != y[None, :]]
    states = dict(s_below=int((s < kw['margin_pos']).sum()), s_above=int((s > kw['margin_pos']).sum()),
                  S_above=int((neg > kw['margin_neg']).sum()), S_below=int((neg < kw['margin_neg']).sum()))
    print(states)
    assert all(v > 0 for v in states.values()), states


def test_a_row_without_negatives_costs_nothing():
    """D2D-CE with every label equal: each row's loss is exactly 0 and so is every gradient."""
    h, proxy, _ = make_inputs((9, 12, 3), None, 1)
    lab = torch.full((9,), 2, dtype=torch.int32)
    loss, rows, dh, dp = _cl_gpu(h, proxy, lab, dict(mode='d2d', temperature=0.5, **MARGINS))
    assert float(loss) == 0 and bool((rows == 0).all()) and bool((dh == 0).all()) and bool((dp == 0).all())


def test_contrastive_is_first_order_and_checks_its_arguments():
    from gan_lab_amd import ops
    h, proxy, lab = make_inputs((7, 12, 3), None, 0)
    h, proxy, lab = h.cuda().requires_grad_(True), proxy.cuda().requires_grad_(True), lab.cuda()
    for mode in ('2c', 'd2d'):
        g, = torch.autograd.grad(ops.class_contrastive(h, proxy, lab, mode=mode), h, create_graph=True)
        with pytest.raises(RuntimeError, match='first order'):
            g.sum().backward()
    with pytest.raises(ValueError, match='mode'):
        ops.class_contrastive(h, proxy, lab, mode='3c')
    with pytest.raises(ValueError, match='temperature'):
        ops.class_contrastive(h, proxy, lab, temperature=0.0)
    with pytest.raises(ValueError, match='E'):
        ops.class_contrastive(torch.zeros(4, 1025).cuda(), torch.zeros(3, 1025).cuda(), torch.zeros(4, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match='K'):
        ops.class_contrastive(torch.zeros(4, 8).cuda(), torch.zeros(1, 8).cuda(), torch.zeros(4, dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        ops.class_contrastive(h, proxy[:, :5], lab)


def test_forward_launch_counts_do_not_depend_on_the_shape():
    """The library counts the launches of the calling thread: the forwards (the backward runs on autograd's own thread)."""
    from gan_lab_amd import _lib, ops
    for shape in ((7, 12, 3), (130, 40, 4)):
        h, proxy, lab = make_inputs(shape, None, 0)
        h, proxy, lab = h.cuda(), proxy.cuda(), lab.cuda()
        c0 = _lib.launch_count()
        ops.class_contrastive(h, proxy, lab, mode='d2d')
        c1 = _lib.launch_count()
        ops.class_cross_entropy(h, lab)
        c2 = _lib.launch_count()
        assert (c1 - c0, c2 - c1) == (2, 1), (shape, c1 - c0, c2 - c1)


def test_forward_and_backward_replay_from_a_graph():
    """No host readback, no upload: forward + backward captured with torch.cuda.graph replays to the bits of the eager run."""
    from gan_lab_amd import ops
    h, proxy, lab = make_inputs((130, 40, 4), None, 0)
    (z, zl), _, _ = _ce_case((64, 10), None)
    h, proxy, z = (t.cuda().requires_grad_(True) for t in (h, proxy, z))
    lab, zl = lab.cuda(), zl.cuda()

    def run():
        outs = []
        for mode in ('2c', 'd2d'):
            loss = ops.class_contrastive(h, proxy, lab, mode=mode, temperature=0.5)
            outs += [loss, *torch.autograd.grad(loss, (h, proxy))]
        ce = ops.class_cross_entropy(z, zl)
        return outs + [ce, *torch.autograd.grad(ce, z)]

    eager = [t.detach().clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.detach().zero_()              # a capture records, it does not run
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b.detach())


# ---- the learner --------------------------------------------------------------------------------------------------------------
N_B, N_K = 8, 3


def _learner(mode, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    kw.setdefault('random_seed', 7)
    kw.setdefault('lr_base', 0.)        # the step leaves the parameters where they are: the composition sees the same networks
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=N_B,
                      num_iters_save_model=10 ** 9, log_every=0, len_latent=32, num_classes=N_K, cgan=mode, cond_embed=24,
                      cond_temperature=0.5, **kw)
    cfg.fmap_g, cfg.fmap_d = 8, 8
    torch.manual_seed(7)
    return GANLearner(cfg)


def _step_data():
    g = torch.Generator().manual_seed(11)
    return dict(real=(torch.rand(N_B, 3, 32, 32, generator=g) * 2 - 1).cuda(), zd=torch.randn(N_B, 32, generator=g).cuda(),
                zg=torch.randn(N_B, 32, generator=g).cuda(), eps=torch.rand(N_B, 1, 1, 1, generator=g).cuda(),
                labels=torch.tensor([0, 2, 2, 0, 1, 2, 0, 1], dtype=torch.int32).cuda())


def _aten_term(L, f, labels):
    """The conditioning term composed from ATen ops on the device, on the critic's own heads."""
    from gan_lab_amd import conditional
    d, p = L.disc_model, L._cond
    if d.cond_mode == 'acgan':
        return F.cross_entropy(d.cls(f), labels.long())
    return ref.contrastive(d.embed(f), conditional.head_weight(d.proxy), labels, mode='2c' if d.cond_mode == 'contra' else 'd2d',
                           temperature=p['temperature'], margin_pos=p['margin_pos'], margin_neg=p['margin_neg'])


def _composed_d(L, dr):
    L.arena_d.zero_grad()
    if L.sn is not None:
        L.sn.refresh(iterate=False)
    with torch.no_grad():
        xgen = L.gen_model(dr['zd'], dr['labels'])
    d_gen = L.disc_model(xgen, dr['labels'])
    d_real, f = L.disc_model(dr['real'], dr['labels'], return_features=True)
    term = _aten_term(L, f, dr['labels'])
    loss = L.loss_func_disc(d_gen, d_real) + L._cond['weight'] * term
    if L.gradient_penalty is not None:
        loss = loss + L.calc_gp(xgen, dr['real'], eps_interp=dr['eps'], labels=dr['labels'])
    loss.backward()
    if L.sn is not None:
        L.sn.backward()
    return loss.detach(), term.detach(), {k: p.grad.detach().clone() for k, p in L.disc_model.named_parameters()}


def _composed_g(L, dr):
    L.arena_g.zero_grad()
    if L.sn is not None:
        L.sn.refresh(iterate=False)
    out, f = L.disc_model(L.gen_model(dr['zg'], dr['labels']), dr['labels'], return_features=True)
    term = _aten_term(L, f, dr['labels'])
    loss = L.loss_func_gen(out) + L._cond['weight'] * term
    loss.backward()
    return loss.detach(), term.detach(), {k: p.grad.detach().clone() for k, p in L.gen_model.named_parameters()}


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _cmp(what, got, want):
    gmax = max(float(v.abs().max()) for v in want.values())
    worst = 0.0
    for k, b in want.items():
        den = gmax if resnet_zero_grad_key(k) else max(float(b.abs().max()), 1e-4 * gmax)
        e = float((got[k].double() - b.double()).abs().max()) / den
        worst = max(worst, e)
        assert e <= TOL, f'{what} {k}: rel err {e:.3e} > {TOL:.1e}'
    print(f'{what}: worst gradient error {worst:.2e} over {len(want)} parameters')


HEADS = {'acgan': ('cls',), 'contra': ('embed', 'proxy'), 'reacgan': ('embed', 'proxy')}
RUNS = [('contra', {}), ('reacgan', {}),
        ('reacgan', dict(loss='hinge', gradient_penalty=None, spectral_norm=True))]


@pytest.mark.parametrize('mode,kw', RUNS, ids=['contra', 'reacgan', 'reacgan-hinge-sn'])
def test_learner_steps_equal_their_composition(mode, kw):
    L = _learner(mode, cond_lambda=0.8, **kw)
    dr = _step_data()
    assert L._pair_critic_batches(dr['real'], dr['real'])        # the new heads leave the paired pass on
    L.set_requires_grad_disc(True)
    loss_d = L.d_step(dr['real'], zb=dr['zd'], eps_interp=dr['eps'], labels=dr['labels'])
    got_d, cond_d = _grads(L.disc_model), L.last_losses['cond_d'].clone()
    want_loss, want_term, want_d = _composed_d(L, dr)
    print(f'{mode} d_step: loss {float(loss_d):.6f} composed {float(want_loss):.6f}  term {float(cond_d):.6f} composed '
          f'{float(want_term):.6f}')
    assert rel_err(loss_d, want_loss) <= TOL and rel_err(cond_d, want_term) <= TOL
    _cmp(f'{mode} critic', got_d, want_d)
    for head in HEADS[mode]:
        assert any(k.startswith(head + '.') and float(v.abs().max()) > 0 for k, v in got_d.items()), head
    L.set_requires_grad_disc(False)
    loss_g = L.g_step(zb=dr['zg'], labels=dr['labels'])
    got_g, cond_g = _grads(L.gen_model), L.last_losses['cond_g'].clone()
    want_loss, want_term, want_g = _composed_g(L, dr)
    print(f'{mode} g_step: loss {float(loss_g):.6f} composed {float(want_loss):.6f}  term {float(cond_g):.6f} composed '
          f'{float(want_term):.6f}')
    assert rel_err(loss_g, want_loss) <= TOL and rel_err(cond_g, want_term) <= TOL
    _cmp(f'{mode} generator', got_g, want_g)
    L.set_requires_grad_disc(True)


@pytest.mark.parametrize('mode', ['contra', 'reacgan'])
def test_zero_weight_launches_nothing_and_checkpoints_carry_the_heads(mode, tmp_path):
    L = _learner(mode, cond_lambda=0., lr_base=1e-3)
    dr = _step_data()
    L.set_requires_grad_disc(True)
    L.d_step(dr['real'], zb=dr['zd'], eps_interp=dr['eps'], labels=dr['labels'])
    assert 'cond_d' not in L.last_losses
    for k, g in _grads(L.disc_model).items():
        if k.split('.')[0] in HEADS[mode]:
            assert bool((g == 0).all()), k
    # with the weight on the heads train; the checkpoint restores them bit for bit
    L = _learner(mode, cond_lambda=1., lr_base=1e-3)
    before = {k: v.clone() for k, v in L.disc_model.state_dict().items() if k.split('.')[0] in HEADS[mode]}
    L.d_step(dr['real'], zb=dr['zd'], eps_interp=dr['eps'], labels=dr['labels'])
    L.set_requires_grad_disc(False)
    L.g_step(zb=dr['zg'], labels=dr['labels'])
    L.set_requires_grad_disc(True)
    sd = L.disc_model.state_dict()
    assert before and all(not torch.equal(sd[k], v) for k, v in before.items() if k.endswith('weight'))
    L.not_trained_yet = False
    path = tmp_path / 'resnetgan_model.tar'
    L.save_model(path)
    with pytest.raises(ValueError, match='reference_format'):
        L.save_model(path, reference_format=True)
    from gan_lab_amd import checkpoint
    saved = checkpoint.load_checkpoint(path, 'cpu')['config']
    assert saved['cgan'] == mode and saved['cond_lambda'] == 1.0
    L2 = _learner(mode, cond_lambda=1., lr_base=1e-3, random_seed=8)
    L2.load_model(path)
    sd2 = L2.disc_model.state_dict()
    assert list(sd.keys()) == list(sd2.keys())
    for k in sd:
        assert torch.equal(sd[k].cpu(), sd2[k].cpu()), k


def test_acgan_head_equals_its_composition():
    """A critic built with ``cgan='acgan'``: the score is unconditional, and ``cond_term`` on the feature of the same pass gives
    the loss and the parameter gradients of ``F.cross_entropy`` on ``cls(f)`` within TOL."""
    from gan_lab_amd import conditional
    from gan_lab_amd.resnetgan import architectures as A
    torch.manual_seed(7)
    d = A.Discriminator32PixResnet(fmap=8, cgan='acgan', num_classes=N_K).cuda().train()
    dr = _step_data()
    out, f = d(dr['real'], dr['labels'], return_features=True)
    assert torch.equal(out, d.linear1(f).view(-1)) and tuple(d.cls.linear.weight.shape) == (N_K, 8)
    term = conditional.cond_term(d, f, dr['labels'], None)
    (out.mean() + 0.8 * term).backward()
    got = _grads(d)
    d.zero_grad()
    out, f = d(dr['real'], dr['labels'], return_features=True)
    want_term = F.cross_entropy(d.cls(f), dr['labels'].long())
    (out.mean() + 0.8 * want_term).backward()
    term, want_term = term.detach(), want_term.detach()
    print(f'acgan head: term {float(term):.6f} composed {float(want_term):.6f}')
    assert rel_err(term, want_term) <= TOL
    _cmp('acgan critic', got, _grads(d))
    assert float(got['cls.linear.weight'].abs().max()) > 0
