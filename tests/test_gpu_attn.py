"""GPU tests of the self-attention kernels (csrc/attention.hip), the block (attention.py), the ResNet networks and the
learner with ``config.self_attention``.

Core bound, per tensor: ``rel_err <= max(1e-5, 16 * e_cpu)`` where ``e_cpu`` is the error of the reference (attn_reference.py)
run in fp32 on the CPU against its own float64 run on the same inputs; the factor 16 is the headroom tests/test_gpu_sn.py
allows for another summation order and a hardware ``exp``.  A wrong mask, tail or rescale is O(1).

Measured errors: not recorded yet; every test prints its figures before it asserts.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_reference as ref
from util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the block / network rule of tests/test_gpu_resnet.py
SHAPES = [(1, 4, 16, 1, 1), (2, 4, 16, 37, 5), (2, 8, 32, 130, 67), (1, 64, 256, 96, 300), (3, 16, 64, 256, 64),
          (1, 16, 64, 1024, 256)]
CASES = [(s, 'std3') for s in SHAPES] + [((2, 8, 32, 130, 67), 'pm80')]
NAMES = ('o', 'lse', 'dq', 'dk', 'dv')


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Inputs (CPU fp32), the float64 reference and e_cpu of every tensor; computed once, never modified."""
    n, dk, dv, l, s = shape
    g = torch.Generator().manual_seed(1000 * l + s)
    a = (3.0 / dk ** 0.5) ** 0.5                       # logits = sum of dk products of N(0, a^2) pairs: std 3
    q, k = torch.randn(n, dk, l, generator=g) * a, torch.randn(n, dk, s, generator=g) * a
    v, d_o = torch.randn(n, dv, s, generator=g), torch.randn(n, dv, l, generator=g)
    if kind == 'pm80':                                 # logits reach about +-80: exp overflows without the max subtraction
        q = q * (80.0 / torch.einsum('ndl,nds->nls', q.double(), k.double()).abs().max().item())
    want = ref.attention_with_grads(q, k, v, d_o, torch.float64)
    cpu = ref.attention_with_grads(q, k, v, d_o, torch.float32)
    e_cpu = [rel_err(c, w) for c, w in zip(cpu, want)]
    return (q, k, v, d_o), want, e_cpu


def _gpu(q, k, v, d_o):
    from gan_lab_amd import ops
    q, k, v = (t.cuda().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(q, k, v)
    lse = o.grad_fn.saved_tensors[4] if hasattr(o.grad_fn, 'saved_tensors') else None
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o.cuda())
    return o.detach(), lse, dq, dk, dv


@pytest.mark.parametrize('shape,kind', CASES, ids=[f'{"x".join(map(str, s))}-{k}' for s, k in CASES])
def test_core_against_float64(shape, kind):
    from gan_lab_amd import ops
    inputs, want, e_cpu = _case(shape, kind)
    got = list(_gpu(*inputs))
    got[1] = ops.k_attn_fwd(*(t.cuda() for t in inputs[:3]))[1]
    errs = [rel_err(g_, w) for g_, w in zip(got, want)]
    print(f'attn {shape} {kind}: ' + ' '.join(f'{nm} gpu {e:.2e} cpu {c:.2e}' for nm, e, c in zip(NAMES, errs, e_cpu)))
    for nm, e, c in zip(NAMES, errs, e_cpu):
        assert e <= max(1e-5, 16 * c), f'{nm}: {e:.3e} > max(1e-5, 16 * {c:.3e})'


def test_tails_stay_inside_their_buffers():
    """Outputs live inside NaN-poisoned buffers with gaps: the kernels write their tensors and nothing else."""
    from gan_lab_amd import _lib, ops
    shape = (2, 8, 32, 130, 67)
    n, dk, dv, l, s = shape
    (q, k, v, d_o), _, _ = _case(shape, 'std3')
    q, k, v, d_o = (t.cuda() for t in (q, k, v, d_o))
    sizes = dict(o=n * dv * l, lse=n * l, dq=n * dk * l, dk=n * dk * s, dv=n * dv * s, ws=n * l)
    gap = 61
    buf = torch.full((sum(sizes.values()) + gap * (len(sizes) + 1),), float('nan'), device='cuda')
    views, off = {}, gap
    for name, size in sizes.items():
        views[name] = buf[off:off + size]
        off += size + gap
    L, p, st = _lib.lib(), ops._p, ops._st()
    _lib.check(L.ganlab_attn_fwd_f32(p(q), p(k), p(v), p(views['o']), p(views['lse']), n, dk, dv, l, s, st), 'fwd')
    _lib.check(L.ganlab_attn_bwd_f32(p(q), p(k), p(v), p(views['o']), p(views['lse']), p(d_o), p(views['dq']), p(views['dk']),
                                     p(views['dv']), n, dk, dv, l, s, p(views['ws']), sizes['ws'] * 4, st), 'bwd')
    torch.cuda.synchronize()
    o, lse, dq, dk_, dv_ = _gpu(q.cpu(), k.cpu(), v.cpu(), d_o.cpu())
    for name, t in (('o', o), ('dq', dq), ('dk', dk_), ('dv', dv_)):
        assert torch.equal(views[name], t.reshape(-1)), name
    inside = torch.zeros_like(buf, dtype=torch.bool)
    off = gap
    for size in sizes.values():
        inside[off:off + size] = True
        off += size + gap
    assert bool(torch.isnan(buf[~inside]).all())
    assert not bool(torch.isnan(buf[inside]).any())


def test_two_runs_are_bit_equal():
    inputs, _, _ = _case((2, 8, 32, 130, 67), 'std3')
    a, b = _gpu(*inputs), _gpu(*inputs)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    inputs, _, _ = _case((1, 16, 64, 1024, 256), 'std3')
    a, b = _gpu(*inputs), _gpu(*inputs)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_forward_and_backward_replay_from_a_graph():
    """No host readback, no upload: forward + backward captured with torch.cuda.graph replays to the bits of the eager run."""
    from gan_lab_amd import ops
    (q, k, v, d_o), _, _ = _case((2, 8, 32, 130, 67), 'std3')
    q, k, v = (t.cuda().requires_grad_(True) for t in (q, k, v))
    d_o = d_o.cuda()

    def run():
        o = ops.attention(q, k, v)
        return (o,) + torch.autograd.grad(o, (q, k, v), d_o)

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


def test_no_attention_map_is_materialised():
    from gan_lab_amd import ops
    n, dk, dv, l, s = 8, 16, 64, 1024, 256
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(*sh, generator=g).cuda().requires_grad_(True) for sh in ((n, dk, l), (n, dk, s), (n, dv, s)))
    d_o = torch.randn(n, dv, l, generator=g).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    o = ops.attention(q, k, v)
    grads = torch.autograd.grad(o, (q, k, v), d_o)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f'attention fwd+bwd at {(n, dk, dv, l, s)}: peak grows by {grown} bytes, the map would be {n * l * s * 4}')
    assert grown < n * l * s * 4
    assert all(bool(torch.isfinite(t).all()) for t in grads)


def test_unsupported_geometry_raises():
    from gan_lab_amd import ops
    from gan_lab_amd._lib import GanlabLibraryError
    q, k, v = torch.randn(1, 6, 8).cuda(), torch.randn(1, 6, 4).cuda(), torch.randn(1, 16, 4).cuda()
    assert not ops.attention_ok(1, 6, 16, 8, 4)
    with pytest.raises(GanlabLibraryError, match='EUNSUPPORTED'):
        ops.attention(q, k, v)
    with pytest.raises(TypeError):
        ops.attention(q.cpu(), k.cpu(), v.cpu())


def test_double_backward_raises():
    from gan_lab_amd import ops
    q, k, v = (torch.randn(*sh).cuda().requires_grad_(True) for sh in ((1, 4, 9), (1, 4, 4), (1, 16, 4)))
    gq, = torch.autograd.grad(ops.attention(q, k, v).square().sum(), q, create_graph=True)
    with pytest.raises(NotImplementedError, match='self_attention'):
        torch.autograd.grad(gq.sum(), q)
    x = torch.randn(1, 2, 4, 4).cuda().requires_grad_(True)
    gx, = torch.autograd.grad(ops.max_pool2x2(x).square().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match='self_attention'):
        torch.autograd.grad(gx.sum(), x)


# ---- max_pool2x2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 3, 6, 10), (1, 16, 32, 32)])
def test_max_pool_against_aten(shape):
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(shape[-1])
    x, gy = torch.randn(*shape, generator=g), torch.randn(shape[0], shape[1], shape[2] // 2, shape[3] // 2, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = torch.nn.functional.max_pool2d(xr, 2)
    gr, = torch.autograd.grad(yr, xr, gy)
    xg = x.cuda().requires_grad_(True)
    yg = ops.max_pool2x2(xg)
    gg, = torch.autograd.grad(yg, xg, gy.cuda())
    assert torch.equal(yg.detach().cpu(), yr.detach()) and torch.equal(gg.cpu(), gr)
    with pytest.raises(ValueError, match='even'):
        ops.max_pool2x2(torch.zeros(1, 1, 3, 4).cuda())


def test_max_pool_ties_go_to_the_first():
    from gan_lab_amd import ops
    x = torch.tensor([[1., 1., 0., 2., 5., 5.],
                      [1., 1., 2., 2., 5., 4.],
                      [3., 0., 0., 0., -1., -2.],
                      [0., 3., 0., 0., -1., -1.]]).reshape(1, 1, 4, 6)
    gy = torch.arange(1., 7.).reshape(1, 1, 2, 3)
    xr = x.clone().requires_grad_(True)
    gr, = torch.autograd.grad(torch.nn.functional.max_pool2d(xr, 2), xr, gy)
    xg = x.cuda().requires_grad_(True)
    y = ops.max_pool2x2(xg)
    gg, = torch.autograd.grad(y, xg, gy.cuda())
    want = torch.tensor([[1., 0., 0., 2., 3., 0.],
                         [0., 0., 0., 0., 0., 0.],
                         [4., 0., 5., 0., 6., 0.],
                         [0., 0., 0., 0., 0., 0.]]).reshape(1, 1, 4, 6)
    assert torch.equal(gg.cpu(), want) and torch.equal(gr, want)
    assert torch.equal(y.detach().cpu(), torch.tensor([[1., 2., 5.], [3., 0., -1.]]).reshape(1, 1, 2, 3))


# ---- the block ----------------------------------------------------------------------------------------------------------------
def _block(ni, seed):
    from gan_lab_amd.attention import SelfAttention2d
    torch.manual_seed(seed)
    blk = SelfAttention2d(ni)
    with torch.no_grad():
        for c in (blk.theta, blk.phi, blk.g, blk.o):
            c.conv2d.weight.mul_(3.0)                # logits of order 1 rather than the initialisation's ~0.1
    return blk


@pytest.mark.parametrize('ni,shape', [(32, (2, 32, 8, 8)), (128, (2, 128, 16, 16))])
def test_block_against_float64(ni, shape):
    blk = _block(ni, ni)
    with torch.no_grad():
        blk.gamma.fill_(0.7)
    g = torch.Generator().manual_seed(ni + 1)
    x, cot = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    leaves = [t.detach().double().clone().requires_grad_(True) for t in
              (x, blk.theta.conv2d.weight, blk.phi.conv2d.weight, blk.g.conv2d.weight, blk.o.conv2d.weight, blk.gamma)]
    want = ref.block(*leaves)
    want_g = torch.autograd.grad(want, leaves, cot.double())
    blk.cuda()
    xg = x.cuda().requires_grad_(True)
    out = blk(xg)
    out.backward(cot.cuda())
    got_g = [xg.grad, blk.theta.conv2d.weight.grad, blk.phi.conv2d.weight.grad, blk.g.conv2d.weight.grad,
             blk.o.conv2d.weight.grad, blk.gamma.grad]
    errs = [rel_err(out.detach(), want.detach())] + [rel_err(a, b) for a, b in zip(got_g, want_g)]
    print(f'block ni={ni}: ' + ' '.join(f'{nm} {e:.2e}' for nm, e in
                                        zip(('out', 'dx', 'dtheta', 'dphi', 'dg', 'do', 'dgamma'), errs)))
    assert max(errs) <= TOL, errs


def test_block_with_gamma_zero_is_the_identity():
    blk = _block(32, 3).cuda()
    x = torch.randn(2, 32, 8, 8).cuda()
    assert float(blk.gamma.detach()) == 0.0
    assert torch.equal(blk(x).detach(), x)


# ---- the networks ---------------------------------------------------------------------------------------------------------------
def _net_pair(name, kw, seed):
    from gan_lab_amd.resnetgan import architectures as A
    torch.manual_seed(seed)
    off = getattr(A, name)(**kw)
    on = getattr(A, name)(self_attention=True, **kw)
    missing, unexpected = on.load_state_dict(off.state_dict(), strict=False)
    assert not unexpected and all(k.startswith('self_attn.') for k in missing)
    return off.cuda().train(), on.cuda().train()


@pytest.mark.parametrize('name,kw,in_shape', [('Generator64PixResnet', dict(fmap=16, len_latent=32), (2, 32)),
                                              ('Discriminator64PixResnet', dict(fmap=16), (2, 3, 64, 64))])
def test_networks_with_a_closed_and_an_open_gate(name, kw, in_shape):
    off, on = _net_pair(name, kw, 11)
    assert on.self_attn.ni == 32
    g = torch.Generator().manual_seed(12)
    x = torch.randn(*in_shape, generator=g).cuda()
    y_off = off(x)
    cot = torch.randn(*y_off.shape, generator=g).cuda()
    y_off.backward(cot)
    y_on = on(x)
    y_on.backward(cot)
    assert torch.equal(y_on.detach(), y_off.detach())                   # gamma = 0: the block is the identity
    shared = dict(off.named_parameters())
    for k, p in on.named_parameters():
        if k in shared and shared[k].grad is not None:
            assert torch.equal(p.grad, shared[k].grad), k
    on.zero_grad()
    with torch.no_grad():
        on.self_attn.gamma.fill_(0.5)
    y_open = on(x)
    y_open.backward(cot)
    assert not torch.equal(y_open.detach(), y_off.detach())
    for k, p in on.self_attn.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


# ---- the learner ------------------------------------------------------------------------------------------------------------------
def _learner(**kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, num_disc_iters=2, random_seed=7, len_latent=32, **kw)
    cfg.fmap_g, cfg.fmap_d = 32, 32
    torch.manual_seed(7)
    return GANLearner(cfg)


def _batches(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).cuda() for _ in range(n)], \
        [torch.randn(4, 32, generator=g).cuda() for _ in range(n)]


def _iteration(L, reals, zs):
    """One main iteration: generator step, then two critic steps."""
    L.set_requires_grad_disc(False)
    losses = [L.g_step(zb=zs[0])]
    L.set_requires_grad_disc(True)
    for i in range(2):
        losses.append(L.d_step(reals[i], zb=zs[1 + i]))
    return [float(v) for v in losses]


SAGAN = dict(self_attention='gd', spectral_norm=True, loss='hinge', gradient_penalty=None)


def test_learner_sagan_recipe(tmp_path):
    """ResNet GAN 32^2 with attention in both networks, spectral norm, hinge loss, no penalty: finite losses, both gates leave
    0, the block's convolutions are spectrally normalised; a checkpoint restores every tensor to the bit and the run continues
    as if it had never been saved."""
    L = _learner(**SAGAN)
    assert L.gen_model.self_attn.ni == 32 and L.disc_model.self_attn.ni == 32
    assert 'self_attn.theta.conv2d.weight' in L.sn.names and 'self_attn.gamma' not in L.sn.names
    reals, zs = _batches(12)
    for it in range(3):
        losses = _iteration(L, reals[2 * it:2 * it + 2], zs[3 * it:3 * it + 3])
        assert all(np.isfinite(losses)), losses
    gates = float(L.gen_model.self_attn.gamma.detach()), float(L.disc_model.self_attn.gamma.detach())
    print('gates after three iterations:', gates)
    assert gates[0] != 0.0 and gates[1] != 0.0
    assert 'self_attn.theta.conv2d.weight_u' in L.disc_model.state_dict()
    L.not_trained_yet = False
    path = tmp_path / 'resnetgan_model.tar'
    L.save_model(path)
    with pytest.raises(ValueError, match='reference_format'):
        L.save_model(path, reference_format=True)
    L2 = _learner(**SAGAN)
    L2.load_model(path)
    L2.gen_model.train()
    L2.disc_model.train()
    for m, m2 in ((L.gen_model, L2.gen_model), (L.disc_model, L2.disc_model)):
        sd, sd2 = m.state_dict(), m2.state_dict()
        assert list(sd.keys()) == list(sd2.keys())
        for k in sd:
            assert torch.equal(sd[k].cpu(), sd2[k].cpu()), k
    a = _iteration(L, reals[6:8], zs[9:12])
    b = _iteration(L2, reals[6:8], zs[9:12])
    assert a == b, (a, b)


def test_learner_refuses_a_penalty_behind_critic_attention():
    with pytest.raises(ValueError, match='hinge'):
        _learner(self_attention='d', loss='hinge')                 # gradient_penalty keeps its default, wgan-gp
    L = _learner(self_attention='g')                               # the generator's block works with every penalty
    reals, zs = _batches(3)
    assert all(np.isfinite(_iteration(L, reals[:2], zs[:3])))
    assert L.disc_model.self_attn is None and float(L.gen_model.self_attn.gamma.detach()) != 0.0


def test_default_learner_is_untouched():
    L = _learner()
    assert L.gen_model.self_attn is None and L.disc_model.self_attn is None
    for m in (L.gen_model, L.disc_model):
        assert not any('self_attn' in k for k in m.state_dict().keys())
    assert not any('self_attn' in k for k, _ in list(L.gen_model.named_parameters()) + list(L.disc_model.named_parameters()))
