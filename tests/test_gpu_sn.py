"""GPU tests of spectral normalisation (csrc/spectral.hip, gan_lab_amd/spectral_norm.py) and the hinge loss: the batched
refresh / backward kernels against the float64 reference (tests/sn_reference.py) on a job table with awkward shapes, their
convergence, bitwise reproducibility and graph capture, ``ops.hinge_mean``, the normalised critics against the oracle,
and the learner's schedule, checkpoints and key layout.

Bounds.  Kernel results: rel_err (max-abs over max-abs) <= 1e-5 against float64; a CPU fp32 restatement of the formulas
stays below 5.9e-7 on these shapes (worst: v of 512 x 4608), so 1e-5 leaves ~17x for another reduction order while a wrong
tail, stride or layer offset is O(1).  Networks: the 1e-3 rule of tests/test_gpu_resnet.py."""
import numpy as np
import pytest
import torch

import sn_reference as ref
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3
BOUND = 1e-5
SHAPES = [(1, 64), (5, 7), (64, 27), (128, 64), (128, 576), (512, 4608)]     # (R, K): R = 1, K < 64, K % 4 != 0, many blocks
GAP = 8       # floats between two slots (keeps them 16-byte aligned), poisoned with NaN


class _Table(object):
    """A job table over hand-made arenas: every buffer starts as NaN, the slots are filled, the gaps must stay NaN."""

    def __init__(self, shapes, seed=0, weights=None):
        from gan_lab_amd import ops
        g = torch.Generator().manual_seed(seed)
        self.shapes = shapes
        sizes = [r * k for r, k in shapes]
        self.off, self.uoff = [], []
        o = uo = GAP
        for (r, k), n in zip(shapes, sizes):
            self.off.append(o)
            o += (n + 3) // 4 * 4 + GAP
            ru, rv = (r + 3) // 4 * 4, (k + 3) // 4 * 4
            self.uoff.append((uo, uo + ru + GAP, uo + ru + rv + 2 * GAP))
            uo += ru + rv + 4 + 3 * GAP
        nan = lambda n: torch.full((n,), float('nan'), device='cuda')      # noqa: E731
        self.W, self.Wsn, self.G, self.gW, self.uv = nan(o), nan(o), nan(o), nan(o), nan(uo)
        self.mask, self.uvmask = torch.ones(o, dtype=torch.bool), torch.ones(uo, dtype=torch.bool)     # True = gap
        self.W0, self.u0, self.v0, self.G0 = [], [], [], []
        jobs = []
        for i, ((r, k), n, of, (ou, ov, os_)) in enumerate(zip(shapes, sizes, self.off, self.uoff)):
            w = weights[i].float().reshape(-1) if weights is not None else 0.05 * torch.randn(n, generator=g)
            u = torch.nn.functional.normalize(torch.randn(r, generator=g), dim=0)
            v = torch.nn.functional.normalize(torch.randn(k, generator=g), dim=0)
            gs = torch.randn(n, generator=g)
            self.W0.append(w.reshape(r, k)), self.u0.append(u), self.v0.append(v), self.G0.append(gs.reshape(r, k))
            self.mask[of:of + n] = False
            self.uvmask[ou:ou + r] = False
            self.uvmask[ov:ov + k] = False
            self.uvmask[os_] = False
            jobs.append(dict(w=self.W[of:of + n].view(r, k), w_sn=self.Wsn[of:of + n], g_sn=self.G[of:of + n],
                             gw=self.gW[of:of + n], u=self.uv[ou:ou + r], v=self.uv[ov:ov + k], sigma=self.uv[os_:os_ + 1]))
        self.jobs = jobs
        self.reset()
        self.table = ops.SnTable(jobs)

    def reset(self, gw=None):
        for i, j in enumerate(self.jobs):
            j['w'].copy_(self.W0[i])
            j['u'].copy_(self.u0[i])
            j['v'].copy_(self.v0[i])
            j['g_sn'].copy_(self.G0[i].reshape(-1))
            j['w_sn'].fill_(float('nan'))
            j['sigma'].fill_(float('nan'))
            j['gw'].copy_(gw[i].reshape(-1)) if gw is not None else j['gw'].zero_()

    def gaps_untouched(self):
        for buf, m in ((self.W, self.mask), (self.Wsn, self.mask), (self.G, self.mask), (self.gW, self.mask),
                       (self.uv, self.uvmask)):
            assert bool(torch.isnan(buf.cpu()[m]).all()), 'a kernel wrote between two layers\' slots'

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone().view(torch.int32) for b in (self.Wsn, self.gW, self.uv)]


@pytest.fixture(scope='module')
def table():
    return _Table(SHAPES)


def _cmp(what, a, b):
    e = rel_err(a, b)
    print(f'{what}: rel err {e:.3e}')
    assert e <= BOUND, f'{what}: rel err {e:.3e} > {BOUND:.0e}'


def test_batched_refresh(table):
    from gan_lab_amd import _lib, ops
    T = table
    T.reset()
    n0 = _lib.launch_count()
    ops.sn_refresh(T.table, True)
    assert _lib.launch_count() - n0 == 4          # whatever the number of layers
    state = []
    for i, (j, (r, k)) in enumerate(zip(T.jobs, SHAPES)):
        u, v, sigma, wsn = ref.refresh(T.W0[i], T.u0[i])
        _cmp(f'u {r}x{k}', j['u'], u)
        _cmp(f'v {r}x{k}', j['v'], v)
        _cmp(f'sigma {r}x{k}', j['sigma'], sigma.reshape(1))
        _cmp(f'W_sn {r}x{k}', j['w_sn'].view(r, k), wsn)
        state.append((u, v, j['u'].clone(), j['v'].clone()))
    T.gaps_untouched()
    # the weights moved (an optimiser step): sigma and W_sn follow with the stored u, v
    g = torch.Generator().manual_seed(9)
    moved = [w + 0.01 * torch.randn(w.shape, generator=g) for w in T.W0]
    for j, w in zip(T.jobs, moved):
        j['w'].copy_(w)
    n0 = _lib.launch_count()
    ops.sn_refresh(T.table, False)
    assert _lib.launch_count() - n0 == 2
    for i, (j, (r, k)) in enumerate(zip(T.jobs, SHAPES)):
        u, v, u_gpu, v_gpu = state[i]
        _, _, sigma, wsn = ref.refresh(moved[i], u, v, iterate=False)
        assert torch.equal(j['u'], u_gpu) and torch.equal(j['v'], v_gpu)
        _cmp(f'sigma (no iteration) {r}x{k}', j['sigma'], sigma.reshape(1))
        _cmp(f'W_sn (no iteration) {r}x{k}', j['w_sn'].view(r, k), wsn)
    T.gaps_untouched()


def test_batched_backward(table):
    from gan_lab_amd import _lib, ops
    T = table
    T.reset()
    ops.sn_refresh(T.table, True)
    n0 = _lib.launch_count()
    ops.sn_backward(T.table)
    assert _lib.launch_count() - n0 == 2
    want = []
    for i, (j, (r, k)) in enumerate(zip(T.jobs, SHAPES)):
        u, v, sigma, _ = ref.refresh(T.W0[i], T.u0[i])
        gw = ref.backward(T.G0[i], T.W0[i], u, v, sigma)
        want.append(gw)
        got = j['gw'].view(r, k).cpu().double()
        _cmp(f'gW {r}x{k}', got, gw)
        # W_sn does not change when W is rescaled: the gradient is orthogonal to W
        w = T.W0[i].double()
        inner = abs((got * w).sum().item()) / (got.norm().item() * w.norm().item())
        print(f'<gW, W> / |gW||W| {r}x{k}: {inner:.3e}')
        assert inner <= BOUND
    T.gaps_untouched()
    # accumulation: the kernels add to what the gradient arena holds
    g = torch.Generator().manual_seed(4)
    pre = [torch.randn(r, k, generator=g) for r, k in SHAPES]
    T.reset(gw=pre)
    ops.sn_refresh(T.table, True)
    ops.sn_backward(T.table)
    for i, (j, (r, k)) in enumerate(zip(T.jobs, SHAPES)):
        _cmp(f'gW += {r}x{k}', j['gw'].view(r, k), pre[i].double() + want[i])
    T.gaps_untouched()


def test_power_iteration_converges():
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(11)
    U, _ = torch.linalg.qr(torch.randn(48, 48, generator=g, dtype=torch.float64))
    V, _ = torch.linalg.qr(torch.randn(80, 48, generator=g, dtype=torch.float64))
    s = torch.zeros(48, dtype=torch.float64)
    s[:11] = torch.tensor([2.0, 1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1], dtype=torch.float64)
    W = (U * s) @ V.t()
    T = _Table([(48, 80)], seed=2, weights=[W])
    for _ in range(30):
        ops.sn_refresh(T.table, True)
    sigma = T.jobs[0]['sigma'].item()
    print(f'sigma after 30 iterations: {sigma!r}')
    assert abs(sigma - 2.0) / 2.0 <= BOUND
    top = np.linalg.svd(T.jobs[0]['w_sn'].view(48, 80).cpu().double().numpy(), compute_uv=False)[0]
    print(f'top singular value of W_sn: {top!r}')
    assert abs(top - 1.0) <= BOUND
    T.gaps_untouched()


def test_bitwise_reproducible(table):
    from gan_lab_amd import ops
    T = table
    runs = []
    for _ in range(2):
        T.reset()
        ops.sn_refresh(T.table, True)
        ops.sn_backward(T.table)
        ops.sn_refresh(T.table, False)
        runs.append(T.snapshot())
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_refresh_and_backward_replay_from_a_graph(table):
    """Everything is device-resident (no host read of sigma, no allocation, no upload): a captured refresh + backward
    replays to the bits of the eager calls."""
    from gan_lab_amd import ops
    T = table
    T.reset()
    ops.sn_refresh(T.table, True)
    ops.sn_backward(T.table)
    eager = T.snapshot()
    T.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sn_refresh(T.table, True)
        ops.sn_backward(T.table)
    T.reset()               # a capture records, it does not run
    graph.replay()
    for a, b in zip(eager, T.snapshot()):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n', [1, 7, 64])
@pytest.mark.parametrize('a,b', [(1.0, -1.0), (1.0, 1.0)])
def test_hinge_mean(n, a, b):
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(n)
    cases = [torch.randn(n, generator=g) * 2]
    if n == 1:
        cases = [torch.tensor([0.3]), torch.tensor([1.7]), torch.tensor([-1.7])]      # both sides of either kink
    for x in cases:
        x = torch.where((a + b * x).abs() < 1e-2, x + 0.1, x)      # nothing on the kink
        if n > 1:
            assert ((a + b * x) > 0).any() and ((a + b * x) < 0).any()
        xr = x.clone().double().requires_grad_(True)
        lr = torch.relu(a + b * xr).mean()
        lr.backward()
        xg = x.clone().cuda().requires_grad_(True)
        lg = ops.hinge_mean(xg, a, b)
        assert abs(lg.item() - lr.item()) <= 1e-6 * max(abs(lr.item()), 1.0)
        gx, = torch.autograd.grad(lg, xg, create_graph=True)
        assert (gx.detach().cpu().double() - xr.grad).abs().max().item() <= 1e-6
        ggx, = torch.autograd.grad(gx.sum(), xg)
        assert ggx.shape == xg.shape and bool((ggx == 0).all())
    # the loss functions built on it
    from gan_lab_amd.utils import backprop_utils as bp
    df, dr = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g) * 2
    assert_close(bp.loss_disc('hinge', df.cuda(), dr.cuda()).cpu().double(), ref.hinge_disc(df.double(), dr.double()), 1e-6)
    assert_close(bp.loss_gen('hinge', df.cuda()).cpu().double(), ref.hinge_gen(df.double()), 1e-6)


# ---------------------------------------------------------------------------------------------------------------------- #
def _cmp_grads(named, ref_by_key, tol, what):
    """The per-key rule of tests/test_gpu_resnet.py."""
    gmax = max(float(v.abs().max()) for v in ref_by_key.values())
    for k, b in ref_by_key.items():
        a = named[k].grad.detach().double().cpu()
        den = max(b.abs().max().item(), 1e-4 * gmax)
        e = (a - b).abs().max().item() / den
        assert e <= tol, f'{what} {k}: rel err {e:.3e} > {tol:.1e}'


@pytest.mark.parametrize('res,batch,fmap,gp', [(32, 4, 32, False), (64, 2, 16, False), (32, 4, 32, True)],
                         ids=['32', '64', '32-wgan-gp'])
def test_normalised_critic_matches_oracle(res, batch, fmap, gp):
    """The critic with spectral_norm=True = the unchanged oracle critic run on W_sn (float64, from the pre-refresh u);
    parameter gradients = the oracle's gradients towards W_sn pushed through the reference backward.  ``gp``: the WGAN-GP
    term is part of the loss, so the double backward reaches W_sn.grad too."""
    from oracle import resnet, step as ostep
    from gan_lab_amd import ops
    from gan_lab_amd.optim import ParamArena
    from gan_lab_amd.resnetgan import architectures as A
    from gan_lab_amd.spectral_norm import SpectralNorm
    from gan_lab_amd.utils import backprop_utils as bp
    torch.manual_seed(res + gp)
    cls = A.Discriminator32PixResnet if res == 32 else A.Discriminator64PixResnet
    d = cls(fmap=fmap, spectral_norm=True).cuda().train()
    with torch.no_grad():      # every parameter away from its initial 0 / 1
        for k, p in d.named_parameters():
            if k.endswith('bias'):
                p.normal_(0, 0.1)
            elif '.norm.' in k:
                p.add_(0.2 * torch.randn_like(p))
    arena = ParamArena(d.named_parameters(), 'cuda')
    sn = SpectralNorm(d, arena)
    before = {k: v.detach().cpu().double() for k, v in d.state_dict().items()}
    sn.refresh(iterate=True)
    sd = {k: v.detach().cpu().double() for k, v in d.state_dict().items()}
    weights = [k for k in sd if k.endswith(('conv2d.weight', 'linear.weight'))]
    assert len(weights) == len(sn.names) and set(weights) == set(sn.names)
    sd_o, norm = {}, {}
    for k, v in sd.items():
        if k.endswith(('weight_u', 'weight_v')):
            continue
        if k in weights:
            u, vv, sigma, wsn = ref.refresh(before[k], before[k + '_u'])
            assert rel_err(sd[k + '_u'], u) <= BOUND and rel_err(sd[k + '_v'], vv) <= BOUND
            assert rel_err(sn.sigma()[k], sigma.reshape(1)) <= BOUND
            norm[k] = (before[k], u, vv, sigma)
            v = wsn
        sd_o[k] = v.clone().requires_grad_(True)
    x = torch.randn(batch, 3, res, res)
    cot = torch.randn(batch)
    fake, real, eps = torch.randn(batch, 3, res, res), torch.randn(batch, 3, res, res), torch.rand(batch)
    # oracle
    xr = x.double().requires_grad_(True)
    out_r = resnet.disc_forward(sd_o, xr, res)
    loss_r = (out_r * cot.double()).sum()
    if gp:
        loss_r = loss_r + ostep.calc_gp(lambda t: resnet.disc_forward(sd_o, t, res), 'wgan-gp', fake.double(), real.double(),
                                        10.0, 1.0, eps.double().view(-1, 1, 1, 1))
    loss_r.backward()
    # HIP path, the learner's order of calls
    arena.zero_grad()
    xg = x.cuda().requires_grad_(True)
    out = d(xg)
    loss = ops.sum_all(ops.mul(out, cot.cuda()))
    if gp:
        loss = loss + bp.calc_gp(d, 'wgan-gp', fake.cuda(), real.cuda(), lda=10., gamma=1., eps_interp=eps.cuda())
    with ops.direct_param_grads(True):
        loss.backward()
    assert float(sn.gflat.abs().max()) > 0
    sn.backward()
    assert float(sn.gflat.abs().max()) == 0          # zeroed for the next step
    assert_close(out.detach().cpu(), out_r.detach(), TOL, 'D(x)')
    assert_close(loss.detach().cpu(), loss_r.detach(), TOL, 'loss')
    assert_close(xg.grad.cpu(), xr.grad, TOL, 'd loss / d x')
    want = {}
    for k, leaf in sd_o.items():
        want[k] = ref.backward(leaf.grad, *norm[k]) if k in norm else leaf.grad
    _cmp_grads(dict(d.named_parameters()), want, TOL, 'critic grad')


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


def _iteration(L, reals, zs, check=None):
    """One main iteration: generator step, then two critic steps."""
    losses = []
    L.set_requires_grad_disc(False)
    losses.append(L.g_step(zb=zs[0]))
    L.set_requires_grad_disc(True)
    for i in range(2):
        w_before = {k: p.detach().cpu().double() for k, p in L.disc_model.named_parameters() if k in L.sn.names}
        losses.append(L.d_step(reals[i], zb=zs[1 + i]))
        if check is not None:
            check(w_before)
    return [float(v) for v in losses]


def test_learner_hinge_spectral_norm(tmp_path):
    """ResNet GAN 32^2 with spectral_norm + hinge and no gradient penalty: finite losses; the stored sigma of every layer is
    u^T W v of the weights the critic step started from (recomputed in float64 from the saved state); a checkpoint restores
    u, v to the bit and the run continues as if it had never been saved."""
    L = _learner(spectral_norm=True, loss='hinge', gradient_penalty=None)
    assert L.sn is not None and L.disc_model.sn is L.sn
    reals, zs = _batches(12)

    def check(w_before):
        sd = {k: v.detach().cpu().double() for k, v in L.disc_model.state_dict().items()}
        for k, sg in L.sn.sigma().items():
            want = torch.dot(sd[k + '_u'], w_before[k].reshape(w_before[k].shape[0], -1) @ sd[k + '_v'])
            assert abs(sg.item() - want.item()) <= BOUND * abs(want.item()), k

    for it in range(3):
        losses = _iteration(L, reals[2 * it:2 * it + 2], zs[3 * it:3 * it + 3], check)
        assert all(np.isfinite(losses)), losses
    L.not_trained_yet = False
    path = tmp_path / 'resnetgan_model.tar'
    L.save_model(path)
    with pytest.raises(ValueError, match='reference_format'):
        L.save_model(path, reference_format=True)
    L2 = _learner(spectral_norm=True, loss='hinge', gradient_penalty=None)
    L2.load_model(path)
    L2.gen_model.train()
    L2.disc_model.train()
    sd, sd2 = L.disc_model.state_dict(), L2.disc_model.state_dict()
    assert list(sd.keys()) == list(sd2.keys())
    for k in sd:
        assert torch.equal(sd[k].cpu(), sd2[k].cpu()), k
    assert L2.disc_model.sn is L2.sn and L2.sn.arena is L2.arena_d
    a = _iteration(L, reals[6:8], zs[9:12])
    b = _iteration(L2, reals[6:8], zs[9:12])
    assert a == b, (a, b)


def test_default_learner_is_untouched():
    """spectral_norm off (the default): no manager, no override, the critic's keys as before."""
    from util import load_golden, sub
    L = _learner()
    assert L.sn is None and not L.disc_model.spectral_norm
    assert all(m.weight_override is None for m in L.disc_model.modules() if hasattr(m, 'weight_override'))
    assert list(L.disc_model.state_dict().keys()) == list(sub(load_golden('resnet32.npz'), 'd0.').keys())
