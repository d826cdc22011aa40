"""GPU tests of consistency regularisation (gan_lab_amd/consistency.py, csrc/cr.hip): the image transform against its definition
to the bit, the drawn parameter table, the two mean squared differences and their gradients against float64 within bounds derived
from the arithmetic, first order only, graph replay, and the learner's critic and generator steps with every term against a
float64 restatement (the oracle's networks with the terms of tests/cr_reference.py)."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cr_reference as ref
import sn_reference as sn_ref
from test_gpu_resnet import TOL, _cmp_grads
from util import assert_close, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff


# ---- 1: the transform and its parameter table ----------------------------------------------------------------------------------
def _table(n, s):
    """Hand-written rows: every corner (+-s, +-s), both flip values, (0, 0); cycled over the batch."""
    rows = [(f, dx, dy, 0) for f in (0, 1) for dx, dy in ((s, s), (s, -s), (-s, s), (-s, -s), (0, 0), (s, 0), (0, -s), (1, -1))]
    return [np.array([rows[(start + i) % len(rows)] for i in range(n)], dtype=np.int32) for start in range(0, len(rows), n)]


@pytest.mark.parametrize('shape,s', [((3, 3, 8, 8), 4), ((2, 3, 32, 32), 4), ((2, 1, 5, 7), 3), ((1, 3, 4, 4), 3)],
                         ids=['3x3x8x8', '2x3x32x32', '2x1x5x7', '1x3x4x4'])
def test_transform_is_bit_equal_to_its_definition(shape, s):
    from gan_lab_amd import ops
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    xg = x.cuda()
    tables = _table(shape[0], s)
    seen = set()
    for table in tables:
        seen.update(map(tuple, table[:, :3].tolist()))
        y = ops.cr_transform(xg, torch.from_numpy(table).cuda())
        assert torch.equal(y.cpu(), torch.from_numpy(ref.transform(x.numpy(), table))), table.tolist()
    assert all((f, dx, dy) in seen for f in (0, 1) for dx in (s, -s) for dy in (s, -s)) and (0, 0, 0) in seen and (1, 0, 0) in seen
    # an unaligned output view takes the one-element path: the same bits
    pad = torch.empty(x.numel() + 1, device='cuda')[1:].view(shape).copy_(xg)
    assert torch.equal(ops.cr_transform(pad, torch.from_numpy(tables[0]).cuda()).cpu(),
                       torch.from_numpy(ref.transform(x.numpy(), tables[0])))
    with pytest.raises(ValueError, match='params'):
        ops.cr_transform(xg, torch.zeros(shape[0] + 1, 4, dtype=torch.int32).cuda())
    with pytest.raises(RuntimeError, match='no adjoint'):
        ops.cr_transform(xg.clone().requires_grad_(True), torch.from_numpy(tables[0]).cuda())


def test_drawn_table():
    from gan_lab_amd import ops, rng
    n, s = 4096, 4
    t = ops.cr_params(n, s, True, 1234, 77, 'cuda')
    assert t.dtype == torch.int32 and tuple(t.shape) == (n, 4)
    c = t.cpu().numpy()
    assert set(np.unique(c[:, 0])) == {0, 1} and np.all(c[:, 3] == 0)
    for col in (1, 2):
        assert c[:, col].min() == -s and c[:, col].max() == s
        assert set(np.unique(c[:, col])) == set(range(-s, s + 1))            # over 4096 draws every value occurs
        counts = np.bincount(c[:, col] + s, minlength=2 * s + 1)
        assert np.all(np.abs(counts - n / 9) <= 6 * np.sqrt(n / 9 * 8 / 9))  # and none is far off uniform (6 sigma)
    assert abs(c[:, 0].mean() - 0.5) <= 6 * 0.5 / np.sqrt(n)
    assert torch.equal(t, ops.cr_params(n, s, True, 1234, 77, 'cuda'))       # same seed and offset: same table
    assert not torch.equal(t, ops.cr_params(n, s, True, 1234, 78, 'cuda'))
    assert torch.equal(t[1:], ops.cr_params(n - 1, s, True, 1234, 78, 'cuda'))   # row n is counter offset + n ...
    assert torch.equal(t[:16], ops.cr_params(16, s, True, 1234, 77, 'cuda'))    # ... so a short draw is a prefix of a long one
    noflip = ops.cr_params(n, s, False, 1234, 77, 'cuda')
    assert int(noflip[:, 0].abs().max()) == 0 and torch.equal(noflip[:, 1:], t[:, 1:])
    zero = ops.cr_params(64, 0, False, 5, 0, 'cuda')
    assert int(zero.abs().max()) == 0
    rng.manual_seed(11)
    a = rng.cr_params(8, 3, True)
    assert rng._STATE['offset'] == 8
    b = rng.cr_params(8, 3, True)
    assert rng._STATE['offset'] == 16
    rng.manual_seed(11)
    assert torch.equal(torch.cat((a, b)), rng.cr_params(16, 3, True))


# ---- 2, 3: the mean squared differences ------------------------------------------------------------------------------------------
def _check_sqdiff(value, ga, gb, a, b, what):
    """The derived bounds: each term is an fp32 difference (relative error u) squared in fp32 ((1 + u)^2 (1 + u)), the fp64 sum adds
    nothing visible, the result is rounded once more: relative error <= 4u of sum (a - b)^2 / n.  A gradient entry is three fp32
    roundings of (2 / n)(a - b): within 4 ulps."""
    a64, b64 = a.detach().cpu().double().numpy().ravel(), b.detach().cpu().double().numpy().ravel()
    want = np.mean((a64 - b64) ** 2)
    err = abs(float(value.detach().cpu().double()) - want)
    g_want, _ = ref.msd_grads(a64, b64)
    ulp = np.spacing(np.abs(g_want).astype(np.float32)).astype(np.float64)
    g_err = np.abs(ga.detach().cpu().double().numpy().ravel() - g_want)
    print(f'{what}: value rel err {err / max(want, 1e-300):.3e} (bound {4 * U:.3e}), worst gradient error '
          f'{(g_err / ulp).max():.3f} ulps (bound 4)')
    assert err <= 4 * U * want
    assert np.all(g_err <= 4 * ulp)
    assert torch.equal(gb.detach(), -ga.detach())


@pytest.mark.parametrize('n', [1, 5, 64, 257])
def test_msd_against_float64(n):
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(n)
    a, b = (3 * torch.randn(n, generator=g)).cuda().requires_grad_(True), torch.randn(n, 1, generator=g).cuda().requires_grad_(True)
    runs = []
    for _ in range(2):
        a.grad = b.grad = None
        v = ops.cr_msd(a, b)
        assert v.dim() == 0 and v.dtype == torch.float32
        v.backward()
        runs.append((v.detach().clone(), a.grad.clone(), b.grad.clone()))
    assert a.grad.shape == a.shape and b.grad.shape == b.shape
    _check_sqdiff(runs[0][0], runs[0][1], runs[0][2].view(-1), a, b, f'msd n={n}')
    assert all(torch.equal(s, t) for s, t in zip(*runs))                     # two runs: the same bits
    c = a.detach().clone().requires_grad_(True)                              # a == b: exactly 0, value and gradients
    d = a.detach().clone().requires_grad_(True)
    v = ops.cr_msd(c, d)
    v.backward()
    assert float(v.detach()) == 0.0 and float(c.grad.abs().max()) == 0.0 and float(d.grad.abs().max()) == 0.0
    with pytest.raises(ValueError, match='cr_msd'):
        ops.cr_msd(a, torch.zeros(n + 1).cuda())
    with pytest.raises(ValueError, match='cr_msd'):
        ops.cr_msd(torch.zeros(n, 2).cuda(), torch.zeros(n, 2).cuda())


@pytest.mark.parametrize('shape,halves', [((1, 3, 5, 7), False), ((2, 3, 32, 32), False), ((5, 3, 64, 64), False),
                                          ((4, 3, 32, 32), True)], ids=['1x3x5x7', '2x3x32x32', '5x3x64x64', 'halves-4x3x32x32'])
def test_imsd_against_float64(shape, halves):
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(shape[0] + shape[2])
    both = torch.tanh(torch.randn(2 * shape[0], *shape[1:], generator=g)).cuda()
    a = both[:shape[0]].clone().requires_grad_(True)
    b = both[shape[0]:].clone().requires_grad_(True)
    runs = []
    for _ in range(2):
        a.grad = b.grad = None
        v = ops.cr_imsd(a, b)
        assert v.dim() == 0 and v.dtype == torch.float32
        v.backward()
        runs.append((v.detach().clone(), a.grad.clone(), b.grad.clone()))
    _check_sqdiff(runs[0][0], runs[0][1], runs[0][2], a, b, f'imsd {shape}')
    assert all(torch.equal(s, t) for s, t in zip(*runs))
    if halves:
        # one (2N, ...) tensor: the same value, and ONE gradient tensor whose halves are the two-tensor form's, to the bit
        one = both.clone().requires_grad_(True)
        for _ in range(2):
            one.grad = None
            v = ops.cr_imsd(one)
            v.backward()
            assert one.grad.shape == one.shape and one.grad.is_contiguous()
            assert torch.equal(v.detach(), runs[0][0])
            assert torch.equal(one.grad[:shape[0]], runs[0][1]) and torch.equal(one.grad[shape[0]:], runs[0][2])
        with pytest.raises(ValueError, match='halves'):
            ops.cr_imsd(both[:3])
    # an unaligned operand is summed in the same order: the same bits
    off = torch.empty(a.numel() + 1, device='cuda')[1:].view(shape).copy_(a.detach())
    assert torch.equal(ops.cr_imsd(off, b.detach()), runs[0][0])
    c = a.detach().clone().requires_grad_(True)
    d = a.detach().clone().requires_grad_(True)
    v = ops.cr_imsd(c, d)
    v.backward()
    assert float(v.detach()) == 0.0 and float(c.grad.abs().max()) == 0.0 and float(d.grad.abs().max()) == 0.0
    with pytest.raises(ValueError, match='cr_imsd'):
        ops.cr_imsd(a, both)


# ---- 4: first order only; graph replay -----------------------------------------------------------------------------------------
def test_first_order_only():
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(40)
    a, b = torch.randn(9, generator=g).cuda().requires_grad_(True), torch.randn(9, generator=g).cuda().requires_grad_(True)
    x = torch.randn(4, 3, 8, 8, generator=g).cuda().requires_grad_(True)
    y = torch.randn(2, 3, 8, 8, generator=g).cuda().requires_grad_(True)
    for value, leaves in ((ops.cr_msd(a, b), (a, b)), (ops.cr_imsd(x[:2], y), (x, y)), (ops.cr_imsd(x), (x,))):
        first = torch.autograd.grad(value, leaves, create_graph=True)
        with pytest.raises(RuntimeError, match='first order only.*differentiate twice'):
            torch.autograd.grad(sum(f.sum() for f in first), leaves)


def test_ops_replay_from_a_graph():
    """No host readback, no upload: draw, transform, both reductions and their backward captured on one stream replay to the bits
    of the eager run."""
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(41)
    a, b = torch.randn(64, generator=g).cuda().requires_grad_(True), torch.randn(64, generator=g).cuda().requires_grad_(True)
    x = torch.randn(4, 3, 32, 32, generator=g).cuda()
    both = torch.randn(4, 3, 32, 32, generator=g).cuda().requires_grad_(True)

    def run():
        table = ops.cr_params(4, 4, True, 99, 5, 'cuda')
        y = ops.cr_transform(x, table)
        m, i = ops.cr_msd(a, b), ops.cr_imsd(both)
        return (table, y, m, i) + torch.autograd.grad(m, (a, b)) + torch.autograd.grad(i, (both,))

    eager = [t.detach().clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.detach().zero_()                  # a capture records, it does not run
    graph.replay()
    torch.cuda.synchronize()
    for s, t in zip(eager, outs):
        assert torch.equal(s, t.detach())
    assert float(eager[2]) > 0 and float(eager[3]) > 0 and int(eager[0].abs().max()) > 0


# ---- 5: the steps -----------------------------------------------------------------------------------------------------------------
RECIPES = {'wgan-gp': {}, 'hinge-sn': dict(loss='hinge', spectral_norm=True, gradient_penalty=None)}
ALL_ON = dict(cr_real=10., cr_fake=10., cr_latent_d=5., cr_latent_g=0.5)
B = 4
GOLD = load_golden('resnet32.npz')          # the width, latent length and batch of test_gpu_resnet's own step checks


def _learner(seed=7, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=B,
                      num_iters_save_model=10 ** 9, log_every=0, len_latent=int(GOLD['len_latent']), lr_base=0., random_seed=seed,
                      **kw)
    cfg.fmap_g, cfg.fmap_d = int(GOLD['fmap_g']), int(GOLD['fmap_d'])
    torch.manual_seed(seed)
    L = GANLearner(cfg)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                   # every bias and norm affine away from its initial 0 / 1, the projection from 0
        for m in (L.gen_model, L.disc_model):
            for k, p in m.named_parameters():
                if k.endswith('bias') or k == 'proj.linear.weight':
                    p.copy_((0.1 * torch.randn(*p.shape, generator=gen)).cuda())
                elif '.norm.' in k:
                    p.add_((0.2 * torch.randn(*p.shape, generator=gen)).cuda())
    L.gen_model.train()
    L.disc_model.train()
    return L


def _draws(seed=3):
    g = torch.Generator().manual_seed(seed)
    n_lat = int(GOLD['len_latent'])
    s = 4
    rows = [(1, s, -s, 0), (0, -s, s, 0), (1, 0, 0, 0), (0, 2, 1, 0), (0, s, s, 0), (1, -s, -s, 0), (0, 0, 0, 0), (1, -1, 3, 0)]
    return dict(real=torch.rand(B, 3, 32, 32, generator=g) * 2 - 1, zd=torch.randn(B, n_lat, generator=g),
                zg=torch.randn(B, n_lat, generator=g), eps=torch.rand(B, 1, 1, 1, generator=g),
                noise_d=torch.randn(B, n_lat, generator=g), noise_g=torch.randn(B, n_lat, generator=g),
                params=np.array(rows, dtype=np.int32), labels=torch.tensor([0, 2, 2, 1]))


def _dbl(sd):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}


def _gen64(sd, z, labels=None):
    """The 32-pixel generator in training mode, float64, on the oracle's blocks; (K, C) norm tables are indexed by the labels."""
    from oracle import resnet

    def norm(key, t):
        w, b = sd[key + '.norm.weight'], sd[key + '.norm.bias']
        y = F.batch_norm(t, None, None, None, None, training=True, eps=resnet.EPS_NORM)
        if w.dim() == 2:
            return y * w[labels][:, :, None, None] + b[labels][:, :, None, None]
        return y * w[None, :, None, None] + b[None, :, None, None]

    p = 'generator_model.'
    w = sd[p + '1.linear.weight']
    h = F.linear(z, w, sd[p + '1.linear.bias']).view(z.shape[0], w.shape[0] // 16, 4, 4)
    for i in range(3):
        h = resnet._resblock(sd, f'{p}{3 + i}.', h, norm, 'up', pix32=True)
    return torch.tanh(resnet._conv(sd, f'{p}8', F.relu(norm(f'{p}6', h))))


def _disc64(sd, x, labels=None):
    """The 32-pixel critic, float64, on the oracle's blocks (oracle.resnet.disc_forward's 32-pixel branch), plus the projection."""
    from oracle import resnet
    norm = lambda key, t: resnet._ln(sd, key, t)  # noqa: E731
    h1 = F.relu(resnet._conv(sd, 'conv1.conv_layer_1.0', x))
    h = resnet._pool(resnet._conv(sd, 'conv1.conv_layer_2.0', h1)) + resnet._conv(sd, 'conv1.skip_connection.1', resnet._pool(x))
    h = resnet._resblock(sd, 'resblocks.0.', h, norm, 'pool', pix32=True)
    h = resnet._resblock(sd, 'resblocks.1.', h, norm, None, pix32=True)
    h = resnet._resblock(sd, 'resblocks.2.', h, norm, None, pix32=True)
    f = F.relu(h).mean(dim=(2, 3))
    out = F.linear(f, sd['linear1.linear.weight'], sd['linear1.linear.bias']).view(-1)
    if labels is not None:
        out = out + (sd['proj.linear.weight'][labels] * f).sum(dim=1)
    return out


class _Restated(object):
    """The float64 restatement of one learner's steps: its state_dict in the networks above; with spectral normalisation the critic
    runs on W_sn (from the u, v the step starts from) and the gradients towards W_sn are pushed through the reference backward."""

    def __init__(self, L, iterate):
        self.g = {k: v.requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in _dbl(L.gen_model.state_dict()).items()}
        raw = _dbl(L.disc_model.state_dict())
        self.norm, self.d = {}, {}
        for k, v in raw.items():
            if k.endswith(('weight_u', 'weight_v')):
                continue
            if k + '_u' in raw:
                u, vv, sigma, wsn = sn_ref.refresh(v, raw[k + '_u'], raw[k + '_v'], iterate=iterate)
                self.norm[k] = (v, u, vv, sigma)
                v = wsn
            self.d[k] = v.clone().requires_grad_(True)
        self.hinge = L.loss == 'hinge'
        self.gp = L.gradient_penalty

    def disc(self, labels, frozen=False):
        sd = {k: v.detach() for k, v in self.d.items()} if frozen else self.d
        return lambda x: _disc64(sd, x.double(), labels)

    def gen(self, labels):
        n = None if labels is None else labels.shape[0]
        return lambda z: _gen64(self.g, z.double(), None if labels is None else labels.repeat(z.shape[0] // n))

    def d_grads(self):
        return {k: (sn_ref.backward(v.grad, *self.norm[k]) if k in self.norm else v.grad).numpy() for k, v in self.d.items()}

    def g_grads(self):
        return {k: v.grad.numpy() for k, v in self.g.items() if v.requires_grad}

    def d_step(self, w, dr, labels=None):
        from oracle import step as ostep
        terms, (g_z, d_gen, d_real) = ref.critic_terms(
            self.disc(labels), self.gen(labels), dr['real'].double(), dr['zd'].double(), dr['noise_d'].double(), dr['params'],
            w['cr_sigma'], real=w['cr_real'] > 0, fake=w['cr_fake'] > 0, latent=w['cr_latent_d'] > 0)
        loss = sn_ref.hinge_disc(d_gen, d_real) if self.hinge else (d_gen - d_real).mean()
        if self.gp is not None:
            loss = loss + ostep.calc_gp(self.disc(labels), self.gp, g_z, dr['real'].double(), 10.0, 1.0, dr['eps'].double())
        for k, v in terms.items():
            loss = loss + w[k] * v
        loss.backward()
        return loss.detach(), {k: v.detach() for k, v in terms.items()}

    def g_step(self, w, dr, labels=None):
        if w['cr_latent_g'] > 0:
            term, fake = ref.generator_term(self.gen(labels), dr['zg'].double(), dr['noise_g'].double(), w['cr_sigma'])
        else:
            term, fake = None, self.gen(labels)(dr['zg'])
        loss = -self.disc(labels, frozen=True)(fake).mean()             # wgan and hinge share the generator loss
        if term is not None:
            loss = loss - w['cr_latent_g'] * term
        loss.backward()
        return loss.detach(), ({} if term is None else {'cr_latent_g': term.detach()})


def _weights(L):
    cr = L.cr
    return dict(cr_real=cr.real, cr_fake=cr.fake, cr_latent_d=cr.latent_d, cr_latent_g=cr.latent_g, cr_sigma=cr.sigma)


def _run_g(L, dr, labels=None):
    L.set_requires_grad_disc(False)
    loss = L.g_step(zb=dr['zg'].cuda(), labels=labels, cr_noise=dr['noise_g'].cuda())
    L.set_requires_grad_disc(True)
    return loss


def _run_d(L, dr, labels=None):
    return L.d_step(dr['real'].cuda(), zb=dr['zd'].cuda(), eps_interp=dr['eps'].cuda(), labels=labels,
                    cr_noise=dr['noise_d'].cuda(), cr_params=torch.from_numpy(dr['params']).cuda())


def _check_against_restatement(L, dr, what, labels=None):
    """One generator step and one critic step of ``L`` (lr = 0: the parameters stay) against the float64 restatement, with
    test_gpu_resnet's helper and bar."""
    w = _weights(L)
    dev_labels = None if labels is None else labels.int().cuda()
    for name, run, iterate in (('g', _run_g, False), ('d', _run_d, True)):
        R = _Restated(L, iterate)                                            # the state the step starts from
        L.last_losses = {}
        loss = run(L, dr, dev_labels)
        want, terms = (R.g_step if name == 'g' else R.d_step)(w, dr, labels)
        print(f'{what} {name}_step: loss {float(loss):.6f} (float64 {float(want):.6f}) terms '
              f'{ {k: float(v) for k, v in L.last_losses.items()} } (float64 { {k: float(v) for k, v in terms.items()} })')
        assert_close(loss.cpu().double(), want, TOL, f'{what} loss_{name}')
        assert sorted(L.last_losses) == sorted(terms), (sorted(L.last_losses), sorted(terms))
        for k, v in terms.items():
            assert L.last_losses[k].is_cuda and L.last_losses[k].dim() == 0          # a device tensor, not a host float
            assert_close(L.last_losses[k].cpu().double(), v, TOL, f'{what} last_losses[{k}]')
        model, grads = (L.gen_model, R.g_grads()) if name == 'g' else (L.disc_model, R.d_grads())
        _cmp_grads(model, grads, TOL, f'{what} {name} grad')


def _set(L, **w):
    L.cr.real, L.cr.fake, L.cr.latent_d, L.cr.latent_g = (float(w.get(k, 0.)) for k in ('cr_real', 'cr_fake', 'cr_latent_d',
                                                                                       'cr_latent_g'))


def _snapshot(L, model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_weights_at_zero_leave_the_iteration_bit_identical(recipe):
    """(a) drawn latents, so the Philox stream is in play: the same losses, gradients and stream position, to the bit."""
    from gan_lab_amd import rng
    real = _draws()['real'].cuda()
    out = []
    # The first learner is a warm-up and is not compared: the plain critic step of a process's FIRST learner rounds its gradients
    # unlike every later one (measured on the code without the fields: learners A, B, C, D built alike give B = C = D to the bit
    # and A 1e-7 away in 14 critic gradients, losses equal) - a property of the step as it was, not of these fields.
    for kw in ({}, {}, dict(cr_real=0., cr_fake=0., cr_latent_d=0., cr_latent_g=0., cr_sigma=0.05, cr_shift=2, cr_flip=False)):
        gc.collect()
        torch.cuda.empty_cache()
        L = _learner(**RECIPES[recipe], **kw)
        assert L.cr is None
        L.set_requires_grad_disc(False)
        lg = L.g_step()
        gg = _snapshot(L, L.gen_model)
        L.set_requires_grad_disc(True)
        ld = L.d_step(real)
        cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
        out.append((lg.cpu(), ld.cpu(), cpu(gg), cpu(_snapshot(L, L.disc_model)), rng._STATE['offset'], list(L.last_losses)))
        del L, lg, ld, gg              # nothing of this learner stays on the device
    (lg0, ld0, gg0, gd0, off0, ll0), (lg1, ld1, gg1, gd1, off1, ll1) = out[1:]
    assert torch.equal(lg0, lg1) and torch.equal(ld0, ld1) and off0 == off1 > 0
    assert gg0.keys() == gg1.keys() and gd0.keys() == gd1.keys() and len(gg0) > 10 and len(gd0) > 10
    assert all(torch.equal(gg0[k], gg1[k]) for k in gg0) and all(torch.equal(gd0[k], gd1[k]) for k in gd0)
    assert not any(k.startswith('cr_') for k in ll0) and not any(k.startswith('cr_') for k in ll1)


CASES = [dict(cr_real=10.), dict(cr_fake=10.), dict(cr_latent_d=5.), dict(cr_latent_g=0.5), ALL_ON]


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_steps_match_the_float64_restatement(recipe):
    """(b) each weight on alone, then all four together."""
    L = _learner(**RECIPES[recipe], **ALL_ON)
    dr = _draws()
    for case in CASES:
        _set(L, **case)
        _check_against_restatement(L, dr, f'{recipe} {"+".join(case)}')
    _set(L, **ALL_ON)
    # drawn perturbation and table: the stream advances by the draws of the terms, and the terms are reported
    from gan_lab_amd import rng
    before = rng._STATE['offset']
    L.d_step(dr['real'].cuda(), zb=dr['zd'].cuda())
    n_lat = int(GOLD['len_latent'])
    assert rng._STATE['offset'] - before == (B * n_lat + 3) // 4 + 2 * B
    assert all(np.isfinite(float(L.last_losses[k])) for k in ('cr_real', 'cr_fake', 'cr_latent_d'))
    with pytest.raises(ValueError, match='cr_params'):
        L.d_step(dr['real'].cuda(), zb=dr['zd'].cuda(), cr_params=torch.zeros(B, 4, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match='cr_noise'):
        L.d_step(dr['real'].cuda(), zb=dr['zd'].cuda(), cr_noise=torch.zeros(B, 3).cuda())


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_identity_transform_adds_nothing(recipe):
    """(c) cr_shift=0, cr_flip=False: T(x) = x, so both bCR terms vanish - up to the tiling of the rows of a larger critic batch -
    and the critic's gradients are those of the plain step."""
    dr = _draws()
    dr['params'] = np.zeros_like(dr['params'])
    plain = _learner(**RECIPES[recipe])
    L = _learner(**RECIPES[recipe], cr_real=10., cr_fake=10., cr_shift=0, cr_flip=False)
    with torch.no_grad():
        d_max = max(float(L.disc_model(dr['real'].cuda()).abs().max()), float(L.disc_model(L.gen_model(dr['zd'].cuda())).abs().max()))
    L.gen_model.load_state_dict(plain.gen_model.state_dict())               # the probe above moved the running statistics only
    for drawn in (False, True):
        # the plain learner takes the same number of critic updates: lr = 0 keeps the weights, but spectral normalisation's u, v
        # make one power iteration per update
        _run_d(plain, dr)
        want = {k: v.cpu().numpy() for k, v in _snapshot(plain, plain.disc_model).items()}
        L.last_losses = {}
        if drawn:
            L.d_step(dr['real'].cuda(), zb=dr['zd'].cuda(), eps_interp=dr['eps'].cuda())      # the drawn table is all zeros too
        else:
            _run_d(L, dr)
        for k in ('cr_real', 'cr_fake'):
            print(f'{recipe} drawn={drawn} {k}: {float(L.last_losses[k]):.3e} (bound {(1e-5 * d_max) ** 2:.3e})')
            assert 0.0 <= float(L.last_losses[k]) <= (1e-5 * d_max) ** 2
        _cmp_grads(L.disc_model, want, TOL, f'{recipe} identity d grad')


def test_projection_labels_reach_every_part():
    """(d) cgan='projection' with 3 classes, all terms on: one generator and one critic step against the restatement, in which every
    part is produced and scored under the batch's labels."""
    L = _learner(cgan='projection', num_classes=3, **ALL_ON)
    dr = _draws()
    _check_against_restatement(L, dr, 'projection all', labels=dr['labels'])
    other = dict(dr, labels=torch.tensor([1, 0, 0, 2]))          # other labels: other terms (the labels do reach the parts)
    a = {k: float(v) for k, v in _Restated(L, True).d_step(_weights(L), dr, dr['labels'])[1].items()}
    b = {k: float(v) for k, v in _Restated(L, True).d_step(_weights(L), other, other['labels'])[1].items()}
    assert all(abs(a[k] - b[k]) > 1e-3 * abs(a[k]) for k in a), (a, b)


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_unpaired_critic_passes_agree_with_the_paired_pass(recipe, monkeypatch):
    """(e) GANLAB_RESNET_PAIR=0: every critic input makes a pass of its own; the loss and gradients of the one-pass path."""
    dr = _draws()
    out = {}
    for pair in ('1', '0'):
        monkeypatch.setenv('GANLAB_RESNET_PAIR', pair)
        L = _learner(**RECIPES[recipe], **ALL_ON)
        assert L._pair_critic_batches(dr['real'], dr['real']) == (pair == '1')
        loss = _run_d(L, dr)
        out[pair] = (loss.cpu(), {k: v.cpu().numpy() for k, v in _snapshot(L, L.disc_model).items()},
                     {k: v.cpu() for k, v in L.last_losses.items()}, L)
    assert_close(out['0'][0], out['1'][0], TOL, 'loss_d')
    for k in ('cr_real', 'cr_fake', 'cr_latent_d'):
        assert_close(out['0'][2][k], out['1'][2][k], TOL, k)
    _cmp_grads(out['0'][3].disc_model, out['1'][1], TOL, f'{recipe} unpaired d grad')


@pytest.mark.parametrize('kw', [dict(ada='blit'), dict(diffaugment='color')], ids=['ada', 'diffaugment'])
def test_augmentations_are_excluded(kw):
    """(f)"""
    with pytest.raises(ValueError, match=list(kw)[0]):
        _learner(cr_real=10., **kw)
    with pytest.raises(ValueError, match=list(kw)[0]):
        _learner(cr_latent_g=0.5, **kw)
