"""GPU tests of latent-space projection: csrc/project.hip (``ops.pyramid_mse``, ``ops.w_moments``, ``ops.project_step``) against the
float64 reference of tests/project_reference.py, ``StyleGenerator.synthesis`` against ``forward``, and ``StyleGANLearner.project``
end to end.  Where a bar is "the float32 restatement's error times 2", the restatement is the same reference run in float32 on the
CPU, on the same inputs; both errors are printed before the assertion."""
import pytest
import torch

import project_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _widths():
    from gan_lab_amd import progressive as P
    P.FMAP_BASE, P.FMAP_MAX = 64, 16
    yield
    P.FMAP_BASE, P.FMAP_MAX = 8192, 512


def make_learner(seed=1):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    cfg = make_config('stylegan', dev='cuda', pin_memory=False, res_samples=16, res_dataset=16, init_res=16, batch_size=4,
                      len_latent=16, len_dlatent=16, mapping_num_fcs=2, cutoff_trunc_trick=None, nimg_transition=24,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=seed, loss='nonsaturating', gradient_penalty='r1')
    torch.manual_seed(seed)                                  # the layers' initial weights come from torch's generator
    L = StyleGANLearner(cfg)
    L.ds_mean, L.ds_std = torch.full((3,), .5), torch.full((3,), .25)
    with torch.no_grad():
        for k, p in L.gen_model.named_parameters():
            if k.endswith('bias') or k.endswith('noise_weight'):
                p.normal_(0, 0.3)
    L.ewma.flat.copy_(L.arena_g.flat)
    return L


def layer_noise(gen, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, 1, 4 * 2 ** (k // 2), 4 * 2 ** (k // 2), generator=g).cuda() for k in range(len(gen.gen_layers))]


# ---- pyramid_mse ---------------------------------------------------------------------------------------------------------------
def _integers(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, shape, generator=g).float(), torch.randint(-4, 5, shape, generator=g).float())


EXACT = [((2, 1, 4, 4), [1., 1., 1.]), ((2, 4, 32, 32), [1.] * 6), ((2, 4, 64, 64), [1., .5, .25, 2., 4., 1.]),
         ((2, 1, 64, 64), [0., 0., 0., 0., 0., 1.])] + \
        [((1, 4, 32, 32), [float(l == k) for l in range(6)]) for k in range(6)]


@pytest.mark.parametrize('shape,weights', EXACT, ids=[f'{"x".join(map(str, s))}-{i}' for i, (s, _) in enumerate(EXACT)])
def test_pyramid_mse_is_exact_on_integer_images(shape, weights):
    """Integer-valued images, power-of-two weights and channel counts: every difference, mean, square and sum is exact in the
    kernel's formats, so terms, loss and gradient equal the float64 reference bit for bit once it is rounded to float32."""
    from gan_lab_amd import ops
    x, t = _integers(shape, 0)
    xg = x.cuda().requires_grad_(True)
    loss, terms = ops.pyramid_mse(xg, t.cuda(), weights)
    grad, = torch.autograd.grad(loss.sum(), xg)
    x64, t64 = x.double(), t.double()
    assert torch.equal(terms.cpu(), ref.pyramid_terms(x64, t64, len(weights)).float())
    assert torch.equal(loss.cpu(), ref.pyramid_loss(x64, t64, weights).float())
    want = ref.pyramid_grad_analytic(x64, t64, weights)
    assert torch.equal(want, ref.pyramid_grad_autograd(x64, t64, weights))
    assert torch.equal(grad.cpu(), want.float())
    assert loss.shape == (shape[0],) and terms.shape == (shape[0], len(weights)) and not terms.requires_grad
    assert want.abs().max() > 0


def test_pyramid_mse_real_valued_against_float64():
    """(3, 3, 64, 64), six levels.  Bar: twice the error of the float32 torch restatement on the same inputs (measured values:
    DESIGN.md 4.21)."""
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(3, 3, 64, 64, generator=g), torch.randn(3, 3, 64, 64, generator=g)
    weights = [1., .5, .25, 2., 4., 1.]
    want_loss, want_grad = ref.pyramid_loss(x.double(), t.double(), weights), ref.pyramid_grad_autograd(x.double(), t.double(), weights)
    bar_loss = ((ref.pyramid_loss(x, t, weights).double() - want_loss).abs() / want_loss).max().item()
    bar_grad = ref.rel_err(ref.pyramid_grad_autograd(x, t, weights), want_grad)
    xg = x.cuda().requires_grad_(True)
    loss, terms = ops.pyramid_mse(xg, t.cuda(), weights)
    grad, = torch.autograd.grad(loss.sum(), xg)
    err_loss = ((loss.cpu().double() - want_loss).abs() / want_loss).max().item()
    err_grad = ref.rel_err(grad, want_grad)
    print(f'pyramid_mse (3, 3, 64, 64): value {err_loss:.3e} (float32 restatement {bar_loss:.3e}), gradient {err_grad:.3e} '
          f'(float32 restatement {bar_grad:.3e})')
    assert bar_loss > 0 and bar_grad > 0
    assert err_loss <= 2 * bar_loss and err_grad <= 2 * bar_grad
    # loss and terms are roundings of the same fp64 numbers: recombining the rounded terms moves the loss by two roundings at most
    recombined = (terms.cpu().double() * torch.tensor(weights, dtype=torch.float64)).sum(1)
    assert ((recombined - loss.cpu().double()).abs() <= 2 ** -23 * recombined).all()


def test_pyramid_mse_is_reproducible_and_scales_rows():
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(4)
    x, t = torch.randn(3, 3, 64, 64, generator=g).cuda(), torch.randn(3, 3, 64, 64, generator=g).cuda()
    weights = [1.] * 6
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        loss, terms = ops.pyramid_mse(xg, t, weights)
        runs.append((loss, terms, torch.autograd.grad(loss.sum(), xg)[0]))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    xg = x.clone().requires_grad_(True)
    loss, _ = ops.pyramid_mse(xg, t, weights)
    up = torch.tensor([2., 0., -1.]).cuda()
    scaled, = torch.autograd.grad(loss, xg, grad_outputs=up)
    base = runs[0][2]
    assert torch.equal(scaled[0], base[0] * 2) and torch.equal(scaled[2], -base[2])
    assert torch.equal(scaled[1], torch.zeros_like(base[1])) and base[1].abs().max() > 0
    # first order only, and no gradient for the target
    xg = x.clone().requires_grad_(True)
    loss, _ = ops.pyramid_mse(xg, t, weights)
    first, = torch.autograd.grad(loss.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError, match='first order only'):
        first.sum().backward()
    with pytest.raises(RuntimeError, match='target'):
        ops.pyramid_mse(x, t.clone().requires_grad_(True), weights)
    for bad in (dict(weights=[1.] * 7), dict(weights=[]), dict(weights=[-1.])):
        with pytest.raises(ValueError, match='weights'):
            ops.pyramid_mse(x, t, **bad)
    with pytest.raises(ValueError, match='power of two'):
        ops.pyramid_mse(x[..., :48, :48], t[..., :48, :48], [1.])


# ---- w_moments -----------------------------------------------------------------------------------------------------------------
def test_w_moments_against_float64():
    """Rows 100 + randn at (1000, 16).  Bar: the float32 two-pass torch restatement's error times 2 (measured: DESIGN.md 4.21)."""
    from gan_lab_amd import ops
    ws = 100 + torch.randn(1000, 16, generator=torch.Generator().manual_seed(5))
    want_avg, want_std = ref.w_moments(ws.double())
    r_avg, r_std = ref.w_moments(ws)
    bar_avg, bar_std = ref.rel_err(r_avg, want_avg), ref.rel_err(r_std, want_std)
    avg, std = ops.w_moments(ws.cuda())
    err_avg, err_std = ref.rel_err(avg, want_avg), ref.rel_err(std, want_std)
    print(f'w_moments (1000, 16): w_avg {err_avg:.3e} (float32 restatement {bar_avg:.3e}), w_std {err_std:.3e} (float32 '
          f'restatement {bar_std:.3e})')
    assert avg.shape == (16,) and std.shape == ()
    assert err_avg <= 2 * bar_avg and err_std <= 2 * bar_std
    again = ops.w_moments(ws.cuda())
    assert torch.equal(again[0], avg) and torch.equal(again[1], std)
    wide = torch.randn(37, 130, generator=torch.Generator().manual_seed(6))      # three column blocks, the last one partial
    avg, std = ops.w_moments(wide.cuda())
    want_avg, want_std = ref.w_moments(wide.double())
    assert ref.rel_err(avg, want_avg) <= 2 ** -23 and ref.rel_err(std, want_std) <= 2 ** -23


# ---- project_step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', ['w', 'w+'])
def test_project_step_follows_the_float64_restatement(space):
    """N = 2, L = 6, D = 16, num_steps = 8: the eight steps cross the ramp-up, the plateau, the ramp-down and the end of the noise
    ramp.  After every step w_opt, m, v and w_in are compared with the float64 restatement; bar per quantity: the float32
    restatement's largest error over the steps, times 2 (measured: DESIGN.md 4.21)."""
    from gan_lab_amd import ops
    n, layers, d, num_steps, w_std = 2, 6, 16, 8, 0.75
    g = torch.Generator().manual_seed(7)
    shape = (n, d) if space == 'w' else (n, layers, d)
    w0 = torch.randn(shape, generator=g)
    grads = [torch.randn(n, layers, d, generator=g) * 10 ** float(torch.randn((), generator=g)) for _ in range(num_steps)]
    noises = [torch.randn(shape, generator=g) for _ in range(num_steps + 1)]
    hyper = (0.1, 0.05, 0.25, 0.05, 0.75, float(num_steps))

    def fresh(dtype):
        return dict(w_opt=w0.to(dtype), m=torch.zeros(shape, dtype=dtype), v=torch.zeros(shape, dtype=dtype), step=0)

    s64, s32 = fresh(torch.float64), fresh(torch.float32)
    w_opt, m, v = w0.cuda(), torch.zeros(shape).cuda(), torch.zeros(shape).cuda()
    step, std_dev = torch.zeros(1, dtype=torch.int32).cuda(), torch.tensor(w_std).cuda()
    w_in = torch.empty(n, layers, d).cuda()
    ops.project_step(w_opt, None, m, v, step, noises[0].cuda(), std_dev, w_in, hyper)
    assert step.item() == 0 and torch.equal(w_opt.cpu(), w0)
    first = ref.w_in(s64, noises[0], w_std, num_steps, layers)
    assert ref.rel_err(w_in, first) <= 2 ** -23
    errs, bars = {}, {}
    for k in range(num_steps):
        want_in = ref.project_step(s64, grads[k], noises[k + 1], w_std, num_steps)
        rest_in = ref.project_step(s32, grads[k], noises[k + 1], w_std, num_steps)
        ops.project_step(w_opt, grads[k].cuda(), m, v, step, noises[k + 1].cuda(), std_dev, w_in, hyper)
        for name, ours, rest, want in (('w_opt', w_opt, s32['w_opt'], s64['w_opt']), ('m', m, s32['m'], s64['m']),
                                       ('v', v, s32['v'], s64['v']), ('w_in', w_in, rest_in, want_in)):
            errs[name] = max(errs.get(name, 0.), ref.rel_err(ours, want))
            bars[name] = max(bars.get(name, 0.), ref.rel_err(rest, want))
    print(f'project_step {space}: ' + ', '.join(f'{k} {errs[k]:.3e} (float32 restatement {bars[k]:.3e})' for k in errs))
    assert step.item() == num_steps and s64['step'] == num_steps
    assert not torch.equal(w_opt.cpu(), w0)
    for name in errs:
        assert errs[name] <= 2 * bars[name], name
    assert torch.equal(w_in.cpu(), (w_opt.cpu().unsqueeze(1).expand(n, layers, d) if space == 'w' else w_opt.cpu()))   # noise ramp over


# ---- synthesis -----------------------------------------------------------------------------------------------------------------
def test_synthesis_matches_forward_bit_for_bit_and_in_gradient():
    L = make_learner()
    gen = L.gen_model.eval()
    assert not gen.use_truncation_trick and len(gen.gen_layers) == 6
    n, layers = 3, 6
    z = torch.randn(n, 16, generator=torch.Generator().manual_seed(8)).cuda()
    noise = layer_noise(gen, n, 9)
    kept = []
    hook = gen.z_to_w.register_forward_hook(lambda mod, args, out: kept.append(out))
    try:
        img = gen(z, noise=noise)
    finally:
        hook.remove()
    w = kept[0]
    with torch.no_grad():
        assert torch.equal(gen.synthesis(w.detach(), noise=noise), img)
        assert torch.equal(gen.synthesis(w.detach().unsqueeze(1).expand(n, layers, 16), noise=noise), img)
    functional = torch.randn(img.shape, generator=torch.Generator().manual_seed(10)).cuda()
    g_w, = torch.autograd.grad((img * functional).sum(), w)
    ws = w.detach().unsqueeze(1).expand(n, layers, 16).contiguous().requires_grad_(True)
    g_ws, = torch.autograd.grad((gen.synthesis(ws, noise=noise) * functional).sum(), ws)
    assert g_ws.shape == (n, layers, 16) and all(g_ws[:, k].abs().max() > 0 for k in range(layers))
    total, mass = g_ws.double().sum(1), g_ws.double().abs().sum(1)
    bound = 2 * (layers - 1) * 2.0 ** -24 * mass              # either side sums L terms in fp32, in its own order
    assert ((g_w.double() - total).abs() <= bound).all(), ((g_w.double() - total).abs() / mass).max().item()
    # W form: one (N, D) tensor feeds every layer, its gradient is the accumulated one
    w2 = w.detach().clone().requires_grad_(True)
    g_w2, = torch.autograd.grad((gen.synthesis(w2, noise=noise) * functional).sum(), w2)
    assert ((g_w2.double() - total).abs() <= bound).all()


def test_refusals_on_the_device():
    L = make_learner()
    target = torch.rand(2, 3, 16, 16).cuda()
    with pytest.raises(ValueError, match='targets'):
        L.project(torch.rand(2, 3, 8, 8).cuda(), steps=2, w_avg_samples=8)
    L.gen_model.fade_in_phase = True
    try:
        with pytest.raises(ValueError, match='fade_in_phase'):
            L.project(target, steps=2, w_avg_samples=8)
        with pytest.raises(ValueError, match='fade_in_phase'):
            L.gen_model.synthesis(torch.zeros(2, 16).cuda())
    finally:
        L.gen_model.fade_in_phase = False


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def projected():
    """One learner, targets of its own EWMA generator under the projection's own noise maps, and two projections of them."""
    from gan_lab_amd import ops, progressive as P, project
    old = (P.FMAP_BASE, P.FMAP_MAX)
    P.FMAP_BASE, P.FMAP_MAX = 64, 16
    try:
        L = make_learner()
        seed, n = 11, 2
        gen = L.materialize_lagged_generator().cuda().eval()
        L.gen_model_lagged = None
        maps, offset = [], 0
        for k in range(len(gen.gen_layers)):
            side = 4 * 2 ** (k // 2)
            maps.append(ops.randn((1, 1, side, side), project._substream(seed, 1), offset, 'cuda'))
            offset += (side * side + 3) // 4
        z = torch.randn(n, 16, generator=torch.Generator().manual_seed(12)).cuda()
        with torch.no_grad():
            w_star = gen.z_to_w(z)
            target = (gen.synthesis(w_star, noise=maps) * L.ds_std.cuda().view(1, 3, 1, 1) + L.ds_mean.cuda().view(1, 3, 1, 1))
        runs = [L.project(target, steps=100, space='w', noise_mode='const', seed=seed, w_avg_samples=512) for _ in range(2)]
        yield L, target, runs
    finally:
        P.FMAP_BASE, P.FMAP_MAX = old


def test_projection_lowers_the_loss_and_repeats(projected):
    L, target, (a, b) = projected
    assert a.ws.shape == (2, 6, 16) and a.images.shape == target.shape and a.loss.shape == (100, 2) and a.loss.is_cuda
    assert a.w_avg.shape == (16,) and a.w_std.shape == () and a.w_std.item() > 0
    loss = a.loss.cpu()
    assert torch.isfinite(loss).all() and torch.isfinite(a.ws).all() and torch.isfinite(a.images).all()
    print('projection at 16x16, 100 steps, W: final / first loss per target =', (loss[-1] / loss[0]).tolist())
    assert (loss[-1] < loss[0]).all()
    assert torch.equal(a.ws, b.ws) and torch.equal(a.loss, b.loss) and torch.equal(a.images, b.images)
    assert torch.equal(a.ws[:, 0], a.ws[:, 5]) and not torch.equal(a.ws[0], a.ws[1])      # W: one dlatent per target


def test_projection_in_w_plus_and_without_noise(projected):
    L, target, _ = projected
    out = L.project(target, steps=12, space='w+', noise_mode='none', levels=3, weights=[1., 2., 4.], seed=2, w_avg_samples=64,
                    time_average=False, lr0=0.05)
    loss = out.loss.cpu()
    assert out.ws.shape == (2, 6, 16) and loss.shape == (12, 2) and torch.isfinite(loss).all()
    assert not torch.equal(out.ws[:, 0], out.ws[:, 5])                                     # W+: the layers part ways


def test_project_leaves_the_learner_as_found():
    def snapshot(L):
        snap = {'arena_g': L.arena_g.flat.clone(), 'gflat_g': L.arena_g.gflat.clone(), 'arena_d': L.arena_d.flat.clone(),
                'gflat_d': L.arena_d.gflat.clone(), 'ewma': L.ewma.flat.clone()}
        for tag, opt, model in (('g', L.opt_gen, L.gen_model), ('d', L.opt_disc, L.disc_model)):
            mom = opt.export_moments(list(model.named_parameters()))
            snap[f'opt_{tag}.step'] = torch.tensor(mom['step'])
            for kind in ('exp_avg', 'exp_avg_sq'):
                for k, val in mom[kind].items():
                    snap[f'opt_{tag}.{kind}.{k}'] = val
        if L.gen_model.w_ewma is not None:
            snap['w_ewma'] = L.gen_model.w_ewma.clone()
        return snap

    def flags(L):
        from gan_lab_amd import rng
        nets = [L.gen_model, L.disc_model] + ([L.gen_model_lagged] if L.gen_model_lagged is not None else [])
        return ([p.requires_grad for net in nets for p in net.parameters()], [m.training for net in nets for m in net.modules()],
                [(net._use_noise, net._use_mixing_reg) for net in nets if hasattr(net, '_use_noise')],
                L.gen_model_lagged is None, dict(rng._STATE))

    def steps(L, real, zd, zg):
        L.set_requires_grad_disc(True)
        ld = L.d_step(real, zb=zd)
        L.set_requires_grad_disc(False)
        return ld, L.g_step(zb=zg)

    g = torch.Generator().manual_seed(13)
    real = (torch.rand(4, 3, 16, 16, generator=g) * 2 - 1).cuda()
    zs = [torch.randn(4, 16, generator=g).cuda() for _ in range(4)]
    target = torch.rand(2, 3, 16, 16, generator=g).cuda()

    def life(with_projection):
        """A learner's first two iterations, with projections between them or not.  Building it re-seeds the process's Philox
        stream, so the twins draw the same per-layer noise as long as nothing else moved the stream."""
        L = make_learner(seed=3)
        L.gen_model.pct_mixing_reg = 0                        # the mixing draw is host randomness: keep it out of the comparison
        L.gen_model.train()
        L.disc_model.train()
        L.beta = 0.9
        steps(L, real, zs[0], zs[1])                          # moments, EWMA and w_ewma hold something to disturb
        if with_projection:
            before, before_flags = snapshot(L), flags(L)
            for kw in (dict(space='w', noise_mode='const', time_average=True),
                       dict(space='w+', noise_mode='none', time_average=False)):
                L.project(target, steps=3, w_avg_samples=32, seed=5, **kw)
                after = snapshot(L)
                assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before), kw
                assert flags(L) == before_flags, kw
        return steps(L, real, zs[2], zs[3]), L

    (la, A), (lb, B) = life(True), life(False)
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
    assert torch.equal(A.arena_g.flat, B.arena_g.flat) and torch.equal(A.arena_d.flat, B.arena_d.flat)
    assert torch.equal(A.ewma.flat, B.ewma.flat)
    assert la[0].item() == la[0].item() and A.arena_g.flat.abs().max() > 0
