"""GPU tests of DiffAugment (csrc/augment.hip, ops.diff_augment, rng.augment_params, the learners' augmented steps).

The transform is restated below step by step with torch ops on the CPU, exactly as DESIGN.md "DiffAugment" (and the
official DiffAugment code) defines it: brightness, saturation, contrast, translation with zero fill, cutout."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import rel_err

pytestmark = pytest.mark.gpu

PARTS = ('color', 'translation', 'cutout')
POLICIES = [','.join(PARTS[i] for i in c) for k in range(1, 4) for c in itertools.combinations(range(3), k)]
FULL = 'color,translation,cutout'


def _mask(policy):
    from gan_lab_amd import augment
    return augment.parse_policy(policy)


def sizes(h, w):
    return int(h * 0.125 + 0.5), int(w * 0.125 + 0.5), int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)


def ref_augment(x, p, policy):
    """The CPU restatement.  x: (N, 3, H, W) CPU tensor of any float dtype (differentiable), p: (N, 8) rows."""
    n, _, h, w = x.shape
    dt = x.dtype
    parts = policy.split(',')
    sh, sw, ch, cw = sizes(h, w)
    if 'color' in parts:
        b, s, c = (p[:, k].to(dt).view(n, 1, 1, 1) for k in range(3))
        x = x + b                                                    # brightness
        m = x.mean(dim=1, keepdim=True)
        x = (x - m) * s + m                                          # saturation
        m = x.mean(dim=[1, 2, 3], keepdim=True)
        x = (x - m) * c + m                                          # contrast
    if 'translation' in parts:
        pad = F.pad(x, (w, w, h, h))                                 # y[i, j] = x[i + tx, j + ty], zero outside
        x = torch.stack([pad[k, :, h + int(p[k, 3]):2 * h + int(p[k, 3]), w + int(p[k, 4]):2 * w + int(p[k, 4])]
                         for k in range(n)])
    if 'cutout' in parts:
        keep = torch.ones(n, 1, h, w, dtype=torch.bool)
        for k in range(n):
            r0, c0 = int(p[k, 5]) - ch // 2, int(p[k, 6]) - cw // 2
            keep[k, :, max(r0, 0):max(min(r0 + ch, h), 0), max(c0, 0):max(min(c0 + cw, w), 0)] = False
        x = torch.where(keep, x, torch.zeros((), dtype=dt))
    return x


def host_params(n, h, w, gen, edges=True):
    """Random rows in range; with ``edges`` rows 1 and 2 sit on the extremes (tx = +-sh, cut touching two corners)."""
    sh, sw, ch, cw = sizes(h, w)
    p = torch.zeros(n, 8)
    p[:, 0] = torch.rand(n, generator=gen) - 0.5
    p[:, 1] = torch.rand(n, generator=gen) * 2
    p[:, 2] = torch.rand(n, generator=gen) + 0.5
    p[:, 3] = torch.randint(-sh, sh + 1, (n,), generator=gen).float()
    p[:, 4] = torch.randint(-sw, sw + 1, (n,), generator=gen).float()
    p[:, 5] = torch.randint(0, h + 1 - ch % 2, (n,), generator=gen).float()
    p[:, 6] = torch.randint(0, w + 1 - cw % 2, (n,), generator=gen).float()
    if edges and n >= 3:
        p[1, 3:7] = torch.tensor([sh, -sw, 0, 0], dtype=torch.float32)
        p[2, 3:7] = torch.tensor([-sh, sw, h - ch % 2, w - cw % 2], dtype=torch.float32)
    return p


def _judge(gpu, cpu32, ref64, what):
    """Color policies: the HIP result is within 2x the fp32 restatement's own error of float64, or within 1e-6 relative."""
    scale = max(ref64.abs().max().item(), 1e-30)
    e_gpu = (gpu.double() - ref64).abs().max().item()
    e_cpu = (cpu32.double() - ref64).abs().max().item()
    assert e_gpu <= max(2 * e_cpu, 1e-6 * scale), f'{what}: |hip - f64| {e_gpu:.3e}, |cpu32 - f64| {e_cpu:.3e}, scale {scale:.2e}'


CASES = [(4, 4), (8, 3), (16, 4), (64, 2), (256, 3), (1024, 2)]


@pytest.mark.parametrize('h,n', CASES, ids=[f'{h}-b{n}' for h, n in CASES])
def test_forward_and_backward_match_the_restatement(h, n):
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(h * 7 + n)
    x = torch.rand(n, 3, h, h, generator=gen) * 2 - 1
    g = torch.randn(n, 3, h, h, generator=gen)
    p = host_params(n, h, h, gen)
    for policy in POLICIES:
        mask = _mask(policy)
        xg = x.cuda().requires_grad_(True)
        y = ops.diff_augment(xg, p.cuda(), mask)
        (gx,) = torch.autograd.grad(y, xg, g.cuda())
        y, gx = y.detach().cpu(), gx.cpu()
        x32 = x.clone().requires_grad_(True)
        y32 = ref_augment(x32, p, policy)
        (gx32,) = torch.autograd.grad(y32, x32, g)
        if 'color' not in policy:      # pure data movement: bit for bit
            assert torch.equal(y, y32.detach()), f'{policy} forward'
            assert torch.equal(gx, gx32), f'{policy} backward'
            continue
        x64 = x.double().requires_grad_(True)
        y64 = ref_augment(x64, p.double(), policy)
        (gx64,) = torch.autograd.grad(y64, x64, g.double())
        _judge(y, y32.detach(), y64.detach(), f'{policy} forward {h}')
        _judge(gx, gx32, gx64, f'{policy} backward {h}')


@pytest.mark.parametrize('policy', [FULL, 'translation,cutout'])
def test_forward_full_batch_1024(policy):
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(3)
    n, h = 32, 1024
    x = torch.rand(n, 3, h, h, generator=gen) * 2 - 1
    p = host_params(n, h, h, gen)
    y = ops.diff_augment(x.cuda(), p.cuda(), _mask(policy)).cpu()
    with torch.no_grad():
        y32 = ref_augment(x, p, policy)
        if 'color' not in policy:
            assert torch.equal(y, y32)
            return
        for lo in range(0, n, 8):       # float64 in slices (memory)
            sl = slice(lo, lo + 8)
            _judge(y[sl], y32[sl], ref_augment(x[sl].double(), p[sl].double(), policy), f'{policy} b32 [{lo}:]')


@pytest.mark.parametrize('policy', [FULL, 'color', 'translation,cutout'])
def test_backward_is_the_adjoint_at_full_size(policy):
    """<A x, g> = <x, A^T g> for the linear part A x = aug(x) - aug(0), at 32 x 3 x 1024^2 with float64 dot products."""
    from gan_lab_amd import ops
    torch.manual_seed(11)
    n, h = 32, 1024
    gen = torch.Generator().manual_seed(12)
    p = host_params(n, h, h, gen).cuda()
    mask = _mask(policy)
    x = torch.rand(n, 3, h, h, device='cuda') * 2 - 1
    g = torch.randn(n, 3, h, h, device='cuda')
    ax = ops.k_diffaug(x, p, mask) - ops.k_diffaug(torch.zeros_like(x), p, mask)
    atg = ops.k_diffaug(g, p, mask, adjoint=True)
    lhs = (ax.double() * g.double()).sum().item()
    rhs = (x.double() * atg.double()).sum().item()
    bound = (ax.double().norm() * g.double().norm()).item()
    assert bound > 0 and abs(lhs - rhs) <= 1e-6 * bound, (lhs, rhs, bound)


def test_two_calls_are_bitwise_equal():
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(5)
    n, h = 8, 256
    x = (torch.rand(n, 3, h, h, generator=gen) * 2 - 1).cuda()
    g = torch.randn(n, 3, h, h, generator=gen).cuda()
    p = host_params(n, h, h, gen).cuda()
    for policy in (FULL, 'color'):
        m = _mask(policy)
        assert torch.equal(ops.k_diffaug(x, p, m), ops.k_diffaug(x, p, m))
        assert torch.equal(ops.k_diffaug(g, p, m, adjoint=True), ops.k_diffaug(g, p, m, adjoint=True))
    # a sample's result does not depend on the batch around it (the paired critic pass augments [fake; real] at once)
    m = _mask(FULL)
    whole = ops.k_diffaug(x, p, m)
    assert torch.equal(whole[:3], ops.k_diffaug(x[:3].contiguous(), p[:3].contiguous(), m))
    assert torch.equal(whole[3:], ops.k_diffaug(x[3:].contiguous(), p[3:].contiguous(), m))


def test_errors_and_double_backward():
    from gan_lab_amd import ops
    p = torch.zeros(2, 8, device='cuda')
    with pytest.raises(TypeError):
        ops.diff_augment(torch.zeros(2, 3, 8, 8), p, 1)
    with pytest.raises(TypeError):
        ops.diff_augment(torch.zeros(2, 3, 8, 8, device='cuda', dtype=torch.float64), p, 1)
    with pytest.raises(ValueError):
        ops.diff_augment(torch.zeros(2, 4, 8, 8, device='cuda'), p, 1)
    x = torch.rand(2, 3, 8, 8, device='cuda', requires_grad=True)
    y = ops.diff_augment(x, host_params(2, 8, 8, torch.Generator().manual_seed(0)).cuda(), _mask(FULL))
    (gx,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match='diff_augment'):
        gx.sum().backward()


@pytest.mark.parametrize('h', [4, 16, 64, 1024])
def test_parameter_draws(h):
    from gan_lab_amd import ops, rng
    n = 200000
    rng.manual_seed(123)
    off0 = rng._STATE['offset']
    p = rng.augment_params(n, h, h).cpu().double()
    assert rng._STATE['offset'] == off0 + 2 * n
    sh, sw, ch, cw = sizes(h, h)
    b, s, c = p[:, 0], p[:, 1], p[:, 2]
    assert b.min() >= -0.5 and b.max() < 0.5 and s.min() >= 0 and s.max() < 2 and c.min() >= 0.5 and c.max() < 1.5
    assert (p[:, 7] == 0).all()
    for col, lo, hi in ((3, -sh, sh), (4, -sw, sw), (5, 0, h - ch % 2), (6, 0, h - cw % 2)):
        v = p[:, col]
        assert (v == v.round()).all()
        assert set(v.long().unique().tolist()) == set(range(lo, hi + 1)), col
        k = hi - lo + 1                      # discrete uniform: mean, variance
        mean, var = (lo + hi) / 2, (k * k - 1) / 12
        assert abs(v.mean().item() - mean) < 5 * np.sqrt(max(var, 1e-12) / n) + 1e-12, col
        if k > 1:
            assert abs(v.var().item() / var - 1) < 0.05, col
    for v, mean, width in ((b, 0.0, 1.0), (s, 1.0, 2.0), (c, 1.0, 1.0)):
        var = width * width / 12
        assert abs(v.mean().item() - mean) < 5 * np.sqrt(var / n)
        assert abs(v.var().item() / var - 1) < 0.05
    # the device-base form equals the by-value form at the same stream position
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    ops.set_step_scalars(block, 1000, [])
    a = ops.diffaug_params(64, h, h, rng._STATE['seed'], 1000 + 37, 'cuda')
    d = ops.diffaug_params_dev(64, h, h, rng._STATE['seed'], block, 37, 'cuda')
    assert torch.equal(a, d)
    # and successive draws continue the stream: two draws of n = one draw of 2n
    rng.manual_seed(5)
    first = torch.cat([rng.augment_params(10, h, h), rng.augment_params(6, h, h)])
    rng.manual_seed(5)
    assert torch.equal(first, rng.augment_params(16, h, h))


def _philox4x32_10(ctr, seed):
    """Philox4x32-10 (Salmon et al. 2011) on counter (ctr, 0) with key ``seed``, as csrc/common.h runs it."""
    m = 0xFFFFFFFF
    c = [ctr & m, (ctr >> 32) & m, 0, 0]
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & m, p1 & m, ((p0 >> 32) ^ c[3] ^ k1) & m, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c


def _restated_row(words, h, w):
    """The parameter row of one sample from its 8 Philox words (DESIGN.md "DiffAugment"): u = (w >> 8) 2^-24."""
    sh, sw, ch, cw = sizes(h, w)
    u = [wd >> 8 for wd in words]
    two24 = np.float32(2.0 ** -24)
    c24 = u[2] + (1 << 23)                          # 0.5 + u, rounded down to fp32
    if c24 >= 1 << 24:
        c24 &= ~1

    def pick(k, lo, count):
        return float(lo + ((u[k] * count) >> 24))
    return [np.float32(u[0]) * two24 - np.float32(0.5), np.float32(u[1]) * two24 * np.float32(2), np.float32(c24) * two24,
            pick(3, -sh, 2 * sh + 1), pick(4, -sw, 2 * sw + 1), pick(5, 0, h + 1 - ch % 2), pick(6, 0, w + 1 - cw % 2), 0.0]


@pytest.mark.parametrize('h,w', [(64, 18), (4, 1024)])
def test_parameter_rows_restated_from_philox(h, w):
    """The normative mapping: sample n takes the words of counters offset + 2n (columns b, s, c, tx) and offset + 2n + 1
    (ty, ox, oy; the last word unused), u = (w >> 8) 2^-24, integers lo + floor(u (hi - lo + 1)).  The offset crosses a
    32-bit boundary of the counter; the key uses both halves of the seed."""
    from gan_lab_amd import ops
    seed, offset, n = 0x0123456789ABCDEF, 2 ** 32 - 3, 6
    got = ops.diffaug_params(n, h, w, seed, offset, 'cuda').cpu()
    want = torch.tensor([_restated_row(_philox4x32_10(offset + 2 * k, seed) + _philox4x32_10(offset + 2 * k + 1, seed), h, w)
                         for k in range(n)], dtype=torch.float32)
    assert torch.equal(got, want), (got, want)


# ------------------------------------------------------------------------------------------------------------------- #
# learners
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture
def small_widths():
    from gan_lab_amd import progressive as P
    P.FMAP_BASE, P.FMAP_MAX = 64, 16
    yield
    P.FMAP_BASE, P.FMAP_MAX = 8192, 512


def make_learner(kind, res, batch=4, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    common = dict(dev='cuda', pin_memory=False, res_samples=res, res_dataset=res, init_res=kw.pop('init_res', res),
                  batch_size=batch, len_latent=16, nimg_transition=24, num_iters_save_model=10 ** 9, log_every=0)
    common.update(kw)
    if kind == 'stylegan':
        return StyleGANLearner(make_config('stylegan', len_dlatent=16, mapping_num_fcs=2,
                                           cutoff_trunc_trick=None if res < 64 else 4, **common))
    return ProGANLearner(make_config('progan', **common))


def _perturb(named):
    with torch.no_grad():
        for k, p in named:
            if k.endswith('bias') or k.endswith('noise_weight'):
                p.normal_(0, 0.3)
            elif k == 'const_input':
                p.normal_(1.0, 0.5)


def _grad_errors(got, ref, floor=1e-3):
    """Per parameter: max |hip - f64| / max(|f64|, floor * largest gradient of the network)."""
    gmax = max(v.grad.abs().max().item() for v in ref.values() if v.grad is not None)
    out = {}
    for k, v in ref.items():
        if v.grad is None or k not in got:
            continue
        den = max(v.grad.abs().max().item(), floor * gmax, 1e-30)
        out[k] = (got[k].double() - v.grad).abs().max().item() / den
    return out


def _leaves(sd):
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}


@pytest.mark.parametrize('kind,loss,gp', [('stylegan', 'nonsaturating', 'r1'), ('progan', 'wgan', 'wgan-gp')])
def test_progressive_learner_step_matches_the_oracle(kind, loss, gp, small_widths):
    """d_step + g_step with diffaugment='color,translation,cutout' and fixed params against oracle.nets on the CPU (float64)
    fed the restated augmentation: StyleGAN R1 (the shared D(real) forward builds xr from the augmented batch) and ProGAN
    WGAN-GP (paired critic pass: one augment launch over [fake; real]; the penalty interpolates the augmented batches)."""
    from gan_lab_amd.stylegan.architectures import StyleAddNoise
    from oracle import nets, ops as O, step
    torch.manual_seed(3)
    b, res = 4, 16
    L = make_learner(kind, res, batch=b, loss=loss, gradient_penalty=gp, random_seed=3, diffaugment=FULL)
    _perturb(list(L.gen_model.named_parameters()) + list(L.disc_model.named_parameters()))
    L.gen_model.train()
    L.disc_model.train()
    L.beta = 0.99
    if kind == 'stylegan':
        L.gen_model.pct_mixing_reg = 0
        L.gen_model._use_mixing_reg = False
    else:
        assert L._pair_critic_batches(torch.empty(b, 3, res, res), torch.empty(b, 3, res, res))
    sd_g = {k: v.detach().cpu().clone() for k, v in L.gen_model.state_dict().items()}
    sd_d = {k: v.detach().cpu().clone() for k, v in L.disc_model.state_dict().items()}
    gen = torch.Generator().manual_seed(8)
    zd, zg = torch.randn(b, 16, generator=gen), torch.randn(b, 16, generator=gen)
    real = torch.rand(b, 3, res, res, generator=gen) * 2 - 1
    eps = torch.rand(b, 1, 1, 1, generator=gen)
    pd, pg = host_params(2 * b, res, res, gen), host_params(b, res, res, gen)
    kd = kg = {}
    nd = ng = None
    if kind == 'stylegan':
        shapes = [(b, 1, 4 * 2 ** (i // 2), 4 * 2 ** (i // 2)) for i in range(len(L.gen_model.gen_layers))]
        nd = [torch.randn(*s, generator=gen) for s in shapes]
        ng = [torch.randn(*s, generator=gen) for s in shapes]
        kd, kg = dict(noise=[v.cuda() for v in nd]), dict(noise=[v.cuda() for v in ng])
    StyleAddNoise.honour_noise_in_training = True
    try:
        L.set_requires_grad_disc(True)
        ld = L.d_step(real.cuda(), zb=zd.cuda(), gen_kwargs=kd, eps_interp=eps.cuda(), aug_params=pd.cuda())
        gd = {k: v.detach().cpu() for k, v in L.arena_d.views_of(L.arena_d.gflat).items()}
        sd_d1 = {k: v.detach().cpu().double() for k, v in L.disc_model.state_dict().items()}   # after the critic update
        L.set_requires_grad_disc(False)
        lg = L.g_step(zb=zg.cuda(), gen_kwargs=kg, aug_params=pg.cuda())
        gg = {k: v.detach().cpu() for k, v in L.arena_g.views_of(L.arena_g.gflat).items()}
    finally:
        StyleAddNoise.honour_noise_in_training = False

    cfg = nets.make_cfg(use_pixelnorm=(kind == 'progan'))
    fwd = (lambda sd, z, nz: nets.stylegen_forward(sd, z, [v.double() for v in nz], cfg)) if kind == 'stylegan' else \
        (lambda sd, z, nz: nets.progen_forward(sd, z, cfg))
    og, od = _leaves(sd_g), _leaves(sd_d)
    with torch.no_grad():
        fake = fwd(og, zd.double(), nd)
    pd64, pg64 = pd.double(), pg.double()
    total = step.d_loss(od, cfg, ref_augment(fake, pd64[:b], FULL), ref_augment(real.double(), pd64[b:], FULL), loss, gp,
                        10.0, 1.0, 0.001, eps_interp=eps.double())
    total.backward()
    img = fwd(og, zg.double(), ng)
    olg = O.loss_gen(loss, nets.disc_forward(sd_d1, ref_augment(img, pg64, FULL), cfg))
    olg.backward()
    assert rel_err(ld.cpu().double(), total.detach()) < 1e-3, (ld, total)
    assert rel_err(lg.cpu().double(), olg.detach()) < 1e-3, (lg, olg)
    for what, got, ref in (('d', gd, od), ('g', gg, og)):
        errs = _grad_errors(got, ref)
        assert len(errs) > 5
        worst = max(errs.items(), key=lambda kv: kv[1])
        assert worst[1] < 1e-3, f'{what} gradient {worst}'


def test_resnet_learner_step_matches_the_oracle():
    """ResNet GAN WGAN-GP (paired critic pass) d_step + g_step with DiffAugment against oracle.resnet (float64)."""
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    from oracle import resnet
    from util import resnet_zero_grad_key
    torch.manual_seed(4)
    b, res = 4, 32
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=res, res_dataset=res, batch_size=b,
                      num_iters_save_model=10 ** 9, log_every=0, len_latent=16, diffaugment=FULL, random_seed=4)
    cfg.fmap_g, cfg.fmap_d = 8, 8
    L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    sd_g = {k: v.detach().cpu().clone() for k, v in L.gen_model.state_dict().items()}
    sd_d = {k: v.detach().cpu().clone() for k, v in L.disc_model.state_dict().items()}
    gen = torch.Generator().manual_seed(9)
    zd, zg = torch.randn(b, 16, generator=gen), torch.randn(b, 16, generator=gen)
    real = torch.rand(b, 3, res, res, generator=gen) * 2 - 1
    eps = torch.rand(b, 1, 1, 1, generator=gen)
    pd, pg = host_params(2 * b, res, res, gen), host_params(b, res, res, gen)
    assert L._pair_critic_batches(torch.empty(b, 3, res, res), torch.empty(b, 3, res, res))
    L.set_requires_grad_disc(True)
    ld = L.d_step(real.cuda(), zb=zd.cuda(), eps_interp=eps.cuda(), aug_params=pd.cuda())
    gd = {k: v.grad.detach().cpu() for k, v in L.disc_model.named_parameters() if v.grad is not None}
    sd_d1 = {k: v.detach().cpu().double() for k, v in L.disc_model.state_dict().items()}
    L.set_requires_grad_disc(False)
    lg = L.g_step(zb=zg.cuda(), aug_params=pg.cuda())
    gg = {k: v.grad.detach().cpu() for k, v in L.gen_model.named_parameters() if v.grad is not None}

    dbl = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}  # noqa: E731
    gan = resnet.ResnetFunctionalGAN(dbl(sd_g), dbl(sd_d), res, loss='wgan', gp='wgan-gp')
    pd64, pg64 = pd.double(), pg.double()
    with torch.no_grad():
        fake = gan.gen(zd.double())
    total = gan.d_loss(ref_augment(fake, pd64[:b], FULL), ref_augment(real.double(), pd64[b:], FULL), eps.double())
    total.backward()
    out = gan.disc(ref_augment(gan.gen(zg.double()), pg64, FULL), sd_d1)
    olg = -out.mean()
    olg.backward()
    assert rel_err(ld.cpu().double(), total.detach()) < 1e-3, (ld, total)
    assert rel_err(lg.cpu().double(), olg.detach()) < 1e-3, (lg, olg)
    for what, got, ref in (('d', gd, gan.d), ('g', gg, gan.g)):
        errs = _grad_errors(got, {k: v for k, v in ref.items() if not resnet_zero_grad_key(k)}, floor=1e-4)
        assert len(errs) > 5
        worst = max(errs.items(), key=lambda kv: kv[1])
        assert worst[1] < 1e-3, f'{what} gradient {worst}'


def test_paired_critic_pass_equals_two_passes_with_augmentation(small_widths, monkeypatch):
    """With DiffAugment on, the paired ProGAN WGAN-GP critic pass (one augment launch over [fake; real] with the (2B, 8)
    block) sees the same augmented batches bit for bit as the two-pass path; loss and gradients agree as in
    tests/test_gpu_learner.py::test_progan_paired_critic_pass_equals_two_passes."""
    from gan_lab_amd import ops, rng
    from util import assert_close
    b, res = 4, 16
    seen, out = {}, {}
    orig = ops.diff_augment

    def spy(x, params, policy):
        y = orig(x, params, policy)
        seen.setdefault(pair, []).append(y.detach().clone())
        return y
    monkeypatch.setattr(ops, 'diff_augment', spy)
    gen = torch.Generator().manual_seed(9)
    real = (torch.rand(b, 3, res, res, generator=gen) * 2 - 1).cuda()
    zd = torch.randn(b, 16, generator=gen).cuda()
    eps = torch.rand(b, 1, 1, 1, generator=gen).cuda()
    for pair in ('0', '1'):
        monkeypatch.setenv('GANLAB_CRITIC_PAIR', pair)
        torch.manual_seed(5)
        rng.manual_seed(5)
        L = make_learner('progan', res, batch=b, loss='wgan', gradient_penalty='wgan-gp', random_seed=5, diffaugment=FULL)
        L.gen_model.train()
        L.disc_model.train()
        if pair == '0':
            w0 = L.arena_d.flat.detach().clone(), L.arena_g.flat.detach().clone()
        else:
            with torch.no_grad():
                L.arena_d.flat.copy_(w0[0])
                L.arena_g.flat.copy_(w0[1])
            ops.bump_weight_epoch()
        L.set_requires_grad_disc(True)
        off = rng._STATE['offset']
        ld = L.d_step(real, zb=zd, eps_interp=eps, defer_update=True)
        assert rng._STATE['offset'] == off + 2 * 2 * b          # one (2B, 8) draw
        out[pair] = (ld.cpu(), L.arena_d.gflat.detach().cpu().clone())
    assert [t.shape[0] for t in seen['0']] == [b, b] and [t.shape[0] for t in seen['1']] == [2 * b]
    assert torch.equal(torch.cat(seen['0']), seen['1'][0])
    assert out['0'][1].abs().max() > 0
    assert_close(out['1'][0], out['0'][0], 1e-6, 'loss_d')
    assert_close(out['1'][1], out['0'][1], 1e-5, 'critic gradients')


def test_train_with_augmentation_stays_finite_and_is_reproducible(small_widths):
    """train() with diffaugment on runs through a short growth schedule (8 -> 16) and stays finite; two runs from the same
    seeds agree bit for bit."""
    from gan_lab_amd import rng
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader

    def run():
        torch.manual_seed(7)
        np.random.seed(7)
        rng.manual_seed(1)
        L = make_learner('stylegan', 16, init_res=8, batch=4, loss='nonsaturating', gradient_penalty='r1', random_seed=7,
                         diffaugment=FULL)
        L.log_every = 1
        dl = SyntheticImageLoader(4096, 4, 8, seed=3)
        L.train(dl, num_main_iters=6 * 3 + 2)
        torch.cuda.synchronize()
        return L, {k: v.detach().clone() for k, v in list(L.gen_model.state_dict().items()) +
                   [('d.' + k, v) for k, v in L.disc_model.state_dict().items()]}
    L, a = run()
    assert L.gen_model.curr_res == 16 and not L.gen_model.fade_in_phase
    assert np.isfinite(L.last_losses['loss_d']) and np.isfinite(L.last_losses['loss_g'])
    assert all(torch.isfinite(v).all() for v in a.values() if v.is_floating_point())
    del L
    _, b2 = run()
    diff = [k for k in a if not torch.equal(a[k], b2[k])]
    assert not diff, diff[:4]


class _Census(object):
    """Kernel symbols launched through the library while active (see tests/test_gpu_fullsize.py's census)."""

    def __enter__(self):
        from gan_lab_amd import _lib
        self.L, self.saved, self.seen = _lib.lib(), {}, {}
        count = self.L.ganlab_launch_count
        for name in _lib.SIGNATURES:
            if name in ('ganlab_last_launch', 'ganlab_launch_count', 'ganlab_launch_history') or \
                    name.endswith(('_size', '_workspace', '_supported', '_plan', '_slots')):
                continue
            fn = getattr(self.L, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn):
                before = int(count())
                rc = _fn(*a)
                for sym, _ in _lib.launches_since(before):
                    self.seen[sym] = self.seen.get(sym, 0) + 1
                return rc
            setattr(self.L, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.L, name, fn)
        return False

    def symbols(self):
        return set(self.seen)


def test_kernel_census_with_and_without_augmentation(small_widths):
    """A G step with augmentation launches the kernels of the plain G step plus only the augment kernels (the fused G-side
    paths still engage); a D step launches no augment backward; with the option off nothing of augment.hip runs."""
    from gan_lab_amd import rng
    seen = {}
    for policy in (None, FULL):
        torch.manual_seed(2)
        L = make_learner('stylegan', 32, batch=4, loss='nonsaturating', gradient_penalty='r1', random_seed=2,
                         diffaugment=policy)
        L.gen_model.train()
        L.disc_model.train()
        L.beta = 0.99
        L.gen_model.pct_mixing_reg = 0
        L.gen_model._use_mixing_reg = False
        real = torch.rand(4, 3, 32, 32, device='cuda') * 2 - 1
        for _ in range(2):                     # the second iteration is the steady state (packed weights cached)
            L.set_requires_grad_disc(True)
            off = rng._STATE['offset']
            with _Census() as cd:
                L.d_step(real)
            d_draw = rng._STATE['offset'] - off
            L.set_requires_grad_disc(False)
            with _Census() as cg:
                L.g_step()
        torch.cuda.synchronize()
        seen[policy] = (cd.symbols(), cg.symbols(), d_draw)
    aug = lambda syms: {s for s in syms if 'diffaug' in s}  # noqa: E731
    d0, g0, draw0 = seen[None]
    d1, g1, draw1 = seen[FULL]
    assert not aug(d0) and not aug(g0)
    assert draw1 - draw0 == 2 * 8               # (2B, 8) rows: 2 counters each
    assert g0 <= g1 and aug(g1) == g1 - g0
    assert any('diffaug_apply_kernel<true>' in s for s in aug(g1)) and any('diffaug_apply_kernel<false>' in s for s in aug(g1))
    assert d0 <= d1 and not any('diffaug_apply_kernel<false>' in s or 'diffaug_sum_kernel<true>' in s for s in d1)
    assert any('diffaug_apply_kernel<true>' in s for s in d1)


@pytest.mark.parametrize('kind', ['stylegan', 'progan'])
def test_graphed_step_equals_eager_with_augmentation(kind):
    """graphs.GraphedStep with DiffAugment on: every replay draws fresh params through the device-resident stream position;
    parameters, Adam moments, EWMA generator and both losses equal the eager steps BIT FOR BIT after 6 iterations, 4 of
    them replayed (tests/test_gpu_learner.py::test_graphed_step_equals_eager, augmented)."""
    from gan_lab_amd import progressive as P, rng
    from gan_lab_amd.graphs import GraphedStep
    gen = torch.Generator().manual_seed(17)
    reals = [(torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(6)]

    def run(graphed):
        P.FMAP_BASE, P.FMAP_MAX = 1024, 64
        torch.manual_seed(9)
        np.random.seed(9)
        kw = dict(loss='nonsaturating', gradient_penalty='r1') if kind == 'stylegan' else \
            dict(loss='wgan', gradient_penalty='wgan-gp')
        L = make_learner(kind, 32, batch=4, random_seed=21, diffaugment=FULL, **kw)
        L.gen_model.train()
        L.disc_model.train()
        L.beta = 0.99
        torch.manual_seed(10)
        stepper = GraphedStep(L, warmup=2)
        losses = []
        for x in reals:
            if graphed:
                ld, lg = stepper(x)
            else:
                _, kw_d = stepper._mix_kwargs()
                ld = stepper._d_half(x, kw_d)
                _, kw_g = stepper._mix_kwargs()
                lg = stepper._g_half(kw_g)
            losses.append((float(ld), float(lg)))
        torch.cuda.synchronize()
        state = {'g': L.arena_g.flat.clone(), 'd': L.arena_d.flat.clone(), 'lag': L.ewma.flat.clone()}
        for name, opt in (('og', L.opt_gen), ('od', L.opt_disc)):
            ex = opt.export_moments(list(L.gen_model.named_parameters()) if name == 'og' else
                                    list(L.disc_model.named_parameters()))
            for k2, v in ex['exp_avg'].items():
                state[f'{name}.m.{k2}'] = v
            for k2, v in ex['exp_avg_sq'].items():
                state[f'{name}.v.{k2}'] = v
        return state, losses, (len(stepper.graphs) if graphed else 0), rng._STATE['offset']
    try:
        a, la, n_graphs, off_a = run(True)
        b, lb, _, off_b = run(False)
    finally:
        P.FMAP_BASE, P.FMAP_MAX = 8192, 512
    assert n_graphs >= 2, 'nothing was captured'
    assert off_a == off_b, 'the device random stream advanced differently'
    assert la == lb, (la, lb)
    diff = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not diff, f'{len(diff)} of {len(a)} tensors differ between replayed and eager steps, e.g. {diff[:4]}'
