"""GPU tests of ADA (csrc/ada.hip, ops.ada_augment, rng.ada_params, ada.AdaptiveAugment, the learners' augmented steps).

The transform is restated below with torch ops on the CPU exactly as DESIGN.md "ADA" defines it: an affine bilinear warp
with zero fill (output pixel -> source position through the 2x3 matrix M, centred pixel units), then the 3x4 color matrix C.
The composition of M and C from the elementary transforms (x-flip, quarter turns, integer shift, isotropic
scale, pre-rotation, anisotropic scale, post-rotation, fractional shift; brightness, contrast, luma flip, hue rotation,
saturation) is restated in float64 too, and so is the mapping from Philox words to the draws."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_diffaug import (_Census, _grad_errors, _judge, _leaves, _perturb, _philox4x32_10, make_learner,  # noqa: F401
                              small_widths)
from util import rel_err

pytestmark = pytest.mark.gpu

PARTS = ('blit', 'geom', 'color')
POLICIES = [','.join(PARTS[i] for i in c) for k in range(1, 4) for c in itertools.combinations(range(3), k)]
FULL = 'blit,geom,color'
GATES = ('flip', 'turn', 'shift', 'iso', 'pre', 'aniso', 'post', 'frac', 'bright', 'contrast', 'luma', 'hue', 'sat')


# ------------------------------------------------------------------------------------------------------------------- #
# the restatement
# ------------------------------------------------------------------------------------------------------------------- #
def ref_augment(x, rows, coords64=False):
    """The CPU restatement.  x: (N, 3, H, W) CPU tensor of any float dtype (differentiable); rows: (N, 32) fp32 rows, of which
    M (columns 0..5) and C (10..21) are used.  Everything is evaluated in x's dtype, except that ``coords64`` evaluates the
    source positions (not the interpolation) in float64."""
    n, _, h, w = x.shape
    dt = x.dtype
    cdt = torch.float64 if coords64 else dt
    M = rows[:, :6].to(cdt).view(n, 6, 1, 1)
    C = rows[:, 10:22].to(dt).view(n, 3, 4)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    u = (torch.arange(w, dtype=cdt) - cx).view(1, 1, w)
    v = (torch.arange(h, dtype=cdt) - cy).view(1, h, 1)
    sj = M[:, 0] * u + M[:, 1] * v + M[:, 2] + cx
    si = M[:, 3] * u + M[:, 4] * v + M[:, 5] + cy
    j0 = torch.floor(sj).clamp(-2, w + 1)
    i0 = torch.floor(si).clamp(-2, h + 1)
    fx, fy = (sj - j0).clamp(0, 1).to(dt), (si - i0).clamp(0, 1).to(dt)
    flat = x.reshape(n, 3, h * w)
    warped = torch.zeros_like(x)
    for a in (0, 1):
        for b in (0, 1):
            r, c = i0.long() + a, j0.long() + b
            inside = (r >= 0) & (r < h) & (c >= 0) & (c < w)
            idx = (r.clamp(0, h - 1) * w + c.clamp(0, w - 1)).view(n, 1, h * w).expand(n, 3, h * w)
            wgt = (fy if a else 1 - fy) * (fx if b else 1 - fx) * inside.to(dt)
            warped = warped + flat.gather(2, idx).view(n, 3, h, w) * wgt.unsqueeze(1)
    y = [sum(C[:, k, q].view(n, 1, 1) * warped[:, q] for q in range(3)) + C[:, k, 3].view(n, 1, 1) for k in range(3)]
    return torch.stack(y, dim=1)


def compose(h, w, flip=False, turn=None, shift=None, iso=None, pre=None, aniso=None, post=None, frac=None,
            bright=None, contrast=None, luma=False, hue=None, sat=None):
    """(M, G, C) in float64 from the raw draws of the transforms that fire (None / False: that one does not), in the order of
    DESIGN.md "ADA": M = X^-1 Q^-1 T^-1 S^-1 Rpre^-1 A^-1 Rpost^-1 F^-1 (each factor maps an output position to a source
    position), G = F Rpost A Rpre S T Q X (linear parts), C = Sat Hue Luma Contrast Bright."""
    M, G = np.eye(3), np.eye(2)

    def put(minv, lin):
        nonlocal M, G
        M = M @ np.array([[minv[0][0], minv[0][1], minv[0][2]], [minv[1][0], minv[1][1], minv[1][2]], [0, 0, 1.0]])
        G = np.array(lin, dtype=np.float64) @ G

    def rot(c, s):
        put([[c, -s, 0], [s, c, 0]], [[c, s], [-s, c]])
    if flip:
        put([[-1, 0, 0], [0, 1, 0]], [[-1, 0], [0, 1]])
    if turn is not None:
        rot(*[(1, 0), (0, 1), (-1, 0), (0, -1)][int(turn)])
    if shift is not None:
        put([[1, 0, float(shift[0])], [0, 1, float(shift[1])]], [[1, 0], [0, 1]])
    if iso is not None:
        s = 2.0 ** (0.2 * float(iso))
        put([[1 / s, 0, 0], [0, 1 / s, 0]], [[s, 0], [0, s]])
    if pre is not None:
        rot(math.cos(float(pre)), math.sin(float(pre)))
    if aniso is not None:
        s = 2.0 ** (0.2 * float(aniso))
        put([[1 / s, 0, 0], [0, s, 0]], [[s, 0], [0, 1 / s]])
    if post is not None:
        rot(math.cos(float(post)), math.sin(float(post)))
    if frac is not None:
        put([[1, 0, 0.125 * w * float(frac[0])], [0, 1, 0.125 * h * float(frac[1])]], [[1, 0], [0, 1]])
    C = np.eye(3, 4)
    vv = np.full((3, 3), 1.0 / 3.0)
    if bright is not None:
        C[:, 3] += 0.2 * float(bright)
    if contrast is not None:
        C = C * 2.0 ** (0.5 * float(contrast))
    if luma:
        C = (np.eye(3) - 2 * vv) @ C
    if hue is not None:
        cs, sn = math.cos(float(hue)), math.sin(float(hue)) / math.sqrt(3.0)
        cross = np.array([[0, -1, 1], [1, 0, -1], [-1, 1, 0.0]])
        C = (cs * np.eye(3) + sn * cross + (1 - cs) * vv) @ C
    if sat is not None:
        s = 2.0 ** float(sat)
        C = (vv + s * (np.eye(3) - vv)) @ C
    return M[:2], G, C


def make_rows(specs, h, w):
    from gan_lab_amd import ada
    mc = [compose(h, w, **s) for s in specs]
    return ada.rows_from_matrices(np.stack([m for m, _, _ in mc]), np.stack([c for _, _, c in mc]))


def policy_rows(policy, n, h, w, seed):
    """``n`` fixed hand-made rows for a policy.  Row 0 sits on the clamp extremes that make the adjoint's footprint largest
    (largest zoom-in along x, 2^0.6 2^0.6, under 45 degree rotations; largest integer shift), row 1 on the opposite ones
    (largest zoom-out, largest fractional shift); the others are drawn from a seeded generator inside the ranges."""
    gen = np.random.default_rng(seed)
    sh, sw = (h + 4) // 8, (w + 4) // 8
    parts = policy.split(',')
    specs = []
    for k in range(n):
        s = {}
        if 'blit' in parts:
            if k == 0:
                s.update(flip=True, turn=1, shift=(sw, -sh))
            elif k == 1:
                s.update(turn=3, shift=(-sw, sh))
            else:
                s.update(flip=bool(gen.integers(2)), turn=int(gen.integers(4)),
                         shift=(int(gen.integers(-sw, sw + 1)), int(gen.integers(-sh, sh + 1))))
        if 'geom' in parts:
            if k == 0:
                s.update(iso=3.0, pre=math.pi / 4, aniso=3.0, post=-math.pi / 4, frac=(0.3, -0.2))
            elif k == 1:
                s.update(iso=-3.0, pre=-math.pi / 4, aniso=-3.0, frac=(3.0, -3.0))
            else:
                z = np.clip(gen.standard_normal(4), -3, 3)
                th = gen.uniform(-math.pi, math.pi, 2)
                s.update(iso=z[0], pre=th[0], aniso=z[1], post=th[1], frac=(z[2], z[3]))
        if 'color' in parts:
            if k == 0:
                s.update(bright=1.5, contrast=2.0, luma=True, hue=2.5, sat=1.5)
            else:
                z = gen.standard_normal(3)
                s.update(bright=z[0], contrast=z[1], luma=bool(gen.integers(2)), hue=gen.uniform(-math.pi, math.pi), sat=z[2])
        specs.append(s)
    return make_rows(specs, h, w)


def shift_image(x, ty, tx):
    """y[i, j] = x[i + ty, j + tx], zero outside."""
    h, w = x.shape[-2:]
    return F.pad(x, (w, w, h, h))[..., h + ty:2 * h + ty, w + tx:2 * w + tx]


# ------------------------------------------------------------------------------------------------------------------- #
# kernels
# ------------------------------------------------------------------------------------------------------------------- #
CASES = [(4, 4), (8, 3), (16, 4), (64, 3), (256, 3), (1024, 2)]


@pytest.mark.parametrize('h,n', CASES, ids=[f'{h}-b{n}' for h, n in CASES])
def test_forward_and_adjoint_match_the_restatement(h, n):
    """Every policy subset, fixed hand-made rows including the clamp extremes.  The bar is tests/test_gpu_diffaug.py's _judge:
    |hip - f64| <= max(2 |cpu32 - f64|, 1e-6 scale).  The fp32 restatement's own error is dominated by the rounding of its
    source positions (positions up to ~10^3 pixels carry ~10^-4 pixel of fp32 rounding, times the image's gradient), which
    the kernel does not share - it evaluates positions in fp64 - so the fp32 restatement judged against here evaluates only
    its positions in float64 (``coords64``): the stricter yardstick.  The 2x margin is kept."""
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(h * 7 + n)
    x = torch.rand(n, 3, h, h, generator=gen) * 2 - 1
    g = torch.randn(n, 3, h, h, generator=gen)
    for policy in POLICIES:
        rows = policy_rows(policy, n, h, h, seed=h + len(policy))
        xg = x.cuda().requires_grad_(True)
        y = ops.ada_augment(xg, rows.cuda())
        (gx,) = torch.autograd.grad(y, xg, g.cuda())
        y, gx = y.detach().cpu(), gx.cpu()
        x32 = x.clone().requires_grad_(True)
        y32 = ref_augment(x32, rows, coords64=True)
        (gx32,) = torch.autograd.grad(y32, x32, g)
        x64 = x.double().requires_grad_(True)
        y64 = ref_augment(x64, rows)
        (gx64,) = torch.autograd.grad(y64, x64, g.double())
        e = [(t.double() - r).abs().max().item() for t, r in ((y, y64.detach()), (y32.detach(), y64.detach()), (gx, gx64),
                                                               (gx32, gx64))]
        print(f'ada {policy} {h}: fwd |hip-f64| {e[0]:.3e} |cpu32-f64| {e[1]:.3e}  adj |hip-f64| {e[2]:.3e} |cpu32-f64| {e[3]:.3e}')
        _judge(y, y32.detach(), y64.detach(), f'{policy} forward {h}')
        _judge(gx, gx32, gx64, f'{policy} adjoint {h}')


@pytest.mark.parametrize('h,w', [(16, 16), (1024, 1024), (16, 8)])
def test_blit_rows_are_exact_copies(h, w):
    """Flips, quarter turns and integer shifts (also composed, also at the largest shift) reproduce torch.flip, torch.rot90 and
    a zero-filled slice shift bit for bit, forward and adjoint."""
    from gan_lab_amd import ops
    sh, sw = (h + 4) // 8, (w + 4) // 8
    gen = torch.Generator().manual_seed(h + w)
    square = h == w
    specs = [dict(flip=True), dict(turn=2), dict(shift=(sw, -sh)), dict(shift=(-3, 1)), dict(flip=True, turn=2, shift=(-sw, sh))]
    if square:
        specs += [dict(turn=1), dict(turn=3), dict(flip=True, turn=1, shift=(2, -1))]
    n = len(specs)
    x = (torch.rand(n, 3, h, w, generator=gen) * 2 - 1).cuda()
    g = torch.randn(n, 3, h, w, generator=gen).cuda()
    rows = make_rows(specs, h, w).cuda()
    y = ops.k_ada(x, rows)
    gx = ops.k_ada(g, rows, adjoint=True)
    for k, s in enumerate(specs):
        want = x[k]
        if s.get('flip'):
            want = torch.flip(want, [2])
        if s.get('turn') is not None:
            want = torch.rot90(want, s['turn'], [1, 2])
        if s.get('shift') is not None:
            want = shift_image(want, s['shift'][1], s['shift'][0])
        assert torch.equal(y[k], want), f'forward {s}'
        back = g[k]                                     # the adjoint undoes the steps in reverse order
        if s.get('shift') is not None:
            back = shift_image(back, -s['shift'][1], -s['shift'][0])
        if s.get('turn') is not None:
            back = torch.rot90(back, -s['turn'], [1, 2])
        if s.get('flip'):
            back = torch.flip(back, [2])
        assert torch.equal(gx[k], back), f'adjoint {s}'


def _drawn_rows(n, h, w, policy, p, seed=1):
    from gan_lab_amd import ada, rng
    rng.manual_seed(seed)
    state = torch.tensor([p, 0, 0, 0], dtype=torch.float32, device='cuda')
    return rng.ada_params(n, h, w, state, ada.parse_policy(policy))


@pytest.mark.parametrize('policy', [FULL, 'geom'])
def test_adjoint_at_full_size(policy):
    """<A x, g> = <x, A^T g> for the linear part A x = ada(x) - ada(0), at 32 x 3 x 1024^2 with float64 dot products and rows
    drawn at p = 1 (the bound of tests/test_gpu_diffaug.py::test_backward_is_the_adjoint_at_full_size)."""
    from gan_lab_amd import ops
    torch.manual_seed(11)
    n, h = 32, 1024
    rows = _drawn_rows(n, h, h, policy, 1.0)
    x = torch.rand(n, 3, h, h, device='cuda') * 2 - 1
    g = torch.randn(n, 3, h, h, device='cuda')
    ax = ops.k_ada(x, rows) - ops.k_ada(torch.zeros_like(x), rows)
    atg = ops.k_ada(g, rows, adjoint=True)
    lhs = (ax.double() * g.double()).sum().item()
    rhs = (x.double() * atg.double()).sum().item()
    bound = (ax.double().norm() * g.double().norm()).item()
    print(f'ada adjointness {policy}: lhs {lhs:.9e} rhs {rhs:.9e} |lhs - rhs| / bound {abs(lhs - rhs) / bound:.3e}')
    assert bound > 0 and abs(lhs - rhs) <= 1e-6 * bound, (lhs, rhs, bound)


@pytest.mark.parametrize('h', [64, 256])
def test_no_contribution_is_dropped(h):
    """x = 1, C = identity: sum(A^T 1) per sample equals sum(A 1) per sample - the total bilinear weight that lands inside the
    image - summed in float64.  Rows: the clamp extremes (largest footprints a draw can have), a 4x and an 8x zoom-in, which
    lie beyond the clamps (footprints of 9 x 9 and 17 x 17 candidates), and a rotated 4x zoom.  The adjoint of the zoom rows is
    also held to the restatement's autograd element by element.
    Bound: every output of either side is a sum of at most 17^2 = 289 non-negative fp32 products, so its relative rounding
    error stays below 400 * 2^-24; the forward's outputs are at most 1 each (four weights that sum to 1), so either side's
    total is at most 3 H W and the two may differ by 2 * 400 * 2^-24 * 3 H W.  A dropped candidate row or column would take
    a fixed fraction of the total weight with it: thousands of times that."""
    from gan_lab_amd import ada, ops
    specs = [dict(iso=3.0, pre=math.pi / 4, aniso=3.0, post=-math.pi / 4), dict(iso=3.0, pre=math.pi / 4, aniso=-3.0),
             dict(iso=-3.0, aniso=-3.0, frac=(3.0, 3.0)), dict(iso=3.0, aniso=3.0, pre=0.3, frac=(-3.0, 3.0))]
    rows = make_rows(specs, h, h)
    c, s = math.cos(0.7), math.sin(0.7)
    zoom = ada.rows_from_matrices(torch.tensor([[[0.25, 0, 0.4], [0, 0.25, -1.3]], [[0.125, 0, 0], [0, 0.125, 0]],
                                                [[0.25 * c, -0.25 * s, 2.0], [0.25 * s, 0.25 * c, 0.5]]]))
    rows = torch.cat([rows, zoom])
    n = rows.shape[0]
    ones = torch.ones(n, 3, h, h, device='cuda')
    fwd = ops.k_ada(ones, rows.cuda()).double().sum(dim=(1, 2, 3)).cpu()
    adj = ops.k_ada(ones, rows.cuda(), adjoint=True).double().sum(dim=(1, 2, 3)).cpu()
    bound = 2 * 400 * 2.0 ** -24 * 3 * h * h
    print(f'ada weight sums {h}: forward {fwd.tolist()} adjoint {adj.tolist()} bound {bound:.3e}')
    assert (fwd > 0).all()
    assert ((fwd - adj).abs() <= bound).all(), (fwd, adj, bound)
    g = torch.randn(3, 3, h, h, generator=torch.Generator().manual_seed(h))
    x64 = torch.zeros(3, 3, h, h, dtype=torch.float64, requires_grad=True)
    (gx64,) = torch.autograd.grad(ref_augment(x64, zoom), x64, g.double())
    x32 = torch.zeros(3, 3, h, h, requires_grad=True)
    (gx32,) = torch.autograd.grad(ref_augment(x32, zoom, coords64=True), x32, g)
    _judge(ops.k_ada(g.cuda(), zoom.cuda(), adjoint=True).cpu(), gx32, gx64, f'zoom adjoint {h}')


def test_two_calls_are_bitwise_equal():
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(5)
    n, h = 8, 256
    x = (torch.rand(n, 3, h, h, generator=gen) * 2 - 1).cuda()
    g = torch.randn(n, 3, h, h, generator=gen).cuda()
    p = policy_rows(FULL, n, h, h, seed=2).cuda()
    assert torch.equal(ops.k_ada(x, p), ops.k_ada(x, p))
    assert torch.equal(ops.k_ada(g, p, adjoint=True), ops.k_ada(g, p, adjoint=True))
    # a sample's result does not depend on the batch around it (the paired critic pass augments [fake; real] at once)
    for adjoint, t in ((False, x), (True, g)):
        whole = ops.k_ada(t, p, adjoint=adjoint)
        assert torch.equal(whole[:3], ops.k_ada(t[:3].contiguous(), p[:3].contiguous(), adjoint=adjoint))
        assert torch.equal(whole[3:], ops.k_ada(t[3:].contiguous(), p[3:].contiguous(), adjoint=adjoint))


def test_errors_and_double_backward():
    from gan_lab_amd import ops
    p = torch.zeros(2, 32, device='cuda')
    with pytest.raises(TypeError):
        ops.ada_augment(torch.zeros(2, 3, 8, 8), p)
    with pytest.raises(TypeError):
        ops.ada_augment(torch.zeros(2, 3, 8, 8, device='cuda', dtype=torch.float64), p)
    with pytest.raises(ValueError):
        ops.ada_augment(torch.zeros(2, 4, 8, 8, device='cuda'), p)
    with pytest.raises(ValueError):
        ops.ada_augment(torch.zeros(2, 3, 8, 8, device='cuda'), torch.zeros(2, 8, device='cuda'))
    with pytest.raises(ValueError):
        ops.ada_augment(torch.zeros(2, 3, 8, 6, device='cuda'), p)
    x = torch.rand(2, 3, 8, 8, device='cuda', requires_grad=True)
    y = ops.ada_augment(x, policy_rows(FULL, 2, 8, 8, seed=0).cuda())
    (gx,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match='ada_augment'):
        gx.sum().backward()


# ------------------------------------------------------------------------------------------------------------------- #
# parameter rows
# ------------------------------------------------------------------------------------------------------------------- #
def _restated_row(words, h, w, p, mask):
    """One sample's draws from its 32 Philox words (DESIGN.md "ADA", the normative mapping), then (M, G, C) composed from them
    in float64.  Returns (gate bits, the ten raw columns 22..31, M, G, C)."""
    f32 = np.float32
    two24 = 2.0 ** -24
    u = [(wd >> 8) * two24 for wd in words]
    p = float(f32(p))
    prot = 1.0 - math.sqrt(1.0 - min(max(p, 0.0), 1.0))
    group = dict(flip=1, turn=1, shift=1, iso=2, pre=2, aniso=2, post=2, frac=2, bright=4, contrast=4, luma=4, hue=4, sat=4)
    on = {name: bool(mask & group[name]) and u[k] < (prot if name in ('pre', 'post') else p) for k, name in enumerate(GATES)}

    def pick(k, lo, count):
        return lo + (((words[k] >> 8) * count) >> 24)

    def normal(k):
        r = math.sqrt(-2.0 * math.log(((words[k] >> 8) + 1) * two24))
        a = 2.0 * math.pi * u[k + 1]
        return r * math.cos(a), r * math.sin(a)

    def clamp3(z):
        return min(max(z, -3.0), 3.0)
    sh, sw = (h + 4) // 8, (w + 4) // 8
    turn, tx, ty = pick(13, 0, 4), pick(14, -sw, 2 * sw + 1), pick(15, -sh, 2 * sh + 1)
    z_iso, z_aniso = normal(16)
    z_fx, z_fy = normal(20)
    z_bright, _ = normal(22)
    z_contrast, z_sat = normal(24)
    r_iso, r_aniso, r_fx, r_fy = (f32(clamp3(z)) for z in (z_iso, z_aniso, z_fx, z_fy))
    r_bright, r_contrast, r_sat = f32(z_bright), f32(z_contrast), f32(z_sat)
    r_pre, r_post, r_hue = (f32((2.0 * u[k] - 1.0) * math.pi) for k in (18, 19, 26))
    bits = sum(1 << k for k, name in enumerate(GATES) if on[name])
    raw = [f32(bits), f32(turn), f32(tx), f32(ty), r_iso, r_pre, r_aniso, r_post, r_fx, r_fy]
    M, G, C = compose(h, w, flip=on['flip'], turn=turn if on['turn'] else None, shift=(tx, ty) if on['shift'] else None,
                      iso=r_iso if on['iso'] else None, pre=r_pre if on['pre'] else None,
                      aniso=r_aniso if on['aniso'] else None, post=r_post if on['post'] else None,
                      frac=(r_fx, r_fy) if on['frac'] else None, bright=r_bright if on['bright'] else None,
                      contrast=r_contrast if on['contrast'] else None, luma=on['luma'], hue=r_hue if on['hue'] else None,
                      sat=r_sat if on['sat'] else None)
    return bits, raw, M, G, C


@pytest.mark.parametrize('h,w,p,policy', [(64, 20, 0.5, FULL), (4, 1024, 0.9, FULL), (32, 32, 0.7, 'blit,color'),
                                          (16, 16, 1.0, 'geom')])
def test_parameter_rows_restated_from_philox(h, w, p, policy):
    """The normative mapping: sample n takes the 32 words of counters offset + 8n .. offset + 8n + 7.  Gates and raw draws
    (columns 22..31) are bit-equal to the host restatement; M, G and C are within fp32 rounding - 2 ulp of
    max(1, |entry|): one rounding of the entry itself and one of slack for the two libms' last double bit - of the float64
    composition from those raw values, and G M[:, :2] is the identity to 1e-6.  The color draws are not stored in the row
    (its ten spare columns hold the gates and the nine geometric draws): the restatement derives them from the words and C
    answers for them.  The offset crosses a 32-bit boundary of the counter; the key uses both halves of the seed."""
    from gan_lab_amd import ada, ops
    seed, offset, n = 0x0123456789ABCDEF, 2 ** 32 - 20, 24
    mask = ada.parse_policy(policy)
    state = torch.tensor([p, 7, 8, 1], dtype=torch.float32, device='cuda')
    got = ops.ada_params(n, h, w, state, mask, seed, offset, 'cuda').cpu()
    assert torch.equal(state.cpu(), torch.tensor([p, 7, 8, 1], dtype=torch.float32))         # the draw only reads the block
    fired = 0
    for k in range(n):
        words = sum((_philox4x32_10(offset + 8 * k + c, seed) for c in range(8)), [])
        bits, raw, M, G, C = _restated_row(words, h, w, p, mask)
        fired |= bits
        assert got[k, 22:].tolist() == [float(v) for v in raw], (k, got[k, 22:].tolist(), raw)
        want = torch.tensor(np.concatenate([M.reshape(-1), G.reshape(-1), C.reshape(-1)]))
        err = (got[k, :22].double() - want).abs()
        tol = 2.0 ** -22 * want.abs().clamp(min=1.0)
        assert (err <= tol).all(), (k, got[k, :22], want)
        gm = got[k, 6:10].double().view(2, 2) @ got[k, :6].double().view(2, 3)[:, :2]
        assert (gm - torch.eye(2, dtype=torch.float64)).abs().max() <= 1e-6, (k, gm)
    groups = {1: 0b111, 2: 0b11111000, 4: 0b1111100000000}
    allowed = sum(v for g, v in groups.items() if mask & g)
    assert fired & ~allowed == 0 and fired != 0


def test_gate_frequencies_and_the_ends():
    """Over N = 65535 rows every gate fires with its probability (p; the two rotations 1 - sqrt(1 - p)) within 5 standard
    deviations, never at p = 0 and always at p = 1.  Rows drawn at p = 0 are the identity and ada_augment returns its input
    bit for bit.  The stream advances by 8 counters per row, successive draws continue it, and the device-base form equals
    the by-value form."""
    from gan_lab_amd import ada, ops, rng
    n, h = 65535, 32
    mask = ada.parse_policy(FULL)
    for p in (0.0, 0.3, 1.0):
        rng.manual_seed(77)
        off0 = rng._STATE['offset']
        state = torch.tensor([p, 0, 0, 0], dtype=torch.float32, device='cuda')
        rows = rng.ada_params(n, h, h, state, mask).cpu()
        assert rng._STATE['offset'] == off0 + 8 * n
        bits = rows[:, 22].long()
        p32 = float(np.float32(p))
        for k, name in enumerate(GATES):
            q = 1.0 - math.sqrt(1.0 - p32) if name in ('pre', 'post') else p32
            freq = ((bits >> k) & 1).double().mean().item()
            assert abs(freq - q) <= 5 * math.sqrt(q * (1 - q) / n), (p, name, freq, q)
        if p == 0.0:
            ident = ada.rows_from_matrices(torch.tensor([[[1.0, 0, 0], [0, 1, 0]]]))[0, :22]
            assert torch.equal(rows[:, :22], ident.expand(n, 22)) and (bits == 0).all()
            x = (torch.rand(8, 3, h, h) * 2 - 1).cuda()
            assert torch.equal(ops.ada_augment(x, rows[:8].cuda()), x)
            assert torch.equal(ops.k_ada(x, rows[:8].cuda(), adjoint=True), x)
        if p == 1.0:
            assert (bits == (1 << 13) - 1).all()
            # the drawn geometry stays inside the clamps that bound the adjoint's footprint
            G = rows[:, 6:10].abs()
            assert max((G[:, 0] + G[:, 1]).max().item(), (G[:, 2] + G[:, 3]).max().item()) <= math.sqrt(2) * 2 ** 1.2 + 1e-4
            assert rows[:, 26].abs().max() <= 3 and rows[:, 28].abs().max() <= 3 and rows[:, 30:32].abs().max() <= 3
            assert rows[:, 27].abs().max() <= math.pi + 1e-6 and rows[:, 29].abs().max() <= math.pi + 1e-6
    # a policy closes the gates of the groups it leaves out, whatever p
    state = torch.ones(4, device='cuda')
    rows = ops.ada_params(64, h, h, state, ada.GEOM, 5, 0, 'cuda').cpu()
    assert (rows[:, 22].long() == 0b11111000).all() and torch.equal(rows[:, 10:22], torch.eye(3, 4).reshape(1, 12).expand(64, 12))
    # the device-base form equals the by-value form at the same stream position
    state = torch.tensor([0.5, 0, 0, 0], dtype=torch.float32, device='cuda')
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    ops.set_step_scalars(block, 1000, [])
    a = ops.ada_params(64, h, h, state, mask, rng._STATE['seed'], 1000 + 37, 'cuda')
    d = ops.ada_params_dev(64, h, h, state, mask, rng._STATE['seed'], block, 37, 'cuda')
    assert torch.equal(a, d)
    # successive draws continue the stream: two draws of n = one draw of 2n
    rng.manual_seed(5)
    first = torch.cat([rng.ada_params(10, h, h, state, mask), rng.ada_params(6, h, h, state, mask)])
    rng.manual_seed(5)
    assert torch.equal(first, rng.ada_params(16, h, h, state, mask))


# ------------------------------------------------------------------------------------------------------------------- #
# controller
# ------------------------------------------------------------------------------------------------------------------- #
def test_controller_follows_the_host_rule():
    """A scripted sequence of logit batches: p, read back after every call, equals ada.next_p applied on the host at every
    ``interval``-th call - exactly, both add the same fp32 step - and the accumulators are the running sums in between."""
    from gan_lab_amd import ada
    gen = torch.Generator().manual_seed(3)
    interval, kimg, b = 3, 0.5, 16
    aug = ada.AdaptiveAugment('blit', p=0.5, target=0.25, interval=interval, kimg=kimg)
    step = ada.step_size(b, 1, interval, kimg)
    assert 0 < step < 0.2
    p, acc_sum, acc_n, calls = 0.5, 0.0, 0.0, 0
    moved = set()
    for it in range(30):
        bias = (1.5, -1.5, 0.1)[(it // 6) % 3]
        logits = torch.randn(b, 1, generator=gen) + bias
        if it == 4:
            logits[:3] = 0.0                      # sign(0) = 0
        aug.update(logits.cuda())
        acc_sum += float(torch.sign(logits).sum())
        acc_n += b
        calls += 1
        if calls == interval:
            new = ada.next_p(p, acc_sum, acc_n, 0.25, step)
            moved.add(np.sign(new - p))
            p, acc_sum, acc_n, calls = new, 0.0, 0.0, 0
        assert aug.state.cpu().tolist() == [p, acc_sum, acc_n, float(calls)], (it, aug.state, p, acc_sum, acc_n, calls)
        assert aug.p == p
    assert moved >= {1.0, -1.0}


def test_controller_saturates_and_fixed_p_launches_nothing(small_widths):
    from gan_lab_amd import ada
    up = torch.ones(8, device='cuda')
    for p0, logits, end in ((0.9, up, 1.0), (0.1, -up, 0.0)):
        aug = ada.AdaptiveAugment('color', p=p0, target=0.0, interval=1, kimg=0.1)       # step 0.08
        seen = []
        for _ in range(5):
            aug.update(logits)
            seen.append(aug.p)
        assert seen[-1] == end and seen[-2] == end and 0.0 < seen[0] < 1.0, seen
        assert sorted(seen, reverse=(end == 0.0)) == seen
    # fixed p: update is a no-op, and a learner's D step launches no controller kernel
    aug = ada.AdaptiveAugment('color', p=0.3, target=None)
    aug.update(up)
    assert aug.state.cpu().tolist() == [float(np.float32(0.3)), 0.0, 0.0, 0.0]
    seen = {}
    for target in (None, 0.6):
        torch.manual_seed(2)
        L = make_learner('progan', 16, batch=4, loss='wgan', gradient_penalty='wgan-gp', random_seed=2, ada=FULL,
                         ada_p=0.3, ada_target=target, ada_interval=1, ada_kimg=0.1)
        L.gen_model.train()
        L.disc_model.train()
        L.beta = 0.99
        L.set_requires_grad_disc(True)
        real = torch.rand(4, 3, 16, 16, device='cuda') * 2 - 1
        with _Census() as cd:
            L.d_step(real)
        L.set_requires_grad_disc(False)
        with _Census() as cg:
            L.g_step()
        torch.cuda.synchronize()
        seen[target] = (cd.symbols(), cg.symbols(), L.ada.p)
    upd = lambda syms: any('ada_update_kernel' in s for s in syms)  # noqa: E731
    assert not upd(seen[None][0]) and not upd(seen[None][1]) and seen[None][2] == float(np.float32(0.3))
    assert upd(seen[0.6][0]) and not upd(seen[0.6][1]) and seen[0.6][2] != float(np.float32(0.3))
    for d_syms, g_syms, _ in seen.values():
        assert any('ada_fwd_kernel' in s for s in d_syms) and not any('ada_adj_kernel' in s for s in d_syms)
        assert any('ada_fwd_kernel' in s for s in g_syms) and any('ada_adj_kernel' in s for s in g_syms)
        assert not any('diffaug' in s for s in d_syms | g_syms)


# ------------------------------------------------------------------------------------------------------------------- #
# learners
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind,loss,gp', [('stylegan', 'nonsaturating', 'r1'), ('progan', 'wgan', 'wgan-gp')])
def test_progressive_learner_step_matches_the_oracle(kind, loss, gp, small_widths):
    """tests/test_gpu_diffaug.py::test_progressive_learner_step_matches_the_oracle with ada='blit,geom,color' and fixed rows:
    d_step + g_step against oracle.nets on the CPU (float64) fed the restated transform.  Same bars: losses within 1e-3
    relative, every parameter gradient within 1e-3 by _grad_errors."""
    from gan_lab_amd.stylegan.architectures import StyleAddNoise
    from oracle import nets, ops as O, step
    torch.manual_seed(3)
    b, res = 4, 16
    L = make_learner(kind, res, batch=b, loss=loss, gradient_penalty=gp, random_seed=3, ada=FULL, ada_p=0.5)
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
    pd, pg = policy_rows(FULL, 2 * b, res, res, seed=21), policy_rows(FULL, b, res, res, seed=22)
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
    total = step.d_loss(od, cfg, ref_augment(fake, pd[:b]), ref_augment(real.double(), pd[b:]), loss, gp,
                        10.0, 1.0, 0.001, eps_interp=eps.double())
    total.backward()
    img = fwd(og, zg.double(), ng)
    olg = O.loss_gen(loss, nets.disc_forward(sd_d1, ref_augment(img, pg), cfg))
    olg.backward()
    assert rel_err(ld.cpu().double(), total.detach()) < 1e-3, (ld, total)
    assert rel_err(lg.cpu().double(), olg.detach()) < 1e-3, (lg, olg)
    for what, got, ref in (('d', gd, od), ('g', gg, og)):
        errs = _grad_errors(got, ref)
        assert len(errs) > 5
        worst = max(errs.items(), key=lambda kv: kv[1])
        assert worst[1] < 1e-3, f'{what} gradient {worst}'


def test_resnet_learner_step_matches_the_oracle():
    """tests/test_gpu_diffaug.py::test_resnet_learner_step_matches_the_oracle with ada='blit,geom,color' and fixed rows."""
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    from oracle import resnet
    from util import resnet_zero_grad_key
    torch.manual_seed(4)
    b, res = 4, 32
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=res, res_dataset=res, batch_size=b,
                      num_iters_save_model=10 ** 9, log_every=0, len_latent=16, ada=FULL, ada_p=0.5, random_seed=4)
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
    pd, pg = policy_rows(FULL, 2 * b, res, res, seed=31), policy_rows(FULL, b, res, res, seed=32)
    assert L._pair_critic_batches(torch.empty(b, 3, res, res), torch.empty(b, 3, res, res))
    L.set_requires_grad_disc(True)
    ld = L.d_step(real.cuda(), zb=zd.cuda(), eps_interp=eps.cuda(), aug_params=pd.cuda())
    gd = {k: v.grad.detach().cpu() for k, v in L.disc_model.named_parameters() if v.grad is not None}
    sd_d1 = {k: v.detach().cpu().double() for k, v in L.disc_model.state_dict().items()}
    L.set_requires_grad_disc(False)
    lg = L.g_step(zb=zg.cuda(), aug_params=pg.cuda())
    gg = {k: v.grad.detach().cpu() for k, v in L.gen_model.named_parameters() if v.grad is not None}
    assert L.ada.state[2].item() == b and L.ada.state[3].item() == 1          # the D step fed the controller once

    dbl = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}  # noqa: E731
    gan = resnet.ResnetFunctionalGAN(dbl(sd_g), dbl(sd_d), res, loss='wgan', gp='wgan-gp')
    with torch.no_grad():
        fake = gan.gen(zd.double())
    total = gan.d_loss(ref_augment(fake, pd[:b]), ref_augment(real.double(), pd[b:]), eps.double())
    total.backward()
    out = gan.disc(ref_augment(gan.gen(zg.double()), pg), sd_d1)
    olg = -out.mean()
    olg.backward()
    assert rel_err(ld.cpu().double(), total.detach()) < 1e-3, (ld, total)
    assert rel_err(lg.cpu().double(), olg.detach()) < 1e-3, (lg, olg)
    for what, got, ref in (('d', gd, gan.d), ('g', gg, gan.g)):
        errs = _grad_errors(got, {k: v for k, v in ref.items() if not resnet_zero_grad_key(k)}, floor=1e-4)
        assert len(errs) > 5
        worst = max(errs.items(), key=lambda kv: kv[1])
        assert worst[1] < 1e-3, f'{what} gradient {worst}'


def test_paired_critic_pass_equals_two_passes_with_ada(small_widths, monkeypatch):
    """With ADA on, the paired ProGAN WGAN-GP critic pass (one launch over [fake; real] with the (2B, 32) block) sees the same
    augmented batches bit for bit as the two-pass path, and the controller the same statistics."""
    from gan_lab_amd import ops, rng
    from util import assert_close
    b, res = 4, 16
    seen, out = {}, {}
    orig = ops.ada_augment

    def spy(x, params):
        y = orig(x, params)
        seen.setdefault(pair, []).append(y.detach().clone())
        return y
    monkeypatch.setattr(ops, 'ada_augment', spy)
    gen = torch.Generator().manual_seed(9)
    real = (torch.rand(b, 3, res, res, generator=gen) * 2 - 1).cuda()
    zd = torch.randn(b, 16, generator=gen).cuda()
    eps = torch.rand(b, 1, 1, 1, generator=gen).cuda()
    for pair in ('0', '1'):
        monkeypatch.setenv('GANLAB_CRITIC_PAIR', pair)
        torch.manual_seed(5)
        rng.manual_seed(5)
        L = make_learner('progan', res, batch=b, loss='wgan', gradient_penalty='wgan-gp', random_seed=5, ada=FULL, ada_p=0.8)
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
        assert rng._STATE['offset'] == off + 8 * 2 * b          # one (2B, 32) draw
        out[pair] = (ld.cpu(), L.arena_d.gflat.detach().cpu().clone(), L.ada.state.cpu().clone())
    assert [t.shape[0] for t in seen['0']] == [b, b] and [t.shape[0] for t in seen['1']] == [2 * b]
    assert torch.equal(torch.cat(seen['0']), seen['1'][0])
    assert not torch.equal(seen['1'][0][b:], real)               # p = 0.8: the batch really was transformed
    assert out['0'][1].abs().max() > 0
    assert_close(out['1'][0], out['0'][0], 1e-6, 'loss_d')
    assert_close(out['1'][1], out['0'][1], 1e-5, 'critic gradients')
    assert out['0'][2][2].item() == b and out['0'][2][3].item() == 1 and out['1'][2][2:].tolist() == out['0'][2][2:].tolist()


def test_train_with_ada_stays_finite_and_is_reproducible(small_widths):
    """train() with ADA on (adaptive p) runs through a short growth schedule (8 -> 16) and stays finite; two runs from the
    same seeds agree bit for bit, the controller's state included."""
    from gan_lab_amd import rng
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader

    def run():
        torch.manual_seed(7)
        np.random.seed(7)
        rng.manual_seed(1)
        L = make_learner('stylegan', 16, init_res=8, batch=4, loss='nonsaturating', gradient_penalty='r1', random_seed=7,
                         ada=FULL, ada_p=0.5, ada_target=2.0, ada_interval=2, ada_kimg=0.2)      # (see below)
        L.log_every = 1
        dl = SyntheticImageLoader(4096, 4, 8, seed=3)
        L.train(dl, num_main_iters=6 * 3 + 2)
        torch.cuda.synchronize()
        return L, {k: v.detach().clone() for k, v in list(L.gen_model.state_dict().items()) +
                   [('d.' + k, v) for k, v in L.disc_model.state_dict().items()] + [('ada', L.ada.state)]}
    L, a = run()
    assert L.gen_model.curr_res == 16 and not L.gen_model.fade_in_phase
    assert np.isfinite(L.last_losses['loss_d']) and np.isfinite(L.last_losses['loss_g'])
    assert all(torch.isfinite(v).all() for v in a.values() if v.is_floating_point())
    # the controller ran: sign(D(real)) averages to at most 1, so against the unreachable target 2 every one of the 10
    # adjustments (20 D steps, interval 2) steps down by 4 * 2 / 200 = 0.04
    assert abs(L.ada.p - 0.1) < 1e-5 and L.ada.state[1:].tolist() == [0.0, 0.0, 0.0]
    del L
    _, b2 = run()
    diff = [k for k in a if not torch.equal(a[k], b2[k])]
    assert not diff, diff[:4]


@pytest.mark.parametrize('kind', ['stylegan', 'progan'])
def test_graphed_step_equals_eager_with_ada(kind):
    """graphs.GraphedStep with ADA on: every replay draws fresh rows at the device-resident p and runs the controller inside
    the graph; parameters, Adam moments, EWMA generator, both losses and the controller's state block equal the eager steps
    BIT FOR BIT after 6 iterations, 4 of them (2 x ada_interval) replayed."""
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
        # (target 2 is out of reach of a mean of signs: p steps down by 4 * 2 / 100 at every adjustment, so its trajectory is
        # known; the accumulated sign sums, compared after every step, are what depends on the critic's outputs)
        L = make_learner(kind, 32, batch=4, random_seed=21, ada=FULL, ada_p=0.5, ada_target=2.0, ada_interval=2, ada_kimg=0.1,
                         **kw)
        L.gen_model.train()
        L.disc_model.train()
        L.beta = 0.99
        torch.manual_seed(10)
        stepper = GraphedStep(L, warmup=2)
        losses, ps = [], []
        for x in reals:
            if graphed:
                ld, lg = stepper(x)
            else:
                _, kw_d = stepper._mix_kwargs()
                ld = stepper._d_half(x, kw_d)
                _, kw_g = stepper._mix_kwargs()
                lg = stepper._g_half(kw_g)
            losses.append((float(ld), float(lg)))
            ps.append(L.ada.state.cpu().tolist())
        torch.cuda.synchronize()
        state = {'g': L.arena_g.flat.clone(), 'd': L.arena_d.flat.clone(), 'lag': L.ewma.flat.clone(),
                 'ada': L.ada.state.clone()}
        for name, opt in (('og', L.opt_gen), ('od', L.opt_disc)):
            ex = opt.export_moments(list(L.gen_model.named_parameters()) if name == 'og' else
                                    list(L.disc_model.named_parameters()))
            for k2, v in ex['exp_avg'].items():
                state[f'{name}.m.{k2}'] = v
            for k2, v in ex['exp_avg_sq'].items():
                state[f'{name}.v.{k2}'] = v
        return state, losses, ps, (len(stepper.graphs) if graphed else 0), rng._STATE['offset']
    try:
        a, la, pa, n_graphs, off_a = run(True)
        b, lb, pb, _, off_b = run(False)
    finally:
        P.FMAP_BASE, P.FMAP_MAX = 8192, 512
    assert n_graphs >= 2, 'nothing was captured'
    assert off_a == off_b, 'the device random stream advanced differently'
    assert pa == pb, (pa, pb)                                   # the trajectory of (p, acc_sum, acc_n, calls)
    assert len({s[0] for s in pb}) == 4 and [s[3] for s in pb] == [1.0, 0.0] * 3       # p moved at every second step
    assert la == lb, (la, lb)
    diff = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not diff, f'{len(diff)} of {len(a)} tensors differ between replayed and eager steps, e.g. {diff[:4]}'


def test_checkpoint_round_trip_of_the_state_block(tmp_path, small_widths):
    """Save at a p strictly between 0 and 1 with half-filled accumulators, load into a fresh learner: the state block is
    restored and the next adjustment lands on the same p.  The ResNet GAN's file and the progressive learners' plain-format
    dict both carry it, and neither has an ``ada*`` entry while ADA is off."""
    from gan_lab_amd import ada, checkpoint as ckpt
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader

    def build(**kw):
        cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                          num_iters_save_model=10 ** 9, log_every=0, len_latent=16, num_disc_iters=1, random_seed=4, **kw)
        cfg.fmap_g, cfg.fmap_d = 8, 8
        return GANLearner(cfg)
    kw = dict(ada=FULL, ada_p=0.25, ada_interval=4, ada_kimg=0.2)
    L = build(**kw)
    L.train(SyntheticImageLoader(64, 4, 32), num_main_iters=2)
    assert L.ada.state[3].item() == 2 and L.ada.state[2].item() == 8          # two D steps into an interval of four
    with torch.no_grad():
        L.ada.state.copy_(torch.tensor([0.4, 3.0, 8.0, 2.0]))
    path = tmp_path / 'resnetgan_model.tar'
    L.save_model(path)
    ck = ckpt.load_checkpoint(path)
    assert ck['ada_state'] == dict(p=float(np.float32(0.4)), acc_sum=3.0, acc_n=8.0, calls=2.0)
    assert ck['config']['ada'] == FULL and ck['config']['ada_interval'] == 4
    L2 = build(**kw)
    assert L2.ada.p == 0.25
    L2.load_model(path)
    assert torch.equal(L2.ada.state, L.ada.state)
    logits = torch.tensor([1.0, 2.0, -1.0, 0.5], device='cuda')
    for _ in range(2):
        for lr in (L, L2):
            lr.ada.update(logits)
    step = ada.step_size(4, 1, 4, 0.2)
    want = ada.next_p(0.4, 3.0 + 2 * 2, 8.0 + 2 * 4, 0.6, step)
    assert L.ada.p == L2.ada.p == want and want != float(np.float32(0.4))
    assert L2.ada.state.cpu().tolist() == [want, 0.0, 0.0, 0.0]
    # ADA off: no trace in the file
    L3 = build()
    L3.train(SyntheticImageLoader(64, 4, 32), num_main_iters=1)
    L3.save_model(tmp_path / 'plain.tar')
    ck = ckpt.load_checkpoint(tmp_path / 'plain.tar')
    assert 'ada_state' not in ck and not [k for k in ck['config'] if k.startswith('ada')]
    # the progressive learners' plain-format dict
    P = make_learner('progan', 16, batch=4, loss='wgan', gradient_penalty='wgan-gp', random_seed=2, ada='blit', ada_p=0.5,
                     ada_target=None)
    P.train(SyntheticImageLoader(4096, 4, 16), num_main_iters=1)
    d = P._plain_checkpoint_dict()
    assert d['ada_state']['p'] == 0.5 and d['config']['ada'] == 'blit'
    P = make_learner('progan', 16, batch=4, loss='wgan', gradient_penalty='wgan-gp', random_seed=2)
    P.train(SyntheticImageLoader(4096, 4, 16), num_main_iters=1)
    d = P._plain_checkpoint_dict()
    assert 'ada_state' not in d and not [k for k in d['config'] if k.startswith('ada')]
