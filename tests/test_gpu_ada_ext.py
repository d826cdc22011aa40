"""GPU tests of ADA's filter, noise and cutout groups (csrc/ada_filter.hip, ops.ada_augment with ext rows, rng.ada_params
under a policy with a new group, the learners' steps under the six-part policy) against tests/ada_ext_reference.py.

Shapes: N = 3..5 at 4x4 (the halo is 7 periods of reflection), 8x8, 16x20, 24x24 (the first size where torch's own reflect
pad applies), 32x64 and 40x72 (the first with several tiles in both axes and a ragged last tile)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ada_ext_reference as R
from test_gpu_diffaug import _philox4x32_10, make_learner, small_widths  # noqa: F401

pytestmark = pytest.mark.gpu

THREE, SIX = 'blit,geom,color', 'blit,geom,color,filter,noise,cutout'
SHAPES = [(3, 4, 4), (4, 8, 8), (5, 16, 20), (3, 24, 24), (4, 32, 64), (3, 40, 72)]
IDS = [f'{n}x{h}x{w}' for n, h, w in SHAPES]
_BANK = {}


def bank():
    """The library's table, read once."""
    if 'b' not in _BANK:
        from gan_lab_amd import ops
        _BANK['b'] = ops.ada_filter_bank()
    return _BANK['b']


def identity_rows(n):
    from gan_lab_amd import ada
    return ada.rows_from_matrices(torch.tensor([[[1.0, 0, 0], [0, 1, 0]]]).expand(n, 2, 3)).cuda()


def hand_rows(n, h, w, gen):
    """Hand-made ext rows: gains inside the clamp's range (log2-normal, +-3), a noise scale and a rectangle on some rows; row 1
    has every gate closed (a copy), row 2 is filtered with a rectangle as well."""
    from gan_lab_amd import ada
    g = 2.0 ** torch.randn(n, 4, generator=gen).clamp(-3, 3)
    g[1] = 1.0
    sigma = torch.tensor([0.05 * (k % 2) for k in range(n)])
    rect = torch.zeros(n, 4)
    rect[0] = torch.tensor([1, w - 1, 0, (h + 1) // 2])
    rect[2] = torch.tensor([0, w // 2, 1, h])
    return ada.ext_rows(g, sigma, rect)


def drawn(policy, n, h, w, p, seed=3):
    from gan_lab_amd import ada, rng
    rng.manual_seed(seed)
    state = torch.tensor([p, 0, 0, 0], dtype=torch.float32, device='cuda')
    return rng.ada_params(n, h, w, state, ada.parse_policy(policy))


# ------------------------------------------------------------------------------------------------------------------- #
# the table and the parameter rows
# ------------------------------------------------------------------------------------------------------------------- #
def test_exported_table_is_the_recipe():
    from gan_lab_amd import ada
    assert tuple(bank().shape) == (4, 43) and (bank() - ada.filter_bank()).abs().max().item() <= 1e-15


@pytest.mark.parametrize('p', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('policy', [SIX, 'filter', 'noise', 'cutout', 'blit,geom,color,noise,cutout', 'filter,cutout'])
def test_ext_rows_restated_from_philox(policy, p):
    """The normative mapping: sample n takes the 16 words of counters offset + 4n .. offset + 4n + 3, offset being the position
    after the batch's main block.  Gates, rectangle, raw z and the centre are exact; g and sigma are within 1 fp32 ulp of the
    float64 composition.  The offset crosses a 32-bit boundary of the counter; the key uses both halves of the seed."""
    from gan_lab_amd import ada, ops
    seed, offset, n, h, w = 0x0123456789ABCDEF, 2 ** 32 - 20, 24, 40, 72
    mask = ada.parse_policy(policy)
    state = torch.tensor([p, 7, 8, 1], dtype=torch.float32, device='cuda')
    got = ops.ada_ext_params(n, h, w, state, mask, seed, offset, 'cuda').cpu()
    assert torch.equal(state.cpu(), torch.tensor([p, 7, 8, 1], dtype=torch.float32))         # the draw only reads the block
    fired = 0
    for k in range(n):
        words = sum((_philox4x32_10(offset + 4 * k + c, seed) for c in range(4)), [])
        bits, rect, z, cx, cy, g, sigma = R.restated_row(words, h, w, p, mask)
        fired |= bits
        assert got[k, 5:].tolist() == [float(v) for v in rect + [bits] + z + [cx, cy]], (k, got[k], rect, bits, z, cx, cy)
        want = torch.tensor(list(g) + [sigma])
        err = (got[k, :5].double() - want).abs()
        assert (err <= 2.0 ** -23 * want.abs()).all(), (k, got[k, :5], want)
        if bits & 15 == 0:
            assert got[k, :4].tolist() == [1.0, 1.0, 1.0, 1.0]
        assert got[k, 10:14].abs().max() <= 3
    allowed = (15 if mask & 8 else 0) | (16 if mask & 16 else 0) | (32 if mask & 32 else 0)
    assert fired & ~allowed == 0
    assert fired == (allowed if p == 1.0 else 0) or 0.0 < p < 1.0


def test_stream_advance_and_the_three_group_policy():
    """A draw advances the stream by 8N, plus 4N with any new group, plus ceil(3NHW / 4) with noise; the three-group policy
    draws today's rows and advances by 8N (N = 5: 40).  Ext rows and the noise field sit where the rule says, the
    device-base form equals the by-value form, and a policy's new groups leave the main rows alone."""
    from gan_lab_amd import ada, ops, rng
    n, h, w = 5, 16, 20
    state = torch.tensor([0.7, 0, 0, 0], dtype=torch.float32, device='cuda')
    rng.manual_seed(11)
    seed, off0 = rng._STATE['seed'], rng._STATE['offset']
    rows = rng.ada_params(n, h, w, state, ada.parse_policy(THREE))
    assert isinstance(rows, torch.Tensor) and rng._STATE['offset'] - off0 == 40
    assert torch.equal(rows, ops.ada_params(n, h, w, state, 7, seed, off0, 'cuda'))
    for policy, want in ((SIX, 40 + 20 + 1200), ('blit,geom,color,filter,cutout', 60), ('noise', 60 + 1200), ('cutout', 60)):
        rng.manual_seed(11)
        mask = ada.parse_policy(policy)
        d = rng.ada_params(n, h, w, state, mask)
        assert isinstance(d, ops.AdaDraw) and len(d) == n
        assert rng._STATE['offset'] - off0 == want == 8 * n + 4 * n + (math.ceil(3 * n * h * w / 4) if mask & 16 else 0)
        assert torch.equal(d.params, ops.ada_params(n, h, w, state, mask & 7, seed, off0, 'cuda'))
        if mask & 7 == 7:
            assert torch.equal(d.params, rows)
        assert torch.equal(d.ext, ops.ada_ext_params(n, h, w, state, mask, seed, off0 + 8 * n, 'cuda'))
        if mask & 16:
            assert torch.equal(d.noise, ops.randn((n, 3, h, w), seed, off0 + 12 * n, 'cuda'))
        else:
            assert d.noise is None
        half = d[2:]
        assert torch.equal(half.ext, d.ext[2:]) and len(half) == 3
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    ops.set_step_scalars(block, 1000, [])
    a = ops.ada_ext_params(64, h, w, state, 63, seed, 1000 + 37, 'cuda')
    assert torch.equal(a, ops.ada_ext_params_dev(64, h, w, state, 63, seed, block, 37, 'cuda'))


def test_gate_frequencies_and_the_ends():
    """Over N = 4096 rows each of the six gates fires with probability p within 5 standard deviations, never at p = 0 and always
    at p = 1."""
    from gan_lab_amd import ops
    n = 4096
    for p in (0.0, 0.3, 1.0):
        state = torch.tensor([p, 0, 0, 0], dtype=torch.float32, device='cuda')
        bits = ops.ada_ext_params(n, 32, 32, state, 63, 77, 0, 'cuda')[:, 9].long().cpu()
        q = float(np.float32(p))
        for k in range(6):
            freq = ((bits >> k) & 1).double().mean().item()
            assert abs(freq - q) <= 5 * math.sqrt(q * (1 - q) / n), (p, k, freq)
        if p == 0.0:
            assert (bits == 0).all()
        if p == 1.0:
            assert (bits == 63).all()


# ------------------------------------------------------------------------------------------------------------------- #
# forward and adjoint
# ------------------------------------------------------------------------------------------------------------------- #
def _in_units(got, ref64, unit):
    return ((got.double().cpu() - ref64).abs() / unit.clamp(min=1e-300)).max().item()


@pytest.mark.parametrize('n,h,w', SHAPES, ids=IDS)
@pytest.mark.parametrize('rows', ['hand', 'drawn'])
def test_forward_and_adjoint_against_float64(rows, n, h, w):
    """The kernels against the float64 restatement, the error counted at each pixel in units of 2^-24 (|h| * |h| * |x|), and
    ATen's CPU fp32 composition (gather by r, two grouped conv2d; its autograd for the adjoint) measured on the same inputs
    in the same unit: the kernel's maximum may be at most twice ATen's (a different but equally long summation order).  That
    comparison runs without a noise field, so the unit is the plain one; the field is then added in a comparison of its own:
    the output with it is fma(sigma, noise, output without it) within 1 ulp outside the rectangle, and bit-equal on rows
    whose sigma is 0.  Measured on an MI355X, forward / adjoint, kernel vs ATen: see DESIGN.md 4.6."""
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(100 * h + w)
    x = torch.rand(n, 3, h, w, generator=gen) * 2 - 1
    g = torch.randn(n, 3, h, w, generator=gen)
    if rows == 'hand':
        ext, noise = hand_rows(n, h, w, gen), torch.randn(n, 3, h, w, generator=gen)
    else:
        d = drawn(SIX, n, h, w, 1.0, seed=h + w)
        ext, noise = d.ext.cpu(), d.noise.cpu()
        assert (ext[:, 9] == 63).all()
    y = ops.k_ada_ext(x.cuda(), ext.cuda()).cpu()
    ref, unit = R.apply(x, ext, None, bank()), R.unit(x, ext, bank())
    keep = R.keep_mask(ext, h, w).expand_as(ref) > 0
    assert (y[~keep] == 0).all()
    e_k = _in_units(y[keep], ref[keep], unit[keep])
    e_a = _in_units(R.apply(x, ext, None, bank(), torch.float32)[keep], ref[keep], unit[keep])
    yn = ops.k_ada_ext(x.cuda(), ext.cuda(), noise.cuda()).cpu()
    sig = R.sigma(ext)
    assert (sig > 0).any() and (yn[~keep] == 0).all() and torch.equal(yn[sig == 0], y[sig == 0])
    want = y.double() + sig.view(-1, 1, 1, 1) * noise.double()
    ulp = 2.0 ** (torch.floor(torch.log2(yn.double().abs().clamp(min=2.0 ** -126))) - 23)
    assert ((yn.double() - want).abs() <= ulp)[keep].all()
    gx = ops.k_ada_ext(g.cuda(), ext.cuda(), adjoint=True)
    gref, gunit = R.adjoint(g, ext, bank()), R.adjoint_unit(g, ext, bank())
    live = gunit > 0
    assert (gx.cpu()[~live] == 0).all()
    b_k = _in_units(gx.cpu()[live], gref[live], gunit[live])
    b_a = _in_units(R.adjoint(g, ext, bank(), torch.float32)[live], gref[live], gunit[live])
    print(f'ada_ext {rows} {n}x{h}x{w}: forward kernel {e_k:.3f} ATen {e_a:.3f} units; '
          f'adjoint kernel {b_k:.3f} ATen {b_a:.3f} units')
    assert e_k <= 2 * e_a, (e_k, e_a)
    assert b_k <= 2 * b_a, (b_k, b_a)


@pytest.mark.parametrize('n,h,w', SHAPES, ids=IDS)
def test_adjointness(n, h, w):
    """<F x, g> = <x, F^T g> with both sides summed in float64 from the kernels' outputs.  Tolerance: every output is a chain of
    at most c = 2 (43 + 1) P fp32 operations, P = 2 ceil((min(H, W) + 42) / (2 (min(H, W) - 1))) being the most pre-images a
    pixel has along an axis (1 for the forward), each off by at most 2^-24 of the sum of the magnitudes - the unit; so each side
    is within c 2^-24 <|F| |x|, |g|> of the exact pairing, and <|F| |x|, |g|> = <|x|, |F|^T |g|>."""
    from gan_lab_amd import ops
    gen = torch.Generator().manual_seed(7 * h + w)
    x = torch.rand(n, 3, h, w, generator=gen) * 2 - 1
    g = torch.randn(n, 3, h, w, generator=gen)
    ext = hand_rows(n, h, w, gen)
    y = ops.k_ada_ext(x.cuda(), ext.cuda()).double().cpu()
    gx = ops.k_ada_ext(g.cuda(), ext.cuda(), adjoint=True).double().cpu()
    lhs, rhs = (y * g.double()).sum().item(), (x.double() * gx).sum().item()
    m = min(h, w)
    chain = 2 * 44 * 2 * math.ceil((m + 42) / (2 * (m - 1)))
    scale = (R.unit(x, ext, bank()) * R.keep_mask(ext, h, w) * g.double().abs()).sum().item()        # 2^-24 <|F||x|, |g|>
    print(f'ada_ext adjointness {n}x{h}x{w}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {2 * chain * scale:.3e}, lhs {lhs:.6f}')
    assert abs(lhs - rhs) <= 2 * chain * scale


# ------------------------------------------------------------------------------------------------------------------- #
# exactness
# ------------------------------------------------------------------------------------------------------------------- #
def test_closed_gates_are_exact_copies():
    """p = 0, or an empty gate mask in a hand-made row whatever its gains, sigma and rectangle say: the output is
    ops.ada_augment(x, params) bit for bit, forward and backward."""
    from gan_lab_amd import ada, ops
    n, h, w = 3, 40, 72
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand(n, 3, h, w, generator=gen) * 2 - 1).cuda()
    g = torch.randn(n, 3, h, w, generator=gen).cuda()
    d = drawn(SIX, n, h, w, 0.0)
    assert (d.ext[:, 9] == 0).all() and torch.equal(d.ext[:, :9].cpu(), ada.ext_rows(n=n)[:, :9])
    rows3 = drawn(THREE, n, h, w, 0.7)
    # gains, a noise scale and a rectangle without a gate bit: still a copy
    empty = ada.ext_rows(g=torch.full((n, 4), 2.0), sigma=[0.3] * n, rect=[[0, w // 2, 0, h // 2]] * n, gates=[0] * n).cuda()
    field = torch.randn(n, 3, h, w, generator=gen).cuda()
    for params, ext, noise in ((d.params, d.ext, d.noise), (rows3, empty, field), (rows3, ada.ext_rows(n=n).cuda(), None)):
        xr = x.clone().requires_grad_(True)
        y = ops.ada_augment(xr, params, ext, noise)
        xb = x.clone().requires_grad_(True)
        base = ops.ada_augment(xb, params)
        assert torch.equal(y, base)
        assert torch.equal(torch.autograd.grad(y, xr, g)[0], torch.autograd.grad(base, xb, g)[0])


@pytest.mark.parametrize('n,h,w', [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_perfect_reconstruction(n, h, w):
    """Gains (1, 1, 1, 1) with a forced gate bit run the filter on the bank's sum, the unit impulse within 7e-16: the input comes
    back within one unit (pixels in +-[0.25, 1], so that no unit is small against the 1e-16 taps)."""
    from gan_lab_amd import ada, ops
    gen = torch.Generator().manual_seed(2)
    x = (torch.rand(n, 3, h, w, generator=gen) * 0.75 + 0.25) * (torch.randint(0, 2, (n, 3, h, w), generator=gen) * 2 - 1)
    ext = ada.ext_rows(gates=[1, 2, 15][:n] + [8] * (n - 3), n=n)
    y = ops.ada_augment(x.cuda(), identity_rows(n), ext.cuda()).cpu()
    err = _in_units(y, x.double(), R.unit(x, ext, bank()))
    print(f'ada_ext perfect reconstruction {n}x{h}x{w}: {err:.3f} units')
    assert err <= 1.0


def test_cutout_zeroes_the_restated_rectangle():
    """Drawn at p = 1 under 'cutout': inside the rectangle restated from the centre columns the output is 0, elsewhere it is the
    input bit for bit; the gradient through it is the mask."""
    from gan_lab_amd import ops
    n, h, w = 5, 16, 20
    d = drawn('cutout', n, h, w, 1.0, seed=9)
    ext = d.ext.cpu()
    x = (torch.rand(n, 3, h, w) * 2 - 1 + 3).cuda().requires_grad_(True)              # no zero in the input
    y = ops.ada_augment(x, d.params, d.ext)
    inside = torch.zeros(n, 1, h, w, dtype=torch.bool)
    for k in range(n):
        cx, cy = ext[k, 14].item(), ext[k, 15].item()
        jj = torch.tensor([abs((j + 0.5) / w - cx) < 0.25 for j in range(w)])
        ii = torch.tensor([abs((i + 0.5) / h - cy) < 0.25 for i in range(h)])
        inside[k, 0] = ii.view(h, 1) & jj.view(1, w)
    assert inside.any() and not inside.all()
    inside = inside.expand(n, 3, h, w)
    assert torch.equal(y.detach().cpu() == 0, inside)
    assert torch.equal(y.detach().cpu()[~inside], x.detach().cpu()[~inside])
    g = torch.randn(n, 3, h, w).cuda()
    gx = torch.autograd.grad(y, x, g)[0]
    assert torch.equal(gx.cpu(), torch.where(inside, torch.zeros(()), g.cpu()))


def test_noise_is_sigma_times_the_field_at_its_stream_position():
    """Filter off ('blit,geom,color,noise' at p = 1): y - warp_color(x) equals sigma[n] randn at the stream position right after
    the ext block within 1 ulp of y, and the gradient through the noise is that of warp_color alone."""
    from gan_lab_amd import ada, ops, rng
    n, h, w = 4, 24, 24
    policy = 'blit,geom,color,noise'
    d = drawn(policy, n, h, w, 1.0, seed=13)
    field = ops.randn((n, 3, h, w), rng._STATE['seed'], 12 * n, 'cuda')      # the seed's stream started at 0
    assert torch.equal(d.noise, field) and (d.ext[:, 4] > 0).all() and (d.ext[:, 9] == 16).all()
    aug = ada.AdaptiveAugment(policy, p=1.0, target=None)
    x = (torch.rand(n, 3, h, w) * 2 - 1).cuda().requires_grad_(True)
    y = aug(x, d)
    xb = x.detach().clone().requires_grad_(True)
    base = ops.ada_augment(xb, d.params)
    want = base.detach().double() + d.ext[:, 4].double().view(-1, 1, 1, 1) * field.double()
    ulp = 2.0 ** (torch.floor(torch.log2(y.detach().double().abs().clamp(min=2.0 ** -126))) - 23)
    assert ((y.detach().double() - want).abs() <= ulp).all()
    assert not torch.equal(y.detach(), base.detach())
    g = torch.randn(n, 3, h, w).cuda()
    assert torch.equal(torch.autograd.grad(y, x, g)[0], torch.autograd.grad(base, xb, g)[0])


def test_reproducible_gradients_and_errors():
    """Two calls are bitwise equal, forward and backward; torch.autograd.grad of a weighted sum is the restated adjoint
    A^T F^T (mask o g) composed from the two adjoint kernels; the double backward raises; wrong operands raise."""
    from gan_lab_amd import ops
    n, h, w = 3, 40, 72
    d = drawn(SIX, n, h, w, 1.0, seed=21)
    gen = torch.Generator().manual_seed(4)
    x0 = (torch.rand(n, 3, h, w, generator=gen) * 2 - 1).cuda()
    g = torch.randn(n, 3, h, w, generator=gen).cuda()
    outs = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        y = ops.ada_augment(x, d.params, d.ext, d.noise)
        gx, = torch.autograd.grad((y * g).sum(), x, create_graph=True)
        outs.append((y.detach().clone(), gx.detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][1], ops.k_ada(ops.k_ada_ext(g, d.ext, adjoint=True), d.params, adjoint=True))
    inner = R.adjoint(g.cpu(), d.ext.cpu(), bank())
    got = ops.k_ada_ext(g, d.ext, adjoint=True).double().cpu()
    chain = 2 * 44 * 2 * math.ceil((h + 42) / (2 * (h - 1)))           # test_adjointness derives it
    assert ((got - inner).abs() <= chain * R.adjoint_unit(g.cpu(), d.ext.cpu(), bank())).all()
    x = x0.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(ops.ada_augment(x, d.params, d.ext, d.noise).square().sum(), x, create_graph=True)
    with pytest.raises(NotImplementedError, match='ada_augment'):
        gx.sum().backward()
    with pytest.raises(ValueError):
        ops.ada_augment(x0, d.params, d.ext[:2], None)
    with pytest.raises(ValueError):
        ops.ada_augment(x0[:2], d.params[:2], d.ext[:2], d.noise)
    with pytest.raises(ValueError):
        ops.ada_augment(x0, d.params, None, d.noise)
    with pytest.raises(TypeError):
        ops.ada_augment(x0, d.params, d.ext.cpu())


# ------------------------------------------------------------------------------------------------------------------- #
# learners
# ------------------------------------------------------------------------------------------------------------------- #
def _state(L):
    return {k: v.detach().clone() for k, v in list(L.gen_model.state_dict().items()) +
            [('d.' + k, v) for k, v in L.disc_model.state_dict().items()] + [('ada', L.ada.state)]}


def test_resnet_learner_trains_with_the_six_part_policy():
    """A ResNet GAN 32-pixel learner under the six-part policy at fixed p = 0.5 steps a few iterations, stays finite and is
    bitwise equal across two seeded runs, the stream position included.  A run is a process of its own
    (tests/ada_ext_resnet_worker.py; the two go side by side): the gradients of a ResNet GAN learner round differently with
    what its process ran before it, with ada=None as well (tests/test_gpu_cr.py), and three Adam steps turn that rounding into
    signs on the biases in front of a norm layer, so two learners of ONE process are not what "two runs" can mean here."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ada_ext_resnet_worker.py')
    procs = [subprocess.Popen([sys.executable, worker], stdout=subprocess.PIPE, text=True) for _ in range(2)]
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), [p.returncode for p in procs]
    a, b = (json.loads(o.strip().splitlines()[-1]) for o in outs)
    assert a['p'] == 0.5 and a['finite'] and all(math.isfinite(v) for pair in a['losses'] for v in pair)
    assert len(a['losses']) == 3 and len(a['digests']) > 50
    assert a['losses'] == b['losses'] and a['offset'] == b['offset'] > 0
    diff = [k for k in a['digests'] if a['digests'][k] != b['digests'][k]]
    assert not diff, diff[:4]


def test_stylegan_learner_trains_with_the_six_part_policy(small_widths):
    """A small-width StyleGAN learner under the six-part policy at fixed p = 0.5 trains through 8 -> 16, stays finite and is
    bitwise equal across two seeded runs."""
    from gan_lab_amd import rng
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader

    def run():
        torch.manual_seed(7)
        np.random.seed(7)
        rng.manual_seed(1)
        L = make_learner('stylegan', 16, init_res=8, batch=4, loss='nonsaturating', gradient_penalty='r1', random_seed=7,
                         ada=SIX, ada_p=0.5, ada_target=None)
        L.log_every = 1
        L.train(SyntheticImageLoader(4096, 4, 8, seed=3), num_main_iters=6 * 3 + 2)
        torch.cuda.synchronize()
        return L, _state(L)
    L, a = run()
    assert L.gen_model.curr_res == 16 and not L.gen_model.fade_in_phase and L.ada.p == 0.5
    assert np.isfinite(L.last_losses['loss_d']) and np.isfinite(L.last_losses['loss_g'])
    assert all(torch.isfinite(v).all() for v in a.values() if v.is_floating_point())
    del L
    _, b = run()
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff[:4]


def test_graphed_step_equals_eager_with_the_six_part_policy():
    """graphs.GraphedStep of the progressive (StyleGAN) learner under the six-part policy: every replay draws fresh rows, ext rows
    and a fresh noise field at the device-resident p; parameters, Adam moments, EWMA generator, both losses, the state block
    and the stream position equal the eager steps BIT FOR BIT after 6 iterations."""
    from gan_lab_amd import progressive as P, rng
    from gan_lab_amd.graphs import GraphedStep
    gen = torch.Generator().manual_seed(17)
    reals = [(torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(6)]

    def run(graphed):
        P.FMAP_BASE, P.FMAP_MAX = 1024, 64
        torch.manual_seed(9)
        np.random.seed(9)
        L = make_learner('stylegan', 32, batch=4, random_seed=21, ada=SIX, ada_p=0.5, ada_target=2.0, ada_interval=2,
                         ada_kimg=0.1, loss='nonsaturating', gradient_penalty='r1')
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
    assert pa == pb, (pa, pb)
    assert la == lb, (la, lb)
    assert all(math.isfinite(v) for pair in la for v in pair)
    diff = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not diff, f'{len(diff)} of {len(a)} tensors differ between replayed and eager steps, e.g. {diff[:4]}'
