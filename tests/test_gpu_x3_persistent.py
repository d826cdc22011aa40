"""The persistent split-product conv kernels with many tiles per workgroup (csrc/conv_x3.hip, conv_x3_up.hip, conv_x3_down.hip).

All three launch min(ntiles, 256) workgroups; workgroup b takes the tiles remap(b) + i * G and runs its k-loop on from one tile
into the next.  The activation ring slot, the weight double-buffer parity and the next tile's prologue (staged under this tile's
epilogue) carry across that boundary, so a case with one tile per workgroup says nothing about them.  Every case here restates
the launcher's tile count and grid in Python and asserts how many tiles per workgroup it gives and which carried states the
workgroups start their tiles in; the launch itself is checked to have used that grid.

Each case compares the whole output with the exact-fp32 kernels (set_x3(False)) and three images - the first, one in the middle
and the last, on different tile iterations i - with float64 on the CPU, at the bars of tests/test_gpu_x3.py.  A failure names the
worst tile and the workgroup and iteration that computed it."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import assert_close

pytestmark = pytest.mark.gpu
TOL = 2e-4
GRID_MAX = 256          # every persistent launcher: grid = min(ntiles, 256)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gan_lab_amd import ops as _ops, _lib
    _lib.lib()
    return _ops


def rms_rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


# ---- the launch geometry, restated --------------------------------------------------------------------------------------------
def xcd_remap(b, n):
    """common.h gl_xcd_remap: the first tile of workgroup b of a grid of n."""
    q, r, xcd, i = n >> 3, n & 7, b & 7, b >> 3
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + i


class Tiling:
    """One launch of a persistent kernel.  ``digits``: the kernel's tile decode, innermost first, as (name, count) pairs - the
    tile index is the mixed-radix number they spell, with the image index n outermost.  ``state(k)``: the carried state a
    workgroup starts its k-th tile in."""

    def __init__(self, kernel, n, digits, state):
        self.kernel, self.n, self.digits, self.state = kernel, n, digits, state
        self.per_image = 1
        for _, c in digits:
            self.per_image *= c
        self.ntiles = n * self.per_image
        self.grid = min(self.ntiles, GRID_MAX)
        self.first = [xcd_remap(b, self.grid) for b in range(self.grid)]
        assert sorted(self.first) == list(range(self.grid))          # gl_xcd_remap is a bijection of the grid
        self.owner_of = {t: b for b, t in enumerate(self.first)}
        counts = [(self.ntiles - t + self.grid - 1) // self.grid for t in self.first]
        self.min_per_wg, self.max_per_wg = min(counts), max(counts)

    def tile(self, n, **d):
        t = n
        for name, c in reversed(self.digits):
            t = t * c + d[name]
        return t

    def where(self, t):
        """(workgroup, iteration i) that computes tile t"""
        return self.owner_of[t % self.grid], t // self.grid

    def decode(self, t):
        d = {}
        for name, c in self.digits:
            d[name] = t % c
            t //= c
        return t, d

    def states_reached(self):
        """the carried states at tile starts that every workgroup goes through"""
        return {self.state(k) for k in range(self.min_per_wg)}

    def check_coverage(self, min_per_wg, states=None, ragged=False):
        assert self.min_per_wg >= min_per_wg, (self.kernel, self.ntiles, self.min_per_wg, min_per_wg)
        if states is not None:
            assert len(self.states_reached()) == states, (self.kernel, sorted(self.states_reached()), states)
        if ragged:    # some workgroups take one tile more: the last tile's nvalid = false beside workgroups still going
            assert self.ntiles % GRID_MAX != 0 and self.max_per_wg == self.min_per_wg + 1
        return self

    def images(self):
        """first, middle and last image; they start on different tile iterations"""
        sel = [0, self.n // 2, self.n - 1]
        starts = [n * self.per_image // self.grid for n in sel]
        assert len(set(starts)) == 3, (sel, starts)
        assert (self.n * self.per_image - 1) // self.grid == self.max_per_wg - 1      # the last image reaches the last iteration
        return sel

    def describe(self, n, d):
        t = self.tile(n, **d)
        b, i = self.where(t)
        return (f'worst tile (n={n}, ' + ', '.join(f'{k}={d[k]}' for k, _ in reversed(self.digits)) +
                f') = tile {t} of {self.ntiles}: workgroup {b} (first tile {self.first[b]}), iteration i={i} of grid {self.grid}')


def fwd_tiling(n, ci, co, h, w):
    """conv_x3_fwd_kernel (ci, co: the GEMM roles - contracted and output channels).  Carried: ring slot r0 = k ndc mod 3,
    weight-buffer parity = k * 9 ndc mod 2 (ndc = ci / 64 double chunks of 9 weight stages per tile)."""
    ndc = ci // 64
    t = Tiling('conv_x3_fwd_kernel', n, [('co_t', co // 64), ('tx', w // 16), ('ty', h // 16)],
               lambda k: (k * ndc % 3, k * 9 * ndc % 2))
    t.tile_of = lambda nn, c, y, x: (nn, dict(co_t=c // 64, tx=x // 16, ty=y // 16))
    return t


def up_tiling(n, ci, co, hl, wl):
    """conv_x3_up_kernel: output (n, co, 2hl, 2wl), tiles of 8 x 16 low-resolution pixels x 64 channels x one row parity py
    (the 32-channel form: 32 channels, both parities).  Carried: ring slot = k * ci / 16 halves mod 3; the weight parity
    restarts every tile (ci / 8 k-steps, a multiple of 8); the row parity of the next tile (the wrap's patch offset)."""
    c32 = co % 64 != 0
    digits = [('co_t', co // 32)] if c32 else [('co_t', co // 64), ('py', 2)]
    t = Tiling('conv_x3_up_kernel', n, digits + [('tx', wl // 16), ('ty', hl // 8)], lambda k: (k * (ci // 16) % 3,))
    if c32:
        t.tile_of = lambda nn, c, y, x: (nn, dict(co_t=c // 32, tx=(x // 2) // 16, ty=(y // 2) // 8))
    else:
        t.tile_of = lambda nn, c, y, x: (nn, dict(co_t=c // 64, py=y & 1, tx=(x // 2) // 16, ty=(y // 2) // 8))
    return t


def down_tiling(n, ci, co, hl, wl):
    """conv_x3_down_kernel: output (n, co, hl, wl), tiles of 8 x 16 pixels x 128 channels.  Carried: ring slot = k * ci / 8
    quarters mod 3; the weight parity restarts every tile (ci / 2 k-steps)."""
    t = Tiling('conv_x3_down_kernel', n, [('co_t', co // 128), ('tx', wl // 16), ('ty', hl // 8)],
               lambda k: (k * (ci // 8) % 3,))
    t.tile_of = lambda nn, c, y, x: (nn, dict(co_t=c // 128, tx=x // 16, ty=y // 8))
    return t


# ---- running and comparing ----------------------------------------------------------------------------------------------------
def run_x3_and_exact(ops, tl, fn):
    """fn() on the split-product kernel (asserted: tl.kernel with grid tl.grid) and on the exact-fp32 kernels"""
    from gan_lab_amd import _lib
    c0 = _lib.launch_count()
    a = fn()
    seen = [(k or '', g) for k, g in _lib.launches_since(c0)]
    hits = [g for k, g in seen if tl.kernel in k]
    assert hits == [tl.grid], (tl.kernel, tl.grid, seen)
    prev = ops.set_x3(False)
    try:
        c0 = _lib.launch_count()
        b = fn()
        assert not any(tl.kernel in (k or '') for k, _ in _lib.launches_since(c0))
    finally:
        ops.set_x3(prev)
    return a, b


def close(got, ref, what, tl, images=None):
    """assert_close of test_gpu_x3 (max |got - ref| / max |ref| <= TOL); on failure, the worst element's tile and workgroup.
    ``images``: the image indices of got / ref's first axis (None: all)."""
    got, ref = got.double(), ref.to(got.device).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = (got - ref).abs()
    e = d.max().item() / max(ref.abs().max().item(), 1e-30)
    if not e <= TOL:
        idx = [int(v) for v in torch.unravel_index(d.argmax(), d.shape)]
        n = images[idx[0]] if images is not None else idx[0]
        where = tl.describe(*tl.tile_of(n, *idx[1:])) if len(idx) == 4 else f'(n, c) = ({n}, {idx[1]})'
        bad = int((d > TOL * ref.abs().max()).sum())
        raise AssertionError(f'{what}: rel err {e:.3e} > {TOL:.1e} ({bad} elements over); {where}')
    return e


def rms_bar(y3, y1, yd, what):
    """'fp32' = no further from float64 than the exact-fp32 kernels (rms over the selected images)"""
    e3, e1 = rms_rel(y3, yd), rms_rel(y1, yd)
    assert e3 <= 1.1 * e1, (what, e3, e1)
    return e3, e1


def cpu(t, sel):
    return t[sel].cpu()


def rand(shape, gen):
    return torch.randn(*shape, device='cuda', generator=gen)


# ---- conv_x3_fwd_kernel: forward, input gradient ---------------------------------------------------------------------------------
# N, Cin, Cout, H, W; the comment gives (tiles, tiles per workgroup) of the forward / input gradient and the carried states
# (ring slot r0, weight parity) their workgroups start tiles in
FWD_CASES = [
    (6, 64, 64, 256, 256),       # 1536, 6 / 1536, 6: ndc = 1, all 6 (r0, parity) pairs
    (100, 64, 64, 64, 64),       # 1600, 6-7 ragged / the same: all 6 pairs, the last tile's nvalid = false beside live ones
    (12, 128, 128, 128, 128),    # 1536, 6 / 1536, 6: ndc = 2, two co tiles: r0 = 2k mod 3 (3 states), parity fixed
    (12, 192, 64, 128, 128),     # 768, 3: ndc = 3, r0 fixed, parity alternates (2 states) / 2304, 9: ndc = 1, all 6
]
FWD_STATES = {1: 6, 2: 3, 3: 2}     # ndc -> carried states of its period


@pytest.mark.parametrize('case', FWD_CASES)
@pytest.mark.parametrize('role', ['fwd', 'dgrad'])
def test_x3_persistent_forward_and_input_gradient(ops, case, role):
    n, ci, co, h, w = case
    dgrad = role == 'dgrad'
    tl = fwd_tiling(n, co, ci, h, w) if dgrad else fwd_tiling(n, ci, co, h, w)
    ndc = (co if dgrad else ci) // 64
    tl.check_coverage(min_per_wg=3 if ndc == 3 else 6, states=FWD_STATES[ndc], ragged=n == 100)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(101 + n + ci + co + dgrad)
    wt = rand((co, ci, 3, 3), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1)
    assert ops.x3_ok(geom, dgrad)
    scale = 1.0 / (3 * ci ** 0.5)
    wd = wt.double().cpu() * scale
    if dgrad:
        gy = rand((n, co, h, w), g)
        a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_dgrad(gy, wt, geom, scale))
        xd = torch.zeros(len(sel), ci, h, w, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(F.conv2d(xd, wd, padding=1), xd, cpu(gy, sel).double())
    else:
        x, bias = rand((n, ci, h, w), g), rand((co,), g)
        a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_fwd(x, wt, bias, geom, scale, 0.5, ops.ACT_LRELU, 0.2))
        ref = F.leaky_relu(F.conv2d(cpu(x, sel).double(), wd, None, padding=1) + 0.5 * bias.double().cpu().view(1, -1, 1, 1), 0.2)
    close(a, b, f'x3 {role} vs exact-fp32 kernel', tl)
    close(cpu(a, sel), ref, f'x3 {role} vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, role)
    print(f'SUMMARY x3 persistent {role} {case}: {tl.ntiles} tiles, {tl.min_per_wg}-{tl.max_per_wg} per workgroup, '
          f'states {sorted(tl.states_reached())}')


def test_x3_persistent_headline_forward(ops):
    """The headline step's 64 -> 64 @256^2 layer at batch 32: 8192 tiles, 32 per workgroup (profiles/r05b_x3_bench.txt once
    recorded max |diff| 4.41 against the exact kernel here)."""
    n, ci, co, h, w = 32, 64, 64, 256, 256
    tl = fwd_tiling(n, ci, co, h, w).check_coverage(min_per_wg=32, states=6)
    assert tl.max_per_wg == 32
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(17)
    x, wt, bias = rand((n, ci, h, w), g), rand((co, ci, 3, 3), g), rand((co,), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1)
    scale = 1.0 / (3 * ci ** 0.5)
    assert ops.x3_ok(geom)
    a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_fwd(x, wt, bias, geom, scale, 0.5, ops.ACT_LRELU, 0.2))
    diff = (a - b).abs().max().item()
    close(a, b, 'x3 headline forward vs exact-fp32 kernel', tl)
    ref = F.leaky_relu(F.conv2d(cpu(x, sel).double(), wt.double().cpu() * scale, None, padding=1) +
                       0.5 * bias.double().cpu().view(1, -1, 1, 1), 0.2)
    close(cpu(a, sel), ref, 'x3 headline forward vs float64', tl, sel)
    e3, e1 = rms_bar(cpu(a, sel), cpu(b, sel), ref, 'headline forward')
    print(f'SUMMARY x3 headline 64->64 @256 x32: {tl.ntiles} tiles, {tl.min_per_wg} per workgroup; max |x3 - exact| {diff:.3e} '
          f'(max |y| {b.abs().max().item():.2f}); rms vs float64: x3 {e3:.3e}, exact {e1:.3e}')


# ---- conv_x3_fwd_kernel: the masked input gradient, the affine-on-load forward and the whole layer tail -----------------------------
MULTI = (6, 64, 64, 256, 256)     # 1536 tiles, 6 per workgroup, ndc = 1: all 6 (r0, parity) pairs


def test_x3_persistent_masked_input_gradient(ops):
    n, ci, co, h, w = MULTI
    tl = fwd_tiling(n, co, ci, h, w).check_coverage(min_per_wg=6, states=6)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(23)
    x = F.leaky_relu(rand((n, ci, h, w), g), 0.2)
    wt, gy = rand((co, ci, 3, 3), g), rand((n, co, h, w), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1)
    a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_dgrad_mask(gy, wt, x, geom, 0.03, 0.2))
    close(a, b, 'x3 masked input gradient vs exact-fp32 kernel', tl)
    xd = torch.zeros(len(sel), ci, h, w, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(F.conv2d(xd, wt.double().cpu() * 0.03, padding=1), xd, cpu(gy, sel).double())
    ref = ref * torch.where(cpu(x, sel) > 0, 1.0, 0.2).double()
    close(cpu(a, sel), ref, 'x3 masked input gradient vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, 'masked input gradient')


def test_x3_persistent_affine_forward(ops):
    n, ci, co, h, w = MULTI
    tl = fwd_tiling(n, ci, co, h, w).check_coverage(min_per_wg=6, states=6)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(29)
    a_, wt = rand((n, ci, h, w), g), rand((co, ci, 3, 3), g)
    s_ = torch.rand(n, ci, device='cuda', generator=g) + 0.5
    t_ = rand((n, ci), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1)
    a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_fwd_aff(a_, s_, t_, wt, geom, 0.02))
    close(a, b, 'x3 affine-on-load forward vs exact-fp32 kernel', tl)
    bd = cpu(a_, sel).double() * cpu(s_, sel).double().view(-1, ci, 1, 1) + cpu(t_, sel).double().view(-1, ci, 1, 1)
    ref = F.conv2d(bd, wt.double().cpu() * 0.02, None, padding=1)
    close(cpu(a, sel), ref, 'x3 affine-on-load forward vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, 'affine forward')


def test_x3_persistent_affine_layer_tail(ops):
    """y = lrelu(conv(a*s + t) + noise_w * noise + bias) and the InstanceNorm statistics of y from the epilogue's per-tile
    partial sums: a workgroup writes the partials of six different tiles."""
    from gan_lab_amd import _lib
    n, ci, co, h, w = MULTI
    tl = fwd_tiling(n, ci, co, h, w).check_coverage(min_per_wg=6, states=6)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(31)
    a_, wt, bias = rand((n, ci, h, w), g), rand((co, ci, 3, 3), g), rand((co,), g)
    s_ = torch.rand(n, ci, device='cuda', generator=g) + 0.5
    t_ = rand((n, ci), g)
    nz, nw = rand((n, 1, h, w), g), rand((co,), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1)
    scale, eps = 0.02, 1e-8
    L = _lib.lib()
    p = lambda v: ctypes.c_void_p(v.data_ptr())

    def tail():
        y = torch.empty(n, co, h, w, device='cuda')
        mean, rstd = torch.empty(n, co, device='cuda'), torch.empty(n, co, device='cuda')
        if ops.x3_enabled():
            chunks = L.ganlab_conv_fwd_aff_tail_x3_chunks(geom.ref())
            assert chunks == (h // 16) * (w // 16) * 4
            ws = torch.empty(n * co * chunks * 2, dtype=torch.float64, device='cuda')
            _lib.check(L.ganlab_conv_fwd_aff_tail_x3(p(a_), p(ops._packed_x3(wt, ops.PACK_FWD, scale)), p(s_), p(t_), p(bias), p(nz),
                                                     p(nw), p(y), p(mean), p(rstd), geom.ref(), 0.7, ops.ACT_LRELU, 0.2, eps, p(ws),
                                                     ws.numel() * 8, None), 'tail x3')
        else:
            chunks = L.ganlab_conv_fwd_aff_tail_chunks(geom.ref())
            assert chunks > 0
            ws = torch.empty(n * co * chunks * 2, dtype=torch.float64, device='cuda')
            _lib.check(L.ganlab_conv_fwd_aff_tail_f32(p(a_), p(ops._packed(wt, ops.PACK_FWD, scale)), p(s_), p(t_), p(bias), p(nz),
                                                      p(nw), p(y), p(mean), p(rstd), geom.ref(), 0.7, ops.ACT_LRELU, 0.2, eps,
                                                      p(ws), ws.numel() * 8, None), 'tail exact')
        return torch.cat([y.flatten(), mean.flatten(), rstd.flatten()])

    def split(v):
        k = n * co * h * w
        return v[:k].view(n, co, h, w), v[k:k + n * co].view(n, co), v[k + n * co:].view(n, co)

    (y3, m3, r3), (y1, m1, r1) = (split(v) for v in run_x3_and_exact(ops, tl, tail))
    close(y3, y1, 'x3 layer tail vs exact-fp32 kernel', tl)
    close(m3, m1, 'x3 layer tail: mean vs exact-fp32 kernel (every image)', tl)
    close(r3, r1, 'x3 layer tail: rstd vs exact-fp32 kernel (every image)', tl)
    bd = cpu(a_, sel).double() * cpu(s_, sel).double().view(-1, ci, 1, 1) + cpu(t_, sel).double().view(-1, ci, 1, 1)
    pre = F.conv2d(bd, wt.double().cpu() * scale, None, padding=1) + 0.7 * bias.double().cpu().view(1, -1, 1, 1) + \
        nw.double().cpu().view(1, -1, 1, 1) * cpu(nz, sel).double()
    yd = F.leaky_relu(pre, 0.2)
    md = yd.mean(dim=(2, 3))
    rd = 1.0 / torch.sqrt(yd.var(dim=(2, 3), unbiased=False) + eps)
    close(cpu(y3, sel), yd, 'x3 layer tail vs float64', tl, sel)
    close(cpu(m3, sel), md, 'x3 layer tail: mean vs float64', tl, sel)
    close(cpu(r3, sel), rd, 'x3 layer tail: rstd vs float64', tl, sel)
    rms_bar(cpu(y3, sel), cpu(y1, sel), yd, 'layer tail')


# ---- conv_x3_up_kernel: an up layer's forward (+ affine on load), the 32-channel form, a pooled layer's input gradient -----------
# N, Cin, Cout, Hl, Wl of the up layer (input hl x wl, output 2hl x 2wl)
UP_CASES = [
    (24, 64, 64, 64, 64),        # 1536 tiles, 6 per workgroup: ring slots 0, 1, 2 (4 halves per tile)
    (25, 64, 64, 64, 64),        # 1600, 6-7 ragged
    (8, 64, 192, 64, 64),        # 1536, 6: 3 co tiles, so a workgroup's next tile can have the other row parity (the wrap's offset)
    (48, 64, 32, 64, 64),        # 1536, 6: the 32-channel form (both row parities in one workgroup)
]


def _py_changes(tl):
    """does some workgroup go on to a tile of the other row parity?"""
    def py(t):
        return tl.decode(t)[1].get('py', 0)
    return any(py(t) != py(t + tl.grid) for t in range(tl.ntiles - tl.grid))


@pytest.mark.parametrize('case', UP_CASES)
@pytest.mark.parametrize('aff', [False, True])
def test_x3_persistent_up_layer_forward(ops, case, aff):
    n, ci, co, hl, wl = case
    tl = up_tiling(n, ci, co, hl, wl).check_coverage(min_per_wg=6, states=3, ragged=n == 25)
    assert _py_changes(tl) == (co == 192)          # (256 tiles on: same parity whenever the co tiles divide 128)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(41 + n + co + aff)
    x, wt, bias = rand((n, ci, hl, wl), g), rand((co, ci, 3, 3), g), rand((co,), g)
    s_ = torch.rand(n, ci, device='cuda', generator=g) + 0.5
    t_ = rand((n, ci), g)
    geom = ops.Geom(n, ci, hl, wl, co, 3, 1, up=1)
    assert ops.x3_s2_ok(geom)
    scale = 1.0 / (3 * ci ** 0.5)
    xs = cpu(x, sel).double()
    if aff:
        a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_fwd_aff(x, s_, t_, wt, geom, scale))
        xs = xs * cpu(s_, sel).double().view(-1, ci, 1, 1) + cpu(t_, sel).double().view(-1, ci, 1, 1)
        ref = F.conv2d(F.interpolate(xs, scale_factor=2, mode='nearest'), wt.double().cpu() * scale, None, padding=1)
    else:
        a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_fwd(x, wt, bias, geom, scale, 0.5, ops.ACT_LRELU, 0.2))
        ref = F.leaky_relu(F.conv2d(F.interpolate(xs, scale_factor=2, mode='nearest'), wt.double().cpu() * scale, None, padding=1) +
                           0.5 * bias.double().cpu().view(1, -1, 1, 1), 0.2)
    what = 'x3 up layer' + (', affine on load' if aff else '')
    close(a, b, what + ' vs exact-fp32 kernel', tl)
    close(cpu(a, sel), ref, what + ' vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, what)


# N, Cin, Cout, H, W of the pooled layer (input h x w, output h/2 x w/2); its input gradient runs the up kernel with the roles
# swapped: Cout contracted, Cin out
POOL_DGRAD_CASES = [
    (24, 64, 64, 128, 128),      # 1536 tiles, 6 per workgroup: ring slots 0, 1, 2
    (25, 64, 64, 128, 128),      # 1600, 6-7 ragged
    (48, 32, 64, 128, 128),      # 1536, 6: 32 channels out - the 32-channel form
]


@pytest.mark.parametrize('case', POOL_DGRAD_CASES)
def test_x3_persistent_pooled_layer_input_gradient(ops, case):
    n, ci, co, h, w = case
    tl = up_tiling(n, co, ci, h // 2, w // 2).check_coverage(min_per_wg=6, states=3, ragged=n == 25)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(43 + n + ci)
    wt, gy = rand((co, ci, 3, 3), g), rand((n, co, h // 2, w // 2), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1, pool=1)
    assert ops.x3_s2_ok(geom, True)
    scale = 1.0 / (3 * ci ** 0.5)
    a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_dgrad(gy, wt, geom, scale))
    close(a, b, 'x3 pooled layer input gradient vs exact-fp32 kernel', tl)
    xd = torch.zeros(len(sel), ci, h, w, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(F.avg_pool2d(F.conv2d(xd, wt.double().cpu() * scale, padding=1), 2), xd, cpu(gy, sel).double())
    close(cpu(a, sel), ref, 'x3 pooled layer input gradient vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, 'pooled layer input gradient')


# ---- conv_x3_down_kernel: a pooled layer's forward, an up layer's input gradient ------------------------------------------------
# N, Cin, Cout, H, W of the pooled layer (output h/2 x w/2)
POOL_FWD_CASES = [
    (24, 64, 256, 128, 128),     # 1536 tiles, 6 per workgroup, 2 co tiles: ring slot 8k mod 3 - all three
    (50, 32, 128, 128, 128),     # 1600, 6-7 ragged: 4 quarters per tile, ring slot k mod 3
]


@pytest.mark.parametrize('case', POOL_FWD_CASES)
def test_x3_persistent_pooled_layer_forward(ops, case):
    n, ci, co, h, w = case
    tl = down_tiling(n, ci, co, h // 2, w // 2).check_coverage(min_per_wg=6, states=3, ragged=n == 50)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(47 + n + ci)
    x, wt, bias = rand((n, ci, h, w), g), rand((co, ci, 3, 3), g), rand((co,), g)
    geom = ops.Geom(n, ci, h, w, co, 3, 1, pool=1)
    assert ops.x3_s2_down_ok(geom)
    scale = 1.0 / (3 * ci ** 0.5)
    a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_fwd(x, wt, bias, geom, scale, 0.5, ops.ACT_LRELU, 0.2))
    close(a, b, 'x3 pooled layer forward vs exact-fp32 kernel', tl)
    ref = F.leaky_relu(F.avg_pool2d(F.conv2d(cpu(x, sel).double(), wt.double().cpu() * scale, None, padding=1), 2) +
                       0.5 * bias.double().cpu().view(1, -1, 1, 1), 0.2)
    close(cpu(a, sel), ref, 'x3 pooled layer forward vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, 'pooled layer forward')


# N, Cin, Cout, Hl, Wl of the up layer; its input gradient contracts Cout and writes Cin channels at hl x wl
UP_DGRAD_CASES = [
    (24, 256, 64, 64, 64),       # 1536 tiles, 6 per workgroup, 2 co tiles: ring slot 8k mod 3
    (50, 128, 32, 64, 64),       # 1600, 6-7 ragged: 4 quarters per tile, ring slot k mod 3
]


@pytest.mark.parametrize('case', UP_DGRAD_CASES)
def test_x3_persistent_up_layer_input_gradient(ops, case):
    n, ci, co, hl, wl = case
    tl = down_tiling(n, co, ci, hl, wl).check_coverage(min_per_wg=6, states=3, ragged=n == 50)
    sel = tl.images()
    g = torch.Generator(device='cuda').manual_seed(53 + n + ci)
    wt, gy = rand((co, ci, 3, 3), g), rand((n, co, 2 * hl, 2 * wl), g)
    geom = ops.Geom(n, ci, hl, wl, co, 3, 1, up=1)
    assert ops.x3_s2_down_ok(geom, True)
    scale = 1.0 / (3 * ci ** 0.5)
    a, b = run_x3_and_exact(ops, tl, lambda: ops.k_conv_dgrad(gy, wt, geom, scale))
    close(a, b, 'x3 up layer input gradient vs exact-fp32 kernel', tl)
    xd = torch.zeros(len(sel), ci, hl, wl, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(F.conv2d(F.interpolate(xd, scale_factor=2, mode='nearest'), wt.double().cpu() * scale, padding=1), xd,
                               cpu(gy, sel).double())
    close(cpu(a, sel), ref, 'x3 up layer input gradient vs float64', tl, sel)
    rms_bar(cpu(a, sel), cpu(b, sel), ref, 'up layer input gradient')


# ---- the weight gradients at steady-state strip counts --------------------------------------------------------------------------
def wgrad_plan(pairs, nstrips):
    """xw_plan / xs_plan: (k-splits, strips per split) for `pairs` channel-tile pairs"""
    splits = min((512 + pairs - 1) // pairs, nstrips)
    splits = max(splits, 1)
    sps = (nstrips + splits - 1) // splits
    return (nstrips + sps - 1) // sps, sps


def strip_ranges(splits, sps, nstrips, strips_x):
    """per split: the images its strips come from"""
    return [sorted({s // strips_x for s in range(k * sps, min((k + 1) * sps, nstrips))}) for k in range(splits)]


@pytest.mark.parametrize('aff', [False, True])
def test_x3_weight_gradient_several_strips_per_split(ops, aff):
    """512 -> 512 channels: 128 channel-tile pairs leave 4 k-splits; 5 images x 3 strips of 32 columns = 15 strips, 4 per split,
    so splits run their strip loop four times and splits 0-2 cross an image boundary (the affine's per-image reload)."""
    from gan_lab_amd import _lib
    n, ci, co, h, w = 5, 512, 512, 4, 96
    pairs, strips_x = (co // 32) * (ci // 64), w // 32          # XW_CO = 32, XW_CI = 64
    splits, sps = wgrad_plan(pairs, n * strips_x)
    assert (splits, sps) == (4, 4)
    ranges = strip_ranges(splits, sps, n * strips_x, strips_x)
    assert sum(len(r) > 1 for r in ranges) == 3, ranges
    geom = ops.Geom(n, ci, h, w, co, 3, 1)
    assert ops.x3_wgrad_ok(geom)
    assert _lib.lib().ganlab_conv_wgrad_x3_workspace(geom.ref()) == splits * co * ci * 9 * 4
    g = torch.Generator(device='cuda').manual_seed(59 + aff)
    x, gy = rand((n, ci, h, w), g), rand((n, co, h, w), g)
    s_ = torch.rand(n, ci, device='cuda', generator=g) + 0.5
    t_ = rand((n, ci), g)
    scale = 0.013
    run = (lambda: ops.k_conv_wgrad_aff(gy, x, s_, t_, geom, scale)) if aff else (lambda: ops.k_conv_wgrad(gy, x, geom, scale))
    c0 = _lib.launch_count()
    gw3 = run()
    seen = [(k or '', grid) for k, grid in _lib.launches_since(c0)]
    assert [grid for k, grid in seen if 'conv_x3_wgrad_kernel' in k] == [pairs * splits], seen
    prev = ops.set_x3(False)
    try:
        # (the exact-fp32 affine-on-load weight gradient does not take every geometry: then the materialised operand)
        if aff and not ops.conv_aff_ok((n, ci, h, w), torch.empty(co, ci, 3, 3)):
            gw1 = ops.k_conv_wgrad(gy, x * s_.view(n, ci, 1, 1) + t_.view(n, ci, 1, 1), geom, scale)
        else:
            gw1 = run()
        assert 'x3w_reduce_kernel' not in (_lib.last_launch()[0] or '')
    finally:
        ops.set_x3(prev)
    xin = x.double().cpu()
    if aff:
        xin = xin * s_.double().cpu().view(n, ci, 1, 1) + t_.double().cpu().view(n, ci, 1, 1)
    wd = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    gwd, = torch.autograd.grad(F.conv2d(xin, wd, padding=1), wd, gy.double().cpu())
    gwd = gwd * scale
    assert_close(gw3.cpu(), gwd, TOL, 'x3 weight gradient (4 strips per split) vs float64')
    assert_close(gw3.cpu(), gw1.cpu(), TOL, 'x3 weight gradient (4 strips per split) vs exact-fp32 kernel')
    assert rms_rel(gw3, gwd) <= max(1.1 * rms_rel(gw1, gwd), 2.5e-7), (rms_rel(gw3, gwd), rms_rel(gw1, gwd))


@pytest.mark.parametrize('kind', ['pool', 'up'])
def test_x3_stride2_weight_gradient_several_strips_per_split(ops, kind):
    """512 low-resolution x 512 high-resolution channels: 128 pairs, 4 k-splits; 5 images x 3 strips = 15 strips, 4 per split,
    splits 0-2 crossing an image boundary."""
    from gan_lab_amd import _lib
    up = kind == 'up'
    n, cl, cb, hl, wl = 5, 512, 512, 4, 96
    pairs, strips_x = (cl // 64) * (cb // 32), (wl + 31) // 32      # XS_CL = 64, XS_CB = 32
    splits, sps = wgrad_plan(pairs, n * strips_x)
    assert (splits, sps) == (4, 4)
    ranges = strip_ranges(splits, sps, n * strips_x, strips_x)
    assert sum(len(r) > 1 for r in ranges) == 3, ranges
    if up:      # the up layer: cl -> cb channels, input hl x wl
        ci, co, hi, wi = cl, cb, hl, wl
        geom = ops.Geom(n, ci, hi, wi, co, 3, 1, up=1)
    else:       # the pooled layer: cb -> cl channels, input 2hl x 2wl
        ci, co, hi, wi = cb, cl, 2 * hl, 2 * wl
        geom = ops.Geom(n, ci, hi, wi, co, 3, 1, pool=1)
    assert ops.x3_s2_wgrad_ok(geom)
    assert _lib.lib().ganlab_conv_s2_wgrad_x3_workspace(geom.ref()) == pairs * splits * 64 * 32 * 9 * 4
    g = torch.Generator(device='cuda').manual_seed(61 + up)
    x = rand((n, ci, hi, wi), g)
    gy = rand((n, co, 2 * hl, 2 * wl), g) if up else rand((n, co, hl, wl), g)
    scale = 0.017
    c0 = _lib.launch_count()
    gw3 = ops.k_conv_wgrad(gy, x, geom, scale)
    seen = [(k or '', grid) for k, grid in _lib.launches_since(c0)]
    assert [grid for k, grid in seen if 'conv_x3_s2_wgrad_kernel' in k] == [pairs * splits], seen
    prev = ops.set_x3(False)
    try:
        gw1 = ops.k_conv_wgrad(gy, x, geom, scale)
        assert 'x3sw_reduce_kernel' not in (_lib.last_launch()[0] or '')
    finally:
        ops.set_x3(prev)
    wd = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    xd = x.double().cpu()
    yd = F.conv2d(F.interpolate(xd, scale_factor=2, mode='nearest'), wd, padding=1) if up else \
        F.avg_pool2d(F.conv2d(xd, wd, padding=1), 2)
    gwd, = torch.autograd.grad(yd, wd, gy.double().cpu())
    gwd = gwd * scale
    assert_close(gw3.cpu(), gwd, TOL, 'x3 stride-2 weight gradient (4 strips per split) vs float64')
    assert_close(gw3.cpu(), gw1.cpu(), TOL, 'x3 stride-2 weight gradient (4 strips per split) vs exact-fp32 kernel')
    assert rms_rel(gw3, gwd) <= max(1.1 * rms_rel(gw1, gwd), 2.5e-7), (rms_rel(gw3, gwd), rms_rel(gw1, gwd))
