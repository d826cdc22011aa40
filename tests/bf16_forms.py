"""The bf16-compute convolution kernels by name: one row per kernel per edge (csrc/conv_bf16.hip, BASELINE config #2).

Same shape as tests/exact_forms.py.  A row is a ``Form`` of tests/x3_forms.py (geometry, operands, GPU call) plus
  * ``symbol``: the kernel the call must launch, with its template arguments (compared as ``exact_forms.norm`` does);
  * ``plan``: every launch of the call as (symbol, workgroups) in launch order, from the plain-Python restatements below of the
    launcher code - ``bf16_ok``, ``bf16_wgrad_ok``, ``bf16_splitk_plan``, ``launch_fwd``'s tile choice and grid, ``wr_plan``,
    ``wgrad_slots``, the two reduce grids and the split-K finish grid.  Nothing of it is imported from the library;
  * ``facts``: what the restated plan says about the row's geometry, and ``edge``: a predicate over ``facts`` that says what the
    row is for (``why`` says it in words), so that tests/test_bf16_forms_host.py proves without a GPU that the row reaches it;
  * ``restate``: the operation in float64 from explicit shifted sums, and ``define``: the ``torch.autograd`` definition - in
    float64 it guards ``restate``, in fp32 on the CPU it is the ATen yardstick of tests/test_gpu_bf16_kernels.py.
The kernels round their operands to bf16 (round to nearest even) on the way into LDS and multiply exactly, so every reference
takes ROUNDED operands: ``round_operands`` rounds x and gy with ``rne_bf16`` and the weight as ``rne_bf16(w * scale)``, the
product taken in fp32 as ``pack_bf16_kernel`` takes it.  The references then use the weight as it is.
Shapes are (N, Cin, Cout, H, W) of the layer - of a stride-2 layer its LOW resolution; the 3x3 taps of an up / pooled layer run
at (2H, 2W).  Out of reach of a float64 reference in seconds, and so not in this table: config #2's own layer sizes
(tests/test_gpu_bf16.py test_bf16_full_size_triple_product keeps those).  Nothing here asserts a bar."""
import collections

import torch
import torch.nn.functional as F

import x3_forms as X
from exact_forms import cdiv, norm, plan_found, r_box, r_conv, r_lrelu, r_up2
from x3_forms import BIAS_SCALE, SLOPE

CK, COT, RW_T, WG_CI, WTH, STRIP = 32, 64, 64, 32, 4, 32     # the constants of conv_bf16.hip
PACK_FWD, PACK_DGRAD = 0, 1
FP32_MAX = 3.4028234663852886e38            # finite in fp32, inf once rounded to bf16
TOL_FWD, TOL_GRAD = 2e-5, 5e-5              # tests/test_gpu_bf16.py's bars against float64 on the rounded operands


# ==== rounding =======================================================================================================================
def rne_bf16(t):
    """fp32 -> bf16 -> fp32, round to nearest even, in integer arithmetic on the bit pattern: add 0x7fff and the lowest kept bit,
    drop the low 16 bits.  The carry runs into the exponent, so the values above bf16's maximum become inf and subnormals need
    no case of their own.  NaN stays NaN (quiet, sign kept)."""
    assert t.dtype == torch.float32
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = torch.where(nan, (u | 0x00400000) & 0xFFFF0000, r)
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r)
    return r.to(torch.int32).view(torch.float32).view(t.shape)


def from_bits(u):
    """fp32 tensor of the given bit patterns (any integers below 2^32)"""
    u = torch.as_tensor(u, dtype=torch.int64)
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def trunc_bf16(t):
    """the mistake: the low 16 bits dropped without rounding"""
    u = t.contiguous().view(torch.int32) & -65536
    return u.view(torch.float32).view(t.shape)


def bf16_bits(t):
    """the 16 bits of a bf16-representable fp32 tensor, as int16"""
    return (t.contiguous().view(torch.int32) >> 16).to(torch.int16)


def round_operands(f, T, rne=rne_bf16, scale_first=True):
    """The operands as the kernels see them (fp32 tensors holding bf16 numbers); the bias is not rounded."""
    d = {}
    for k in T._fields:
        v = getattr(T, k)
        if k in ('x', 'gy'):
            v = rne(v)
        elif k == 'wt':
            v = rne(v * f.scale) if scale_first else rne(v) * f.scale
        d[k] = v
    return T._replace(**d)


# ==== the launchers' plans, restated =================================================================================================
def taps_of(kind, h, w):
    return (h, w) if kind == 'plain' else (2 * h, 2 * w)


def bf16_ok(n, ci, co, hin, win, up=0, pool=0, ks=3, pad=1):
    if ks != 3 or pad != 1 or (up and pool) or min(n, ci, co, hin, win) <= 0 or ci % 64 or co % 64:
        return False
    m = 2 if up else 1
    h, w = hin * m, win * m
    if not ((h % 8 == 0 and w % 32 == 0) or (h % 16 == 0 and w % 16 == 0)):
        return False
    return ci * h * w * 4 < 2 ** 31 and co * h * w * 4 < 2 ** 31


def bf16_wgrad_ok(n, ci, co, hin, win, up=0, pool=0, roll=True):
    if not bf16_ok(n, ci, co, hin, win, up, pool):
        return False
    m = 2 if up else 1
    return (hin * m) % 8 == 0 and (win * m) % 32 == 0 and (not (up or pool) or roll)


def bf16_splitk_plan(n, CI, CO, H, W):
    wide = W % 32 == 0 and H % 8 == 0
    tiles = n * ((W // 32) * (H // 8) if wide else (W // 16) * (H // 16)) * (CO // COT)
    chunks = CI // CK
    if tiles >= 128 or chunks < 8:
        return 1
    s = min(cdiv(256, tiles), 4)
    while s > 1 and chunks // s < 4:
        s -= 1
    return 1 if s < 2 else s


def split_sizes(chunks, s):
    """chunks of each K split: ks_chunks = ceil(chunks / S), the last one takes what is left"""
    k = cdiv(chunks, s)
    return [min(chunks, (i + 1) * k) - i * k for i in range(s)]


MODE = {('fwd', 'plain'): 0, ('fwd', 'up'): 1, ('fwd', 'pool'): 2, ('dgrad', 'plain'): 0, ('dgrad', 'up'): 2, ('dgrad', 'pool'): 1}


def fwd_facts(role, kind, n, ci, co, h, w):
    """launch_fwd as the forward (role 'fwd') or the input gradient ('dgrad') of a layer: mode 1 = UP (the streamed operand is
    stored at half the taps' resolution), 2 = POOL (the result is)."""
    H, W = taps_of(kind, h, w)
    CI, CO = (ci, co) if role == 'fwd' else (co, ci)
    mode = MODE[role, kind]
    wide = W % 32 == 0 and H % 8 == 0
    th, tw = (8, 32) if wide else (16, 16)
    tiles_x, tiles_y, tiles_co = W // tw, H // th, CO // COT
    tiles = n * tiles_x * tiles_y * tiles_co
    s = bf16_splitk_plan(n, CI, CO, H, W)
    chunks = CI // CK
    sym = 'conv_fwd_bf16_kernel<%d, %d, %s, %s>' % (th, tw, 'true' if mode == 1 else 'false', 'true' if mode == 2 else 'false')
    plan = [(sym, tiles * (s if s > 1 else 1))]
    if s > 1:
        total = n * CO * (H // 2 if mode == 2 else H) * (W // 2 if mode == 2 else W)
        plan.append(('bf16_splitk_finish_kernel', cdiv(total, 256)))
    return dict(H=H, W=W, CI=CI, CO=CO, mode=mode, tile=(th, tw), tiles_x=tiles_x, tiles_y=tiles_y, tiles_co=tiles_co, tiles=tiles,
                S=s, chunks=chunks, splits=split_sizes(chunks, s) if s > 1 else [chunks], plan=plan)


def wr_plan(n, ci, co, H, W):
    """the rolling weight gradient at the taps' resolution H x W"""
    rs = 4
    for d in range(32, 3, -1):
        if H % d == 0:
            rs = d
            break
    segs_y, strips = H // rs, W // 32
    nseg = n * strips * segs_y
    npairs = (co // RW_T) * (ci // RW_T)
    want = max(1, min(cdiv(512, npairs), nseg))
    per = cdiv(nseg, want)
    streams = cdiv(nseg, per)
    return dict(RS=rs, segs_y=segs_y, strips=strips, nseg=nseg, npairs=npairs, tiles_ci=ci // RW_T, tiles_co=co // RW_T,
                streams=streams, flush=(streams + 1) // 2, nloop=cdiv(nseg, streams), pad_steps=(rs + 4) // 3 * 3 - (rs + 2))


def roll_facts(kind, n, ci, co, h, w):
    H, W = taps_of(kind, h, w)
    p = wr_plan(n, ci, co, H, W)
    sym = 'conv_wgrad_bf16_roll_kernel<%s, %s>' % ('true' if kind == 'up' else 'false', 'true' if kind == 'pool' else 'false')
    p.update(H=H, W=W, plan=[(sym, p['npairs'] * p['flush']), ('wgrad_bf16_roll_reduce_kernel', cdiv(p['npairs'] * 4 * 36 * 64, 256))])
    return p


def wgrad_slots(n, ci, co, h, w):
    groups = (co // COT) * (ci // WG_CI)
    ntiles = n * (h // WTH) * (w // STRIP)
    return max(1, min(cdiv(2 * 256, groups), ntiles, 64))


def tile_facts(kind, n, ci, co, h, w):
    """the tile weight gradient (GANLAB_BF16_WGRAD_ROLL=0): plain geometries only - an up / pooled layer's half-resolution
    operand is materialised at the taps' resolution in front of it"""
    H, W = taps_of(kind, h, w)
    slots = wgrad_slots(n, ci, co, H, W)
    return dict(H=H, W=W, slots=slots, ntiles=n * (H // WTH) * (W // STRIP), tiles_co=co // COT, tiles_ci=ci // WG_CI,
                strips=W // STRIP, row_tiles=H // WTH,
                plan=[('conv_wgrad_bf16_kernel', (co // COT) * (ci // WG_CI) * slots), ('wgrad_bf16_reduce_kernel', cdiv(9 * co * ci, 256))])


def geom_args(kind, n, ci, co, h, w):
    """(N, Cin, Hin, Win, Cout, up, pool) of the layer's ganlab_conv_geom"""
    hin, win = (2 * h, 2 * w) if kind == 'pool' else (h, w)
    return n, ci, hin, win, co, int(kind == 'up'), int(kind == 'pool')


# ==== float64 restatements (explicit shifted sums) and definitions (autograd) ========================================================
# T: the ROUNDED operands; T.wt is rne(w * scale).  ``mistake``: a targeted error, for tests/test_bf16_forms_host.py.
def _rows_up(v, shift=0):
    """nearest 2x upsample whose row R is source row (R + shift) >> 1"""
    hs = v.shape[2]
    idx = ((torch.arange(2 * hs) + shift) >> 1).clamp(max=hs - 1)
    return v[:, :, idx].repeat_interleave(2, dim=3)


def r_fwd(f, T, mistake=None):
    x, w = T.x, T.wt
    if mistake == 'drop_last_chunk':            # the last K split stops one chunk early
        x, w = x[:, :-CK], w[:, :-CK]
    y = r_conv(r_up2(x) if f.kind == 'up' else x, w, 1)
    if f.kind == 'pool':
        y = r_box(y) if mistake == 'no_quarter' else r_box(y) / 4
    if f.bias:
        y = y + BIAS_SCALE * T.b.view(1, -1, 1, 1)
    return (r_lrelu(y) if f.act else y),


def r_dgrad(f, T, mistake=None):
    gy, w = T.gy, T.wt
    if mistake == 'drop_last_chunk':
        gy, w = gy[:, :-CK], w[:-CK]
    gv = gy
    if f.kind == 'pool':
        gv = r_up2(gy) if mistake == 'no_quarter' else r_up2(gy) / 4
    gx = r_conv(gv, w.flip(2, 3).transpose(0, 1), 1)
    return (r_box(gx) if f.kind == 'up' else gx),


def _wgrad_sum(gv, xp, cols=None):
    """gw[o][i][ky][kx] = sum gv[n][o][y][x] xp[n][i][y + ky][x + kx]; xp: the input with one pixel of padding"""
    h, wd = gv.shape[2], gv.shape[3]
    gw = torch.empty(gv.shape[1], xp.shape[1], 3, 3, dtype=gv.dtype)
    for ky in range(3):
        for kx in range(3):
            gw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', gv, xp[:, :, ky:ky + h, kx:kx + wd])
    return gw


def r_wgrad(f, T, mistake=None):
    xv = r_up2(T.x) if f.kind == 'up' else T.x
    gv = T.gy
    if f.kind == 'pool':
        gv = r_up2(gv) if mistake == 'no_quarter' else r_up2(gv) / 4
    return _wgrad_sum(gv, F.pad(xv, (1, 1, 1, 1))) * f.scale,


def r_wgrad_by_strips(f, T, halo_wrong_side=False):
    """the same sum strip by strip as the kernels walk it: 32 columns and one halo column each side.  ``halo_wrong_side``: the
    left halo column is the pixel right of the strip - the neighbouring strip's wrong side"""
    xv = r_up2(T.x) if f.kind == 'up' else T.x
    gv = r_up2(T.gy) / 4 if f.kind == 'pool' else T.gy
    xp = F.pad(xv, (1, 1, 1, 1))
    gw = 0
    for ox0 in range(0, gv.shape[3], STRIP):
        xs = xp[:, :, :, ox0:ox0 + STRIP + 2].clone()
        if halo_wrong_side:
            xs[..., 0] = xs[..., STRIP + 1]
        gw = gw + _wgrad_sum(gv[..., ox0:ox0 + STRIP], xs)
    return gw * f.scale,


def r_wgrad_by_segments(f, T, rs, odd_start_row_off_by_one=False):
    """the same sum segment by segment (``rs`` gradient rows each).  ``odd_start_row_off_by_one``: in a segment that starts on an
    odd row of the taps the half-resolution operand is read at source row (R + 1) >> 1"""
    assert f.kind in ('up', 'pool')
    H = 2 * f.shape[3]
    gw = 0
    for r0 in range(0, H, rs):
        shift = 1 if (odd_start_row_off_by_one and r0 % 2) else 0
        xv = _rows_up(T.x, shift) if f.kind == 'up' else T.x
        gv = (_rows_up(T.gy, shift) / 4 if f.kind == 'pool' else T.gy).clone()
        gv[:, :, :r0] = 0
        gv[:, :, r0 + rs:] = 0
        gw = gw + _wgrad_sum(gv, F.pad(xv, (1, 1, 1, 1)))
    return gw * f.scale,


def d_lin(f, x, w):
    if f.kind == 'up':
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    y = F.conv2d(x, w, None, padding=1)
    return F.avg_pool2d(y, 2) if f.kind == 'pool' else y


def d_fwd(f, T):
    y = d_lin(f, T.x, T.wt)
    if f.bias:
        y = y + BIAS_SCALE * T.b.view(1, -1, 1, 1)
    return (F.leaky_relu(y, SLOPE) if f.act else y),


def d_dgrad(f, T):
    xd = torch.zeros(f.n, f.ci, *f.hw_in, dtype=T.gy.dtype, requires_grad=True)
    return torch.autograd.grad(d_lin(f, xd, T.wt), xd, T.gy)[0],


def d_wgrad(f, T):
    wd = torch.zeros(f.co, f.ci, 3, 3, dtype=T.gy.dtype, requires_grad=True)
    return torch.autograd.grad(d_lin(f, T.x, wd), wd, T.gy)[0] * f.scale,


def pack_layout(wq, mode, flip=True):
    """pack_bf16_kernel's layout [chunk = ci / 32][tap][kg = (ci % 32) / 8][CO][ci % 8] of the rounded weight ``wq``
    (Cout, Cin, 3, 3).  PACK_DGRAD swaps the roles - CO = Cin, the contraction runs over Cout - and flips the taps."""
    w9 = wq.reshape(wq.shape[0], wq.shape[1], 9)
    if mode == PACK_DGRAD:
        w9 = w9.transpose(0, 1)
        if flip:
            w9 = w9.flip(2)
    co, ci = w9.shape[0], w9.shape[1]
    return w9.reshape(co, ci // CK, 4, 8, 9).permute(1, 4, 2, 0, 3).contiguous()


# ==== the rows =======================================================================================================================
def _g_fwd(ops, f, g, T):
    return ops.k_conv_fwd(T.x, T.wt, T.b if f.bias else None, g, f.scale, BIAS_SCALE, ops.ACT_LRELU if f.act else ops.ACT_NONE, SLOPE),


def _g_dgrad(ops, f, g, T):
    return ops.k_conv_dgrad(T.gy, T.wt, g, f.scale),


def _g_wgrad(ops, f, g, T):
    return ops.k_conv_wgrad(T.gy, T.x, g, f.scale),


# op: needs, outs, role, bias, act, gpu, restate, define, bar against float64
OPS = {
    'fwd': (('x', 'wt', 'b'), ('y',), 'fwd', True, True, _g_fwd, r_fwd, d_fwd, TOL_FWD),
    'fwd_nobias': (('x', 'wt'), ('y',), 'fwd', False, True, _g_fwd, r_fwd, d_fwd, TOL_FWD),
    'fwd_noact': (('x', 'wt', 'b'), ('y',), 'fwd', True, False, _g_fwd, r_fwd, d_fwd, TOL_FWD),
    'dgrad': (('gy', 'wt'), ('gx',), 'dgrad', False, False, _g_dgrad, r_dgrad, d_dgrad, TOL_GRAD),
    'wgrad': (('x', 'gy'), ('gw',), 'wgrad', False, False, _g_wgrad, r_wgrad, d_wgrad, TOL_GRAD),
}


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


class Row(X.Form):
    """One kernel at one edge.  ``shape``: (N, Cin, Cout, H, W); ``plan``: [(symbol, workgroups)] the call must launch, in order;
    ``tile``: a row of the tile weight gradient, run in a process with GANLAB_BF16_WGRAD_ROLL=0; ``factor``: the bar of the
    ratio yardstick (2: exact_forms' factor)."""

    def __init__(self, name, op, kind, shape, facts, edge, why, dists=False, tile=False, factor=2.0):
        needs, outs, role, bias, act, gpu, restate, define, tol = OPS[op]
        n, ci, co, h, w = shape
        # (the scale as the fp32 number the library receives, so that float64 and the kernels multiply by the same value)
        X.Form.__init__(self, name, kind, role, shape, facts['plan'][0][0], f32(1.0 / (3 * ci ** 0.5)), needs,
                        lambda ops, f, g, T, x3: gpu(ops, f, g, T), restate, outs=outs)
        self.op, self.bias, self.act, self.define, self.tol = op, bias, act, define, tol
        self.facts, self.plan, self.edge, self.why, self.dists, self.tile, self.factor = facts, facts['plan'], edge, why, dists, tile, factor

    def at(self, shape):
        raise NotImplementedError('a row is its geometry')

    def geom(self, ops):
        n, ci, hin, win, co, up, pool = geom_args(self.kind, *self.shape)
        with ops.compute_dtype('bf16'):
            g = ops.Geom(n, ci, hin, win, co, 3, 1, up=up, pool=pool)
        assert g.bf is not None, self.name
        return g


def _rows():
    rows = []

    def conv(name, op, kind, shape, edge, why, **kw):
        rows.append(Row(name, op, kind, shape, fwd_facts(OPS[op][2], kind, *shape), edge, why, **kw))

    def roll(name, kind, shape, edge, why, **kw):
        rows.append(Row(name, 'wgrad', kind, shape, roll_facts(kind, *shape), edge, why, **kw))

    def tile(name, kind, shape, edge, why, **kw):
        rows.append(Row(name, 'wgrad', kind, shape, tile_facts(kind, *shape), edge, why, tile=True, **kw))

    def unsplit(th, tw, mode, **more):
        return lambda p: p['tile'] == (th, tw) and p['mode'] == mode and p['S'] == 1 and len(p['plan']) == 1 and \
            all(p[k] == v for k, v in more.items())

    def split(th, tw, mode, sizes):
        return lambda p: p['tile'] == (th, tw) and p['mode'] == mode and p['S'] == len(sizes) and p['splits'] == sizes and \
            len(p['plan']) == 2

    # ---- conv_fwd_bf16_kernel<TH, TW, UP, POOL>: forward rows carry a bias with bias_scale = 0.5 and LeakyReLU
    conv('fwd_8x32', 'fwd', 'plain', (2, 64, 64, 16, 64), unsplit(8, 32, 0, tiles_x=2, tiles_y=2),
         '<8,32> plain, two tiles each way: every halo side meets a neighbouring tile and an image border')
    # ``factor``: an accumulator takes 9 * chunks MFMA results one after the other, and the error of such a sequential fp32 chain
    # grows with the square root of its length, while ATen's blocked sums stay near 1e-7: measured kernel / ATen 1.45 at 18 steps
    # (64 channels), 1.97 at 36 and 1.93 at 45 (within 4 % of the bar of 2, less than ATen's own error moves between hosts),
    # 2.54 at 72 - the rows with chains of 36 steps or more carry the measured ratio with a margin
    conv('fwd_8x32_three_co_tiles', 'fwd', 'plain', (2, 128, 192, 24, 32), unsplit(8, 32, 0, tiles_co=3, tiles_y=3, chunks=4),
         '<8,32> plain, three channel tiles and four K chunks; H = 24 is a multiple of 8 but not of 16', factor=2.5)
    conv('fwd_16x16', 'fwd', 'plain', (2, 64, 128, 32, 48), unsplit(16, 16, 0, tiles_x=3, tiles_y=2, tiles_co=2),
         '<16,16> plain: 3 x 2 tiles, the width a multiple of 16 only')
    conv('fwd_8x32_nobias', 'fwd_nobias', 'plain', (2, 64, 64, 16, 64), unsplit(8, 32, 0), 'no bias (a null pointer), LeakyReLU')
    conv('fwd_16x16_noact', 'fwd_noact', 'plain', (2, 64, 128, 32, 48), unsplit(16, 16, 0), 'bias, no activation')
    conv('up_fwd_8x32', 'fwd', 'up', (2, 64, 64, 8, 32), unsplit(8, 32, 1, tiles_x=2, tiles_y=2),
         '<8,32,true,false> as an up layer\'s forward: taps at 16 x 64 over an 8 x 32 input', dists=True)
    conv('pool_dgrad_8x32', 'dgrad', 'pool', (2, 64, 64, 8, 32), unsplit(8, 32, 1, tiles_x=2, tiles_y=2),
         '<8,32,true,false> as a pooled layer\'s input gradient: up2(gy) / 4 folded into the staging (oscale 0.25)')
    conv('pool_fwd_8x32', 'fwd', 'pool', (2, 64, 64, 8, 32), unsplit(8, 32, 2, tiles_x=2, tiles_y=2),
         '<8,32,false,true> as a pooled layer\'s forward: bias and LeakyReLU after the 2 x 2 sum', dists=True)
    conv('up_dgrad_8x32', 'dgrad', 'up', (2, 64, 64, 8, 32), unsplit(8, 32, 2, tiles_x=2, tiles_y=2),
         '<8,32,false,true> as an up layer\'s input gradient: the 2 x 2 sum with factor 1')
    conv('up_fwd_16x16', 'fwd', 'up', (2, 64, 64, 16, 24), unsplit(16, 16, 1, tiles_x=3, tiles_y=2),
         '<16,16,true,false> as an up layer\'s forward: taps at 32 x 48')
    conv('pool_dgrad_16x16', 'dgrad', 'pool', (2, 64, 64, 16, 8), unsplit(16, 16, 1, tiles_x=1, tiles_y=2),
         '<16,16,true,false> as a pooled layer\'s input gradient: taps at 32 x 16')
    conv('pool_fwd_16x16', 'fwd', 'pool', (2, 64, 64, 16, 24), unsplit(16, 16, 2, tiles_x=3, tiles_y=2),
         '<16,16,false,true> as a pooled layer\'s forward: taps at 32 x 48')
    conv('up_dgrad_16x16', 'dgrad', 'up', (2, 64, 64, 16, 8), unsplit(16, 16, 2, tiles_x=1, tiles_y=2),
         '<16,16,false,true> as an up layer\'s input gradient: taps at 32 x 16')
    # ---- split-K: ks_chunks = ceil(chunks / S), nchunks = min(CI / 32, c_first + ks_chunks)
    conv('splitk_even', 'fwd', 'plain', (2, 256, 64, 16, 16), split(16, 16, 0, [4, 4]), 'split-K, 8 chunks in 2 even splits')
    conv('splitk_ragged_16x16', 'fwd', 'plain', (1, 448, 64, 16, 16), split(16, 16, 0, [5, 5, 4]),
         'ragged split-K: Cin = 448 is 14 chunks, S = 3, splits of 5, 5 and 4 - the last split stops at CI / 32', dists=True)
    conv('splitk_ragged_8x32', 'fwd', 'plain', (1, 448, 64, 8, 32), split(8, 32, 0, [5, 5, 4]),
         'the same ragged split on the <8,32> tile', dists=True)
    conv('splitk_ragged_up', 'fwd', 'up', (1, 448, 64, 8, 8), split(16, 16, 1, [5, 5, 4]),
         'ragged split-K behind the folded upsample (taps at 16 x 16)', dists=True)
    conv('splitk_ragged_pool', 'fwd', 'pool', (1, 448, 64, 8, 8), split(16, 16, 2, [5, 5, 4]),
         'ragged split-K with the 2 x 2 sum, the 1/4, the bias and LeakyReLU in the finish kernel', dists=True)
    conv('splitk_dgrad_cout_chunks', 'dgrad', 'plain', (1, 64, 448, 16, 16), lambda p: split(16, 16, 0, [5, 5, 4])(p) and p['CI'] == 448,
         'an input-gradient split whose Cout = 448, not Cin = 64, makes the 14 chunks', factor=2.5)     # (45 steps: 1.93 measured)
    conv('splitk_off_at_128_tiles', 'fwd', 'plain', (4, 256, 128, 64, 64), unsplit(8, 32, 0, tiles=128, chunks=8),
         'the plan returns 1 because tiles >= 128 although 8 chunks would allow a split: no finish kernel',
         factor=3.0)        # (72 steps, the longest chain of the table: 2.54 measured)
    # ---- conv_wgrad_bf16_roll_kernel<XUP, GUP> + wgrad_bf16_roll_reduce_kernel
    roll('roll_plain', 'plain', (2, 128, 192, 16, 64),
         lambda p: p['strips'] == 2 and p['tiles_ci'] == 2 and p['tiles_co'] == 3 and p['RS'] == 16 and p['pad_steps'] == 0,
         'plain, two strips, 2 x 3 channel tiles (a swapped tiles_ci / tiles_co decode would show); RS = 16: no padding step '
         'of the unroll by 3')
    roll('roll_pad2', 'plain', (2, 64, 64, 8, 32), lambda p: p['RS'] == 8 and p['pad_steps'] == 2, 'H = 8: RS = 8, two padding steps')
    roll('roll_pad1', 'plain', (2, 64, 64, 24, 32), lambda p: p['RS'] == 24 and p['pad_steps'] == 1, 'H = 24: RS = 24, one padding step')
    roll('roll_two_segments', 'plain', (2, 64, 64, 40, 32), lambda p: p['RS'] == 20 and p['segs_y'] == 2,
         'H = 40: RS = 20, two segments per image - a segment\'s rows r0 - 1 and r0 + RS belong to its neighbour')
    roll('roll_odd_streams', 'plain', (3, 64, 64, 8, 32), lambda p: p['streams'] % 2 == 1 and p['streams'] == 3 and p['flush'] == 2,
         'streams = 3 (three segments): the last workgroup\'s second pipeline is dead')
    roll('roll_two_passes', 'plain', (3, 512, 512, 8, 96),
         lambda p: p['nloop'] >= 2 and p['nseg'] % p['streams'] != 0 and (p['nseg'], p['streams'], p['nloop'], p['npairs']) == (9, 5, 2, 64),
         '64 channel-tile pairs want 8 pipelines; 9 segments -> 2 per pipeline, streams = 5, two passes: pipeline 4 is live on '
         'the first pass and dead on the second, and the last workgroup\'s second pipeline is dead throughout')
    roll('roll_up', 'up', (2, 64, 64, 8, 32), lambda p: p['RS'] == 16 and p['strips'] == 2,
         '<true,false>: x at half resolution, even RS = 16, two strips')
    roll('roll_pool', 'pool', (2, 64, 64, 8, 32), lambda p: p['RS'] == 16 and p['strips'] == 2,
         '<false,true>: gy at half resolution, even RS = 16, the 1/4 in the reduce scale')
    odd = lambda p: p['RS'] == 17 and p['segs_y'] == 8 and p['H'] == 136
    roll('roll_up_odd_rs', 'up', (1, 64, 64, 68, 16), odd,
         '<true,false>, taps at 136 x 32: RS = 17, every second segment starts on an odd row and reads x at R >> 1', dists=True)
    roll('roll_pool_odd_rs', 'pool', (1, 64, 64, 68, 16), odd,
         '<false,true>, a 136 x 32 input: RS = 17, every second segment starts on an odd row and reads gy at R >> 1', dists=True)
    roll('roll_plain_odd_rs', 'plain', (1, 64, 64, 136, 32), odd, 'plain at 136 x 32: RS = 17, 19 steps in 21', dists=True)
    # ---- conv_wgrad_bf16_kernel + wgrad_bf16_reduce_kernel (GANLAB_BF16_WGRAD_ROLL=0)
    tile('tile_slots_all', 'plain', (2, 64, 64, 8, 64), lambda p: p['slots'] == p['ntiles'] == 8 and p['strips'] >= 2 and p['row_tiles'] >= 2,
         'slots == ntiles: one 4-row tile per workgroup; two strips and two 4-row tiles per image')
    tile('tile_slots_ragged', 'plain', (2, 192, 128, 24, 128),
         lambda p: p['slots'] < p['ntiles'] and p['ntiles'] % p['slots'] != 0 and (p['tiles_co'], p['tiles_ci']) == (2, 6),
         '43 slots over 48 tiles: five workgroups walk two tiles; two co tiles by six ci tiles (Cin % 64 == 0 keeps the number '
         'of 32-channel ci tiles even, so three cannot occur)', dists=True)
    tile('tile_up_other_path', 'up', (2, 64, 64, 8, 32), lambda p: p['slots'] == p['ntiles'] and (p['H'], p['W']) == (16, 64),
         'an up layer with the rolling kernel off: bf16_wgrad_ok refuses the fused geometry, the wrapper materialises up2(x)')
    tile('tile_pool_other_path', 'pool', (2, 64, 64, 8, 32), lambda p: p['slots'] == p['ntiles'] and (p['H'], p['W']) == (16, 64),
         'a pooled layer with the rolling kernel off: the wrapper materialises up2(gy) / 4')
    return collections.OrderedDict((r.name, r) for r in rows)


ROWS = _rows()

# pack_bf16_kernel: (name, mode, Cout, Cin) - Cout != Cin so that the DGRAD role swap shows
PACK_ROWS = [('pack_fwd', PACK_FWD, 128, 64), ('pack_dgrad', PACK_DGRAD, 128, 64)]

# every instantiation launch_fwd, ganlab_conv_wgrad_bf16 and ganlab_conv_pack_bf16 can launch
INSTANTIATIONS = ['conv_fwd_bf16_kernel<%d, %d, %s>' % (th, tw, m) for th, tw in ((8, 32), (16, 16))
                  for m in ('false, false', 'true, false', 'false, true')] + \
    ['bf16_splitk_finish_kernel', 'conv_wgrad_bf16_roll_kernel<false, false>', 'conv_wgrad_bf16_roll_kernel<true, false>',
     'conv_wgrad_bf16_roll_kernel<false, true>', 'wgrad_bf16_roll_reduce_kernel', 'conv_wgrad_bf16_kernel', 'wgrad_bf16_reduce_kernel',
     'pack_bf16_kernel']

# non-finite values: (row, poisoned pixel of image 0 in the operand's own resolution) - the last row / column of a tile or strip
# that has a neighbour, never the image's first or last row of a weight gradient: there the kernels multiply the row by a slot of
# zeros for the gradient row outside the image, which linear algebra leaves out
NONFINITE = [
    ('fwd_8x32', (7, 31)), ('fwd_16x16', (15, 15)), ('up_dgrad_8x32', (7, 31)), ('pool_dgrad_16x16', (7, 7)), ('splitk_even', (7, 15)),
    ('roll_plain', (7, 31)), ('roll_up', (3, 15)), ('roll_pool', (7, 31)),
]
POISON_CHANNEL = 1


# ==== running a row ==================================================================================================================
def run(ops, f, T):
    """(outputs on the CPU, [(symbol, workgroups)] launched) of row ``f`` on operands ``T`` (CPU fp32, NOT rounded)"""
    from gan_lab_amd import _lib
    Tg = X.to_gpu(T)
    g = f.geom(ops)
    with torch.no_grad():
        c0 = _lib.launch_count()
        out = f.gpu(ops, f, g, Tg, False)
        torch.cuda.synchronize()
        launches = _lib.launches_since(c0)
    return tuple(v.cpu() for v in out), [(norm(k or ''), n) for k, n in launches]
