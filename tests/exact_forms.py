"""The exact-fp32 convolution kernels by name: one row per kernel per edge (csrc/conv.hip, conv_s2.hip, conv_roll_blur.hip,
conv_s2_roll.hip, conv_s2_roll_blur.hip, wgrad_roll.hip and the rolling modulated conv of mod.hip).

A row is a ``Form`` of tests/x3_forms.py (geometry, operands, GPU call) plus
  * ``symbol``: the kernel the call must launch, a substring of the demangled name with the template arguments that select
    another body (compared without blanks and without ``(anonymous namespace)::``);
  * ``plan``: every launch of the call the table restates, as (symbol, workgroups) in launch order - the kernel, then its
    finish kernels - computed by the plain-Python restatements of the launchers' plans below (``run_conv_plan`` for
    ``launch_fwd`` and the dispatch in front of it, ``wgrad_plan`` / ``wr_plan``, ``rb_plan``, the stride-2 plans);
  * ``restate``: the operation in float64 from explicit shifted sums (no autograd, no other gan_lab_amd path) and ``define``:
    the layer's definition with ``torch.autograd`` - run in float64 it guards ``restate`` (tests/test_exact_forms_host.py), run
    in fp32 on the CPU it is the ATen yardstick of tests/test_gpu_exact_kernels.py;
  * ``edge``: what the row is for.
Every row runs with ``ops.set_x3(False)``.  Shapes are (N, Cin, Cout, H, W) of the layer - of a stride-2 layer its LOW
resolution, as in tests/x3_forms.py.  Nothing here asserts a bar."""
import collections
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import x3_forms as X
from x3_forms import BIAS_SCALE, TAIL_BIAS_SCALE, SLOPE, EPS

RGB_SCALE, SMALL_BIAS_SCALE = 0.01, 0.01      # (small: the tiny / huge draws keep the summed outputs inside [1e-20, 1e20])


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


# ==== the launchers' plans, restated =================================================================================================
XS, XV, XU = 0, 1, 2        # staging modes of conv.hip: element-wise, vector, vector with the upsample folded in


def cfg_name(kind, args):
    return '%s<%s>' % (kind, ', '.join(str(a) for a in args))


def pw_small_ok(cin, cout, ks, pad, up, hi, wi):
    hw = hi * wi
    return ks == 1 and pad == 0 and not up and hw % 4 == 0 and hw >= 4096 and ((cin <= 4 and cout <= 64) or (cout <= 4 and cin <= 64))


def _px_tiles(n, ho, wo):
    if ho == 1 and wo == 1:
        return cdiv(n, 64)
    if wo >= 32:
        return cdiv(wo, 32) * cdiv(ho, 8) * n
    if wo >= 16:
        return cdiv(wo, 16) * cdiv(ho, 16) * n
    if wo >= 8:
        return cdiv(wo, 8) * cdiv(ho, 8) * cdiv(n, 4)
    return cdiv(wo, 4) * cdiv(ho, 4) * cdiv(n, 16)


def _px_tiles_mb4(px, n, ho, wo, ks):
    return cdiv(wo, 16) * cdiv(ho, 8) * n if ks == 3 and wo >= 16 else px


def _mb(n, cout, ho, wo, ks):
    """dispatch_co: 16-channel blocks per workgroup"""
    if cout <= 16:
        return 1
    if cout <= 32:
        return 2
    px = _px_tiles(n, ho, wo)
    if _px_tiles_mb4(px, n, ho, wo, ks) * cdiv(cout, 64) >= 256:
        return 4
    return 2 if px * cdiv(cout, 32) >= 256 else 1


def splitk_plan(n, cin, cout, ho, wo, ks):
    if wo >= 32 and not (ho == 1 and wo == 1):
        return 1
    px = _px_tiles(n, ho, wo)
    mb = _mb(n, cout, ho, wo, ks)
    if ks == 3 and mb == 4 and wo < 16:
        mb = 2
    if mb == 4:
        px = _px_tiles_mb4(px, n, ho, wo, ks)
    wgs = px * cdiv(cout, 16 * mb)
    ci_t = 32 if ks == 1 else (16 if (wo >= 16 and mb == 1) else 8)
    chunks = rup(cin, 32 if ks == 1 else 16) // ci_t
    s = min(cdiv(512, wgs), 8 if (ho == 1 and wo == 1) else 4, chunks // 4)
    while s > 1 and (s - 1) * cdiv(chunks, s) >= chunks:
        s -= 1
    return 1 if s < 2 else s


def rb_plan(n, h, w, blur):
    """conv_roll_blur.hip: (64-pixel columns, row strips per column, 4-row steps per strip, workgroups)"""
    cols, steps = w // 64, h // 4
    k = 1
    while k < steps and cols * n * k < 4096 and (steps + k) // (k + 1) >= (16 if blur else 8):
        k += 1
    spu = cdiv(steps, k)
    strips = cdiv(steps, spu)
    return cols, strips, spu, cols * n * strips


def fwd_cfg(n, cin, hi, wi, cout, ks, pad, up):
    """dispatch_co + dispatch_geom: the FwdCfg arguments (KS, MB, TWL, THL, NIL, XMODE)"""
    hv, wv = (2 * hi, 2 * wi) if up else (hi, wi)
    ho, wo = hv + 2 * pad - ks + 1, wv + 2 * pad - ks + 1
    mb = _mb(n, cout, ho, wo, ks)
    if ho == 1 and wo == 1:
        return (ks, mb, 0, 0, 6, XS)
    if wo < 16 or wi % 4 or pad != (ks - 1) // 2:
        mode = XS
    elif up:
        mode = XU if ks == 3 else XS
    else:
        mode = XV
    if ks == 3 and mb == 4 and wo >= 16 and mode == XV:
        return (3, 4, 4, 3, 0, XV)                  # ThickCfg
    if wo >= 32:
        return (ks, mb, 5, 3, 0, mode)
    if wo >= 16:
        return (ks, mb, 4, 4, 0, mode)
    mbs = 2 if (ks == 3 and mb == 4) else mb
    return (ks, mbs, 3, 3, 2, XS) if wo >= 8 else (ks, mbs, 2, 2, 4, XS)


def run_conv_plan(n, cin, hi, wi, cout, ks, pad, up=0, mask=False, ksplit=1):
    """conv.hip run_conv -> launch_fwd: [(symbol, workgroups)]"""
    hv, wv = (2 * hi, 2 * wi) if up else (hi, wi)
    ho, wo = hv + 2 * pad - ks + 1, wv + 2 * pad - ks + 1
    if not mask and pw_small_ok(cin, cout, ks, pad, up, hi, wi):
        items = n * (hi * wi // 4)
        return [('pw_few_to_many_kernel' if cin <= 4 else 'pw_many_to_few_kernel', min(cdiv(items, 256), 4096))]
    cfg = fwd_cfg(n, cin, hi, wi, cout, ks, pad, up)
    _, mb, twl, thl, nil, mode = cfg
    tw, th, ni, co_t = 1 << twl, 1 << thl, 1 << nil, 16 * mb
    ci_t = 32 if ks == 1 else (16 if (mb == 1 and mode != XS) else 8)
    cin_p = rup(cin, 32 if ks == 1 else 16)
    tx, ty, tn, tco = cdiv(wo, tw), cdiv(ho, th), cdiv(n, ni), cdiv(cout, co_t)
    tiles = tx * ty * tn * tco
    name = cfg_name('FwdCfg', cfg)
    if mb == 1 and mode != XS and cin_p == ci_t and wo % tw == 0 and ho % th == 0 and cout % co_t == 0 and not mask:
        if ks == 3 and mode == XV:
            if wo % 64 == 0 and ho % 4 == 0 and cout <= 16 and tco == 1 and not up and pad == 1:
                return [('conv_fwd_roll2_kernel', rb_plan(n, hi, wi, 0)[3])]
            ky = 1
            while ky < ty and tiles // cdiv(ty, ky) < 6144:
                ky += 1
            strip = cdiv(ty, ky)
            return [('conv_fwd_strip2_kernel<%s>' % name, tx * cdiv(ty, strip) * tn * tco)]
        k = 1
        while k < tx and tiles // cdiv(tx, k) < 6144:
            k += 1
        strip = cdiv(tx, k)
        return [('conv_fwd_strip_kernel<%s>' % name, cdiv(tx, strip) * ty * tn * tco)]
    if ksplit > 1:
        assert mode == XS or (mode == XV and tw == 16)
        return [('conv_fwd_kernel<%s, false, true, false, false>' % name, tiles * ksplit),
                ('splitk_finish_kernel', cdiv(n * cout * ho * wo, 256))]
    if mask:
        assert ks == 3 and mode == XV
        return [('conv_fwd_kernel<%s, true, false, false, false>' % name, tiles)]
    return [('conv_fwd_kernel<%s, false, false, false, false>' % name, tiles)]


def wr_plan(n, cin, cout, h, w):
    """wgrad_roll.hip: dict of the unit split of the rolling 3x3 weight gradient"""
    cols, steps = w // 64, h // 4
    tci, tco = cdiv(cin, 16), cdiv(cout, 16)
    target = cdiv(768, tci * tco)
    spu = 16
    for cand in (64, 32):
        units = n * cols * cdiv(steps, cand)
        if steps >= cand and 2 * units >= 5 * target:
            spu = cand
            break
    spu = min(steps, spu)
    strips = cdiv(steps, spu)
    units = n * cols * strips
    s = max(1, min(target, units))
    return dict(cols=cols, steps=steps, spu=spu, strips=strips, units=units, S=s, grid=tco * tci * s,
                units_per_wg=cdiv(units, s))


def wr_ok(n, cin, cout, h, w, ks, pad, up):
    return ks == 3 and pad == 1 and not up and cin <= 32 and cout <= 32 and h % 4 == 0 and w % 64 == 0 and h >= 8


def _reduce_launches(slots, nw):
    nblk = cdiv(nw, 256)
    return [('wgrad_reduce_kernel', nblk * 32), ('wgrad_reduce_kernel', nblk)] if slots >= 64 else [('wgrad_reduce_kernel', nblk)]


def wg_cfg(n, cin, hi, wi, cout, ks, pad, up):
    """plan_wgrad: the WgCfg arguments (KS, NBC, WM, WK, TWL, THL, NIL, XMODE)"""
    hv, wv = (2 * hi, 2 * wi) if up else (hi, wi)
    ho, wo = hv + 2 * pad - ks + 1, wv + 2 * pad - ks + 1
    thin = cout <= 32
    nbc = 1 if (thin and cin <= 16) else 2
    if ho == 1 and wo == 1:
        geo = 'E'
    elif not thin:
        geo = 'A' if wo >= 8 else 'D'
    else:
        geo = 'A' if wo >= 32 else ('B' if wo >= 16 else ('C' if wo >= 8 else 'D'))
    tw = ({'A': 32, 'B': 16}.get(geo, 0)) if thin else (8 if geo == 'A' else 0)
    xm = XS
    if tw >= 8 and not wi % 4 and not wo % 4 and pad == (ks - 1) // 2:
        xm = (XU if ks == 3 else XS) if up else XV
    if thin:
        twl, thl, nil = {'A': (5, 3, 0), 'B': (4, 4, 0), 'C': (3, 3, 2), 'D': (2, 2, 4), 'E': (0, 0, 6)}[geo]
        if geo in 'CDE':
            xm = XS
        return (ks, nbc, 1, 4, twl, thl, nil, xm)
    twl, thl, nil = {'A': (3, 3, 0), 'D': (2, 2, 2), 'E': (0, 0, 6)}[geo]
    return (ks, 2, 4, 1, twl, thl, nil, xm if geo == 'A' else XS)


def wgrad_plan(n, cin, hi, wi, cout, ks, pad, up=0, aff=False):
    """conv.hip ganlab_conv_wgrad_f32 / ganlab_conv_wgrad_aff_f32: [(symbol, workgroups)]"""
    hv, wv = (2 * hi, 2 * wi) if up else (hi, wi)
    ho, wo = hv + 2 * pad - ks + 1, wv + 2 * pad - ks + 1
    nw = cout * cin * ks * ks
    cfg = wg_cfg(n, cin, hi, wi, cout, ks, pad, up)
    _, nbc, wm, wk, twl, thl, nil, _xm = cfg
    tco, tci = cdiv(cout, 16 * wm), cdiv(cin, 16 * nbc)
    n_tiles = cdiv(wo, 1 << twl) * cdiv(ho, 1 << thl) * cdiv(n, 1 << nil)
    s = max(1, min(cdiv(768 if (wm == 1 and nbc == 1) else 512, tco * tci), n_tiles))
    slots = s * wk
    if not aff and pw_small_ok(cin, cout, ks, pad, up, hi, wi):
        btot = cout if cin <= 4 else cin
        out = []
        for _b0 in range(0, btot, 16):
            out += [('pw_cross_sums_kernel', 1024), ('pw_cross_finish_kernel', 1)]
        return out
    if wr_ok(n, cin, cout, hi, wi, ks, pad, up):
        p = wr_plan(n, cin, cout, hi, wi)
        assert p['S'] <= slots          # (else the workspace sized for the tile kernel would not hold the rolling kernel's slots)
        return [('conv_wgrad_roll_kernel<%s>' % ('true' if aff else 'false'), p['grid'])] + _reduce_launches(p['S'], nw)
    if aff:
        assert cfg == (3, 2, 4, 1, 3, 3, 0, XV), cfg
    return [('conv_wgrad_kernel<%s, %s>' % (cfg_name('WgCfg', cfg), 'true' if aff else 'false'), tco * tci * s)] + \
        _reduce_launches(slots, nw)


# ---- stride-2 (conv_s2.hip, conv_s2_roll.hip, conv_s2_roll_blur.hip, wgrad_roll.hip) -------------------------------------------------
def sr_plan(n, hl, wl, min_steps=8):
    """conv_s2_roll.hip sr_plan (min_steps = 16: conv_s2_roll_blur.hip tb_plan): (columns, strips, steps per strip, workgroups)"""
    cols, steps = wl // 32, hl // 2
    k = 1
    while k < steps and cols * n * k < 4096 and (steps + k) // (k + 1) >= min_steps:
        k += 1
    spu = cdiv(steps, k)
    strips = cdiv(steps, spu)
    return cols, strips, spu, cols * strips * n


def _s2_roll_ok(is_t, cin, cout, hl, wl):
    if hl < 4 or hl % 2 or wl % 32:
        return False
    return (16 < cin <= 32 and cout <= 16) if is_t else (cin <= 16 and 16 < cout <= 32)


def s2_S_plan(n, cin, cout, hl, wl):
    """run_S: the strided form (a pooled layer's forward, an up layer's input gradient); cin: HIGH-resolution channels"""
    if _s2_roll_ok(0, cin, cout, hl, wl):
        return [('conv_s2_down_roll_kernel', sr_plan(n, hl, wl)[3])]
    if wl <= 16 and cout > 32:
        cfg = (4, 4, 2)
    elif cout <= 16:
        cfg = (1, 5, 4)
    elif cout <= 32:
        cfg = (2, 5, 4)
    else:
        cfg = (4, 4, 2)
    mb, twl, nb = cfg
    tw = 1 << twl
    th = 64 * nb // tw
    return [('conv_s2_down_kernel<%s>' % cfg_name('SCfg', cfg), cdiv(wl, tw) * cdiv(hl, th) * cdiv(cout, 16 * mb) * n)]


def s2_T_plan(n, cin, cout, hl, wl, aff=False):
    """run_T: the transposed form (an up layer's forward, a pooled layer's input gradient); cin: LOW-resolution channels"""
    if _s2_roll_ok(1, cin, cout, hl, wl):
        return [('conv_s2_up_roll_kernel<%s>' % ('true' if aff else 'false'), sr_plan(n, hl, wl)[3])]
    if aff:
        assert cout > 16 and cin <= 512
        cfg = (1, 2) if cin >= 128 else (2, 2)
    elif cout <= 16:
        cfg = (1, 4)
    else:
        cfg = (1, 2) if cin >= 128 else (2, 2)
    mb, nbl = cfg
    tw, th = (32 if nbl == 4 else 16), (4 if nbl == 1 else 8)
    return [('conv_s2_up_kernel<%s, %s>' % (cfg_name('TCfg', cfg), 'true' if aff else 'false'),
             cdiv(wl, tw) * cdiv(hl, th) * cdiv(cout, 16 * mb) * n)]


def w2r_plan(n, cl, ch, hl, wl):
    cols, steps = wl // 32, hl // 2
    nba = 2 if cl > 16 else 1
    tcl, tch = cdiv(cl, 16 * nba), cdiv(ch, 16)
    target = cdiv(768, tcl * tch)
    spu = 16
    for cand in (64, 32):
        units = n * cols * cdiv(steps, cand)
        if steps >= cand and 2 * units >= 5 * target:
            spu = cand
            break
    spu = min(steps, spu)
    strips = cdiv(steps, spu)
    units = n * cols * strips
    s = max(1, min(target, units))
    return dict(nba=nba, steps=steps, spu=spu, strips=strips, units=units, S=s, grid=tcl * tch * s, units_per_wg=cdiv(units, s))


def s2_wgrad_plan(n, cin, cout, hl, wl, pool, aff=False):
    """ganlab_conv_s2_wgrad_f32 / _aff_f32 and s2_finish_wgrad"""
    cl, ch = (cout, cin) if pool else (cin, cout)
    nk = 16 * cl * ch
    if wl % 32 == 0 and hl % 2 == 0 and hl >= 4:
        p = w2r_plan(n, cl, ch, hl, wl)
        out = [('conv_s2_wgrad_roll2_kernel<%d, %s>' % (p['nba'], 'true' if aff else 'false'), p['grid'])]
        slots = p['S']
    else:
        assert not aff
        nba = 2 if cl > 16 else 1
        tcl, tch = cdiv(cl, 16 * nba), cdiv(ch, 16)
        slots = max(1, min(cdiv(768, tcl * tch), cdiv(wl, 16) * cdiv(hl, 4) * n))
        out = [('conv_s2_wgrad_kernel<WCfg<%d>>' % nba, tcl * tch * slots)]
    groups = slots
    if groups >= 64:
        out.append(('reduce_s2_slots_kernel', cdiv(nk, 256) * 32))
        groups = 32
    if groups > 2:
        out.append(('reduce_s2_slots_kernel', cdiv(nk, 256)))
    out.append(('fold_s2_kernel', cdiv(cout * cin, 128)))
    return out


# ==== float64 restatements (explicit shifted sums) and definitions (autograd) ========================================================
def r_up2(v):
    return v.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def r_box(v):
    n, c, h, w = v.shape
    return v.reshape(n, c, h // 2, 2, w // 2, 2).sum(dim=(3, 5))


def r_conv(x, w, pad):
    """cross-correlation, zero padding ``pad`` each side: sum over the taps of a channel contraction of the shifted input"""
    ks = w.shape[2]
    h, wd = x.shape[2] + 2 * pad - ks + 1, x.shape[3] + 2 * pad - ks + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    y = None
    for ky in range(ks):
        for kx in range(ks):
            t = torch.einsum('nihw,oi->nohw', xp[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx])
            y = t if y is None else y + t
    return y


def r_lin(f, x, w):
    y = r_conv(r_up2(x) if f.kind == 'up' else x, w * f.scale, f.pad)
    return r_box(y) / 4 if f.kind == 'pool' else y


def r_dgrad(f, gy, w):
    gv = r_up2(gy) / 4 if f.kind == 'pool' else gy
    gx = r_conv(gv, (w * f.scale).flip(2, 3).transpose(0, 1), f.ks - 1 - f.pad)
    return r_box(gx) if f.kind == 'up' else gx


def r_wgrad(f, x, gy):
    xv = r_up2(x) if f.kind == 'up' else x
    gv = r_up2(gy) / 4 if f.kind == 'pool' else gy
    h, wd = gv.shape[2], gv.shape[3]
    xp = F.pad(xv, (f.pad,) * 4)
    gw = torch.empty(f.co, f.ci, f.ks, f.ks, dtype=x.dtype)
    for ky in range(f.ks):
        for kx in range(f.ks):
            gw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', gv, xp[:, :, ky:ky + h, kx:kx + wd])
    return gw * f.scale


def r_blur(v):
    """binomial [1 2 1] x [1 2 1] / 16, zero outside the image"""
    p = F.pad(v, (1, 1, 1, 1))
    hz = p[:, :, :, :-2] + 2 * p[:, :, :, 1:-1] + p[:, :, :, 2:]
    return (hz[:, :, :-2] + 2 * hz[:, :, 1:-1] + hz[:, :, 2:]) / 16


def r_lrelu(v):
    return torch.where(v > 0, v, v * SLOPE)


def r_dlrelu(v):
    return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, SLOPE))


def _cb(v, k):
    return k * v.view(1, -1, 1, 1)


def _aff(T, f):
    return T.x * T.s.view(f.n, f.ci, 1, 1) + T.t.view(f.n, f.ci, 1, 1)


def _stats(y):
    return y, y.mean(dim=(2, 3)), 1.0 / torch.sqrt(y.var(dim=(2, 3), unbiased=False) + EPS)


def r_stats(y):
    m = y.sum(dim=(2, 3)) / (y.shape[2] * y.shape[3])
    var = ((y - m[:, :, None, None]) ** 2).sum(dim=(2, 3)) / (y.shape[2] * y.shape[3])
    return y, m, (var + EPS) ** -0.5


def d_lin(f, x, w):
    """the layer's linear part by definition: (nearest upsample ->) conv (-> average pool)"""
    if f.kind == 'up':
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    y = F.conv2d(x, w * f.scale, None, padding=f.pad)
    return F.avg_pool2d(y, 2) if f.kind == 'pool' else y


def d_blur(v):
    k = torch.tensor([1., 2., 1.], dtype=v.dtype)
    k = (k[:, None] * k[None, :] / 16.).expand(v.shape[1], 1, 3, 3)
    return F.conv2d(v, k, padding=1, groups=v.shape[1])


def _d_dgrad(f, T):
    xd = torch.zeros(f.n, f.ci, *f.hw_in, dtype=T.gy.dtype, requires_grad=True)
    return torch.autograd.grad(d_lin(f, xd, T.wt), xd, T.gy)[0]


def _d_wgrad(f, T, x):
    wd = torch.zeros(f.co, f.ci, f.ks, f.ks, dtype=T.gy.dtype, requires_grad=True)
    return torch.autograd.grad(d_lin(f, x, wd), wd, T.gy)[0]


# kind of operation -> (needs, outs, gpu call, restatement, definition); gpu: (ops, f, g, T) -> outputs
def _bits_of(pre):
    """sign bits of a tensor, bit e of byte e >> 3 by the NCHW-linear index: 1 = positive"""
    packed = np.packbits((pre > 0).cpu().numpy().ravel(), bitorder='little')
    return torch.from_numpy(packed.view(np.int32).copy()).cuda()


def _p(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _g_fwd(ops, f, g, T):
    return ops.k_conv_fwd(T.x, T.wt, T.b, g, f.scale, BIAS_SCALE, ops.ACT_LRELU, SLOPE),


def _g_dgrad(ops, f, g, T):
    return ops.k_conv_dgrad(T.gy, T.wt, g, f.scale),


def _g_dgrad_mask(ops, f, g, T):
    return ops.k_conv_dgrad_mask(T.gy, T.wt, T.x, g, f.scale, SLOPE),


def _g_wgrad(ops, f, g, T):
    return ops.k_conv_wgrad(T.gy, T.x, g, f.scale),


def _g_wgrad_aff(ops, f, g, T):
    return ops.k_conv_wgrad_aff(T.gy, T.x, T.s, T.t, g, f.scale),


def _g_fwd_aff(ops, f, g, T):
    return ops.k_conv_fwd_aff(T.x, T.s, T.t, T.wt, g, f.scale),


def _g_tail(entry, chunks_fn):
    def run(ops, f, g, T):
        """y = lrelu(conv(a * s + t) + noise_w * noise + bias) and the InstanceNorm statistics of y, through the library entry"""
        from gan_lab_amd import _lib
        L = _lib.lib()
        y = torch.empty(f.n, f.co, *f.hw_out, device='cuda')
        mean, rstd = torch.empty(f.n, f.co, device='cuda'), torch.empty(f.n, f.co, device='cuda')
        chunks = getattr(L, chunks_fn)(g.ref())
        assert chunks > 0, (f.name, chunks)
        ws = torch.empty(f.n * f.co * chunks * 2, dtype=torch.float64, device='cuda')
        wp = ops._packed(T.wt, ops.PACK_FWD, f.scale)
        _lib.check(getattr(L, entry)(_p(T.x), _p(wp), _p(T.s), _p(T.t), _p(T.b), _p(T.nz), _p(T.nw), _p(y), _p(mean), _p(rstd),
                                     g.ref(), TAIL_BIAS_SCALE, ops.ACT_LRELU, SLOPE, EPS, _p(ws), ws.numel() * 8, None), entry)
        return y, mean, rstd
    return run


def _g_blur(ops, f, g, T):
    out = ops.k_conv_fwd_blur_bits(T.x, T.wt, T.b, g, f.scale, BIAS_SCALE, SLOPE)
    assert out is not None, f.name
    return out[0],


def _g_up_blur_tail(ops, f, g, T):
    return ops.k_conv_s2_fwd_blur_tail(T.x, T.s, T.t, T.wt, T.b, T.nz, T.nw, g, f.scale, TAIL_BIAS_SCALE, ops.ACT_LRELU, SLOPE, EPS)


def _g_pool_dgrad_blur(ops, f, g, T):
    return ops.k_conv_s2_dgrad_blur_act(T.gy, T.wt, _bits_of(T.pre), g, f.scale, SLOPE, SMALL_BIAS_SCALE, True)


def _g_rgb(ops, f, g, T):
    from gan_lab_amd import _lib
    L = _lib.lib()
    gw, gb = torch.zeros(f.ci, 3, device='cuda'), torch.zeros(f.ci, device='cuda')
    ws = torch.empty((L.ganlab_conv_dgrad_rgb_sums_workspace(g.ref()) + 7) // 8, dtype=torch.float64, device='cuda')
    wp = ops._packed(T.wt, ops.PACK_DGRAD, f.scale)
    bits = _bits_of(T.pre)
    _lib.check(L.ganlab_conv_dgrad_rgb_sums_f32(_p(T.gy), _p(wp), ctypes.c_void_p(bits.data_ptr()), _p(T.img), _p(gw), _p(gb), g.ref(),
                                                3, RGB_SCALE, SMALL_BIAS_SCALE, SLOPE, 0, 0, _p(ws), ws.numel() * 8, None),
               'conv_dgrad_rgb_sums')
    return gw, gb


def _r_tail(f, T):
    return r_stats(r_lrelu(r_lin(f, _aff(T, f), T.wt) + T.nw.view(1, -1, 1, 1) * T.nz + _cb(T.b, TAIL_BIAS_SCALE)))


def _d_tail(f, T):
    return _stats(F.leaky_relu(d_lin(f, _aff(T, f), T.wt) + T.nw.view(1, -1, 1, 1) * T.nz + _cb(T.b, TAIL_BIAS_SCALE), SLOPE))


def _r_up_blur_tail(f, T):
    return r_stats(r_lrelu(r_blur(r_lin(f, _aff(T, f), T.wt)) + T.nw.view(1, -1, 1, 1) * T.nz + _cb(T.b, TAIL_BIAS_SCALE)))


def _d_up_blur_tail(f, T):
    return _stats(F.leaky_relu(d_blur(d_lin(f, _aff(T, f), T.wt)) + T.nw.view(1, -1, 1, 1) * T.nz + _cb(T.b, TAIL_BIAS_SCALE), SLOPE))


def _r_pool_dgrad_blur(f, T):
    gz = r_dlrelu(T.pre) * r_blur(r_dgrad(f, T.gy, T.wt))       # (the blur is its own adjoint: symmetric taps, zero padding)
    return gz, SMALL_BIAS_SCALE * gz.sum(dim=(0, 2, 3))


def _d_pool_dgrad_blur(f, T):
    """a = lrelu(pre + bias), z = blur(a), y = pool(conv(z)): the gradients of pre and of the bias (bias_scale * bias = 0)"""
    bd = torch.zeros(f.ci, dtype=T.gy.dtype, requires_grad=True)
    pd = T.pre.clone().requires_grad_(True)
    y = d_lin(f, d_blur(F.leaky_relu(pd + _cb(bd, SMALL_BIAS_SCALE), SLOPE)), T.wt)
    return torch.autograd.grad(y, (pd, bd), T.gy)


def _r_rgb(f, T):
    gz = r_dlrelu(T.pre) * r_dgrad(f, T.gy, T.wt)
    return RGB_SCALE * torch.einsum('nohw,nchw->oc', gz, T.img), SMALL_BIAS_SCALE * gz.sum(dim=(0, 2, 3))


def _d_rgb(f, T):
    """h = lrelu(fromRGB(img)) with fromRGB's output pre (its sign is all the backward keeps), y = conv3x3(h): the gradients
    of fromRGB's weight and bias"""
    wr = torch.zeros(f.ci, 3, 1, 1, dtype=T.gy.dtype, requires_grad=True)
    br = torch.zeros(f.ci, dtype=T.gy.dtype, requires_grad=True)
    lin = F.conv2d(T.img, wr * RGB_SCALE) + _cb(br, SMALL_BIAS_SCALE)
    h = F.leaky_relu(T.pre, SLOPE) + lin * r_dlrelu(T.pre)          # lrelu(pre + lin) to first order in the zero parameters
    gw, gb = torch.autograd.grad(d_lin(f, h, T.wt), (wr, br), T.gy)
    return gw.view(f.ci, 3), gb


_FWD, _DG, _WG, _AFF_N = ('x', 'wt', 'b'), ('gy', 'wt'), ('x', 'gy'), ('x', 's', 't', 'wt')
_TAIL_N = _AFF_N + ('b', 'nz', 'nw')
OPS = {
    # op: needs, outs, role, aff, tail, gpu, restate, define
    'fwd': (_FWD, ('y',), 'fwd', False, False, _g_fwd,
            lambda f, T: (r_lrelu(r_lin(f, T.x, T.wt) + _cb(T.b, BIAS_SCALE)),),
            lambda f, T: (F.leaky_relu(d_lin(f, T.x, T.wt) + _cb(T.b, BIAS_SCALE), SLOPE),)),
    'dgrad': (_DG, ('gx',), 'dgrad', False, False, _g_dgrad,
              lambda f, T: (r_dgrad(f, T.gy, T.wt),), lambda f, T: (_d_dgrad(f, T),)),
    'dgrad_mask': (_DG + ('x',), ('gx',), 'dgrad', False, False, _g_dgrad_mask,
                   lambda f, T: (r_dgrad(f, T.gy, T.wt) * r_dlrelu(T.x),), lambda f, T: (_d_dgrad(f, T) * r_dlrelu(T.x),)),
    'wgrad': (_WG, ('gw',), 'wgrad', False, False, _g_wgrad,
              lambda f, T: (r_wgrad(f, T.x, T.gy),), lambda f, T: (_d_wgrad(f, T, T.x),)),
    'wgrad_aff': (_WG + ('s', 't'), ('gw',), 'wgrad', True, False, _g_wgrad_aff,
                  lambda f, T: (r_wgrad(f, _aff(T, f), T.gy),), lambda f, T: (_d_wgrad(f, T, _aff(T, f)),)),
    'fwd_aff': (_AFF_N, ('y',), 'fwd', True, False, _g_fwd_aff,
                lambda f, T: (r_lin(f, _aff(T, f), T.wt),), lambda f, T: (d_lin(f, _aff(T, f), T.wt),)),
    'tail': (_TAIL_N, ('y', 'mean', 'rstd'), 'fwd', True, True,
             _g_tail('ganlab_conv_fwd_aff_tail_f32', 'ganlab_conv_fwd_aff_tail_chunks'), _r_tail, _d_tail),
    'mod': (_TAIL_N, ('y', 'mean', 'rstd'), 'fwd', True, True,
            _g_tail('ganlab_mod_conv_fwd_f32', 'ganlab_mod_conv_stat_chunks'), _r_tail, _d_tail),
    'blur': (_FWD, ('y',), 'fwd', False, False, _g_blur,
             lambda f, T: (r_blur(r_lrelu(r_lin(f, T.x, T.wt) + _cb(T.b, BIAS_SCALE))),),
             lambda f, T: (d_blur(F.leaky_relu(d_lin(f, T.x, T.wt) + _cb(T.b, BIAS_SCALE), SLOPE)),)),
    'up_blur_tail': (_TAIL_N, ('y', 'mean', 'rstd'), 'fwd', True, True, _g_up_blur_tail, _r_up_blur_tail, _d_up_blur_tail),
    'pool_dgrad_blur': (_DG + ('pre',), ('gz', 'gb'), 'dgrad', False, False, _g_pool_dgrad_blur, _r_pool_dgrad_blur,
                        _d_pool_dgrad_blur),
    'rgb': (_DG + ('pre', 'img'), ('gw_rgb', 'gb_rgb'), 'dgrad', False, False, _g_rgb, _r_rgb, _d_rgb),
}


class Row(X.Form):
    """One kernel at one edge.  ``shape``: (N, Cin, Cout, H, W); ``plan``: [(symbol, workgroups)] the call must launch, in order."""

    def __init__(self, name, op, kind, shape, ks, symbol, plan, edge, dists=False, factor=2.0, claims=None):
        needs, outs, role, aff, tail, gpu, restate, define = OPS[op]
        n, ci, co, h, w = shape
        X.Form.__init__(self, name, kind, role, shape, symbol, 1.0 / (ks * ci ** 0.5), needs, lambda ops, f, g, T, x3: gpu(ops, f, g, T),
                        restate, outs=outs, aff=aff, tail=tail)
        self.op, self.ks, self.pad, self.plan, self.edge, self.dists, self.factor = op, ks, (ks - 1) // 2, plan, edge, dists, factor
        self.define, self.claims = define, claims or {}

    def at(self, shape):
        raise NotImplementedError('a row is its geometry')

    def geom(self, ops):
        return ops.Geom(self.n, self.ci, self.hw_in[0], self.hw_in[1], self.co, self.ks, self.pad, up=int(self.kind == 'up'),
                        pool=int(self.kind == 'pool'))

    def operand_shapes(self):
        d = X.Form.operand_shapes(self)
        d.update(wt=(self.co, self.ci, self.ks, self.ks), pre=(self.n, self.ci) + self.hw_in, img=(self.n, 3) + self.hw_in)
        return d


def _rows():
    rows = []

    def add(name, op, kind, shape, ks, plan, edge, **kw):
        rows.append(Row(name, op, kind, shape, ks, plan[0][0], plan, edge, **kw))

    def conv(n, ci, co, h, w, ks=3, up=0, **kw):           # the forward of a plain (or element-wise upsampled) layer
        return run_conv_plan(n, ci, h, w, co, ks, (ks - 1) // 2, up, **kw)

    def dconv(n, ci, co, h, w, ks=3, **kw):                # its input gradient: a conv of gy with Cout contracted
        return run_conv_plan(n, co, h, w, ci, ks, ks - 1 - (ks - 1) // 2, 0, **kw)

    def wg(n, ci, co, h, w, ks=3, up=0, aff=False):
        return wgrad_plan(n, ci, h, w, co, ks, (ks - 1) // 2, up, aff)

    def splitk(n, ci, co, h, w, ks):
        s = splitk_plan(n, ci, co, h, w, ks)
        assert s >= 2, s
        return conv(n, ci, co, h, w, ks, ksplit=s), s

    # ---- conv_fwd_kernel: the tile kernel in its staging modes and tile geometries
    s = (2, 24, 20, 12, 40)
    add('tile_vec_32x8', 'fwd', 'plain', s, 3, conv(*s), 'vector-staged 32x8 tile: ragged in H (8 + 4) and W (32 + 8), Cin 24 -> 32 '
        'padded, ragged 20-channel tile, two column blocks', dists=True)
    s = (3, 12, 24, 20, 20)
    add('tile_vec_16x16', 'fwd', 'plain', s, 3, conv(*s), 'vector-staged 16x16 tile, ragged in H and W (16 + 4), Cin 12 -> 16')
    s = (2, 32, 32, 10, 12)
    add('tile_upsample_staged', 'fwd', 'up', s, 3, conv(*s, up=1), 'upsample-staged (10 x 12 -> 20 x 24, too narrow for the stride-2 '
        'kernels): 16x16 tiles ragged in H and W', dists=True)
    s = (1, 5, 7, 9, 37)
    add('tile_scalar_32x8', 'fwd', 'plain', s, 3, conv(*s), 'scalar-staged 32x8 tile: odd width 37 (rows not float4-aligned), ragged '
        'tiles, 5 -> 7 channels', dists=True)
    s = (5, 24, 40, 10, 10)
    add('tile_8x8x4', 'fwd', 'plain', s, 3, conv(*s), '8x8 tiles of 4 images: N = 5 leaves a tile with one image, ragged 10 x 10, '
        'three channel tiles with a ragged one (40)')
    s = (3, 6, 5, 7, 7)
    add('tile_4x4x16', 'fwd', 'plain', s, 3, conv(*s), '4x4 tiles of 16 images with N = 3, odd 7 x 7 planes, 6 -> 5 channels')
    s = (2, 24, 72, 60, 120)
    add('tile_thick', 'fwd', 'plain', s, 3, conv(*s), 'ThickCfg (64 channels x 16x8 pixels): ragged in H (60) and W (120), second '
        'channel tile ragged (72), Cin 24 -> 32', dists=True)
    s = (2, 20, 24, 12, 40)
    add('tile_masked', 'dgrad_mask', 'plain', s, 3, dconv(*s, mask=True), 'masked epilogue (input gradient x lrelu\'(x)) on ragged '
        '32x8 tiles', dists=True)
    s = (2, 72, 200, 8, 8)
    plan, k = splitk(*s, ks=3)
    add('tile_splitk_3x3', 'fwd', 'plain', s, 3, plan, 'split-K, S = 2 over 10 chunks of 8 channels (72 -> 80 padded), 13 channel '
        'tiles with a ragged one', claims=dict(ksplit=(k, 2)))
    s = (2, 250, 120, 16, 16)
    plan, k = splitk(*s, ks=3)
    add('tile_splitk_vec16', 'fwd', 'plain', s, 3, plan, 'split-K on the vector-staged 16x16 tiles, S = 4, Cin 250 -> 256, ragged '
        'channel tile (120)', claims=dict(ksplit=(k, 4)))
    s = (4, 1040, 16, 1, 1)
    plan, k = splitk(*s, ks=1)
    add('tile_splitk_cut_back', 'fwd', 'plain', s, 1, plan, 'split-K cut back: 33 chunks of 32 channels ask for S = 8, whose last '
        'workgroup would get nothing (7 x 5 >= 33) -> S = 7; 1x1 x 64-sample tile with N = 4', dists=True,
        claims=dict(ksplit=(k, 7)))
    s = (2, 24, 20, 12, 40)
    add('tile_aff', 'fwd_aff', 'plain', s, 3, [('conv_fwd_kernel<FwdCfg<3, 2, 5, 3, 0, 1>, false, false, true, false>', 2 * 2 * 2)],
        'affine on load, ragged 32x8 tiles: the zero padding must stay zero under x * s + t')
    s = (2, 24, 20, 16, 64)
    add('tile_tail', 'tail', 'plain', s, 3, [('conv_fwd_kernel<FwdCfg<3, 2, 5, 3, 0, 1>, false, false, true, true>', 2 * 2 * 2),
                                             ('conv_tail_stats_finish_kernel', 1)],
        'tail epilogue on the 32-channel tile: 4 statistics chunks per plane, channel padding on both sides', dists=True)
    s = (2, 24, 72, 16, 32)
    add('tile_tail_thick', 'tail', 'plain', s, 3, [('conv_fwd_kernel<FwdCfg<3, 4, 4, 3, 0, 1>, false, false, true, true>', 2 * 2 * 2 * 2),
                                                   ('conv_tail_stats_finish_kernel', 1)],
        'tail epilogue on ThickCfg, second channel tile ragged')
    # ---- the strip kernels (multi-tile strips open at 6144 tiles x 256 pixels x 16 channels = 200 MB per operand: out of reach
    # of a float64 reference in seconds; a workgroup walks one tile in every row here)
    s = (2, 12, 16, 24, 96)
    add('strip2_32x8', 'fwd', 'plain', s, 3, conv(*s), 'vertical strips, 32x8 tiles: three column blocks (96 is no multiple of 64, so '
        'not the rolling kernel), three tile rows, Cin 12 -> 16', dists=True)
    s = (3, 16, 16, 32, 16)
    add('strip2_16x16', 'fwd', 'plain', s, 3, conv(*s), 'vertical strips, 16x16-tile variant: two tile rows')
    s = (2, 16, 16, 16, 8)
    add('strip_upsample', 'fwd', 'up', s, 3, conv(*s, up=1), 'horizontal strip kernel, upsample-staged 16x16 tiles (16 x 8 -> 32 x 16)',
        dists=True)
    s = (2, 20, 16, 16, 64)
    add('strip_1x1', 'fwd', 'plain', s, 1, conv(*s, ks=1), 'horizontal strip kernel as a 1x1 conv: two column blocks, Cin 20 -> 32')
    # ---- the rolling-window forward kernels (conv_roll_blur.hip)
    # (launch_fwd sends only whole 32x8 tiles and whole 16-channel output blocks to the strip / rolling kernels: H = 68 - 17
    # steps - runs the tile kernel; the smallest ragged split of an H % 8 == 0 plane is 22 steps)
    s = (2, 12, 16, 88, 128)
    plan = conv(*s)
    add('roll2_three_strips', 'fwd', 'plain', s, 3, plan, '22 steps = strips of 8 + 8 + 6, two column blocks, Cin 12 -> 16 padded',
        dists=True, claims=dict(strips=(rb_plan(2, 88, 128, 0)[1:3], (3, 8))))
    s = (1, 16, 16, 8, 64)
    add('roll2_one_strip', 'fwd', 'plain', s, 3, conv(*s), 'two steps in one strip, one column: prologue and one prefetch',
        claims=dict(strips=(rb_plan(1, 8, 64, 0)[1:3], (1, 2))))
    s = (2, 16, 10, 88, 128)
    add('roll2_dgrad', 'dgrad', 'plain', s, 3, dconv(*s), 'the same kernel as an input gradient: contracts 10 -> 16 padded channels')
    s = (1, 12, 10, 132, 128)
    add('roll_blur_two_strips', 'blur', 'plain', s, 3, [('conv_fwd_roll_blur_kernel<1>', rb_plan(1, 132, 128, 1)[3])],
        'conv + LeakyReLU + blur: 33 steps = strips of 17 + 16 (each computes one step more for its neighbour\'s rows), two '
        'column blocks', dists=True, claims=dict(strips=(rb_plan(1, 132, 128, 1)[1:3], (2, 17))))
    s = (2, 16, 16, 16, 64)
    add('roll_blur_one_strip', 'blur', 'plain', s, 3, [('conv_fwd_roll_blur_kernel<1>', 2)], 'one strip of 4 steps, one column: all '
        'four image edges in one workgroup')
    s = (2, 12, 10, 68, 128)
    add('roll_rgb_sums', 'rgb', 'plain', s, 3, [('conv_fwd_roll_blur_kernel<2>', rb_plan(2, 68, 128, 0)[3]), ('rb_rgb_finish_kernel', 12 * 4)],
        'fromRGB backward folded into the input gradient: 8 workgroups\' partial sums, two strips, two column blocks', dists=True)
    s = (2, 12, 10, 68, 128)
    add('rollmod_two_strips', 'mod', 'plain', s, 3, [('conv_fwd_rollmod_kernel', 2 * 2 * 2), ('rm_stats_finish_kernel', 1)],
        'rolling modulated conv: strips of 9 + 8 steps, two column blocks, 4 statistics chunks per plane', dists=True,
        claims=dict(strips=(rb_plan(2, 68, 128, 0)[1:3], (2, 9))))         # (mod.hip rm_grid is rb_plan's rule without blur)
    # ---- weight gradients: tile kernel
    s = (2, 24, 20, 12, 40)
    add('wgrad_tile_thin', 'wgrad', 'plain', s, 3, wg(*s), 'thin 32x8 tiles ragged in H and W, 32-channel input block (24 used), '
        'two output tiles with a ragged one', dists=True)
    s = (5, 12, 20, 10, 10)
    add('wgrad_tile_8x8x4', 'wgrad', 'plain', s, 3, wg(*s), 'thin 8x8 x 4-image tiles with N = 5, ragged 10 x 10')
    s = (3, 40, 72, 12, 20)
    add('wgrad_tile_thick', 'wgrad', 'plain', s, 3, wg(*s), 'thick 8x8 tiles (64 output channels per workgroup), ragged in H, W and '
        'both channel tiles')
    s = (2, 24, 40, 12, 40)
    add('wgrad_tile_aff', 'wgrad_aff', 'plain', s, 3, wg(*s, aff=True), 'affine on load in the thick tile kernel: the padding stays '
        'zero under x * s + t', dists=True)
    # ---- weight gradients: rolling window (wgrad_roll.hip)
    s = (2, 24, 20, 68, 128)
    p = wr_plan(2, 24, 20, 68, 128)
    add('wgrad_roll_two_strips', 'wgrad', 'plain', s, 3, wg(*s), '17 steps = units of 16 + 1, two column blocks, 2 x 2 channel tiles '
        'ragged on both sides, one unit per workgroup', dists=True, claims=dict(strips=(p['strips'], 2), units_per_wg=(p['units_per_wg'], 1)))
    s = (2, 12, 10, 68, 128)
    add('wgrad_roll_aff', 'wgrad_aff', 'plain', s, 3, wg(*s, aff=True), 'affine on load in the rolling kernel, units of 16 + 1 steps',
        dists=True)
    # ---- 1x1 streaming kernels (fromRGB / toRGB)
    s = (2, 3, 16, 64, 64)
    add('pw_few_to_many', 'fwd', 'plain', s, 1, conv(*s, ks=1), 'fromRGB forward at its smallest plane (4096 pixels)', dists=True)
    add('pw_many_to_few_dgrad', 'dgrad', 'plain', s, 1, dconv(*s, ks=1), 'fromRGB input gradient')
    s = (2, 12, 3, 64, 64)
    add('pw_many_to_few', 'fwd', 'plain', s, 1, conv(*s, ks=1), 'toRGB forward, 12 of 16 channels', dists=True)
    s = (2, 3, 20, 64, 64)
    add('pw_cross_sums', 'wgrad', 'plain', s, 1, wg(*s, ks=1), 'fromRGB weight gradient: two blocks of the wide side, 16 + 4 channels',
        dists=True)
    # ---- stride-2 tile kernels (conv_s2.hip)
    s = (3, 16, 24, 20, 24)
    add('s2_down', 'fwd', 'pool', s, 3, s2_S_plan(3, 16, 24, 20, 24), 'conv + average pool, 32x8 low-resolution tiles ragged in H and '
        'W, ragged channel tile', dists=True)
    s = (2, 20, 40, 12, 16)
    add('s2_down_w16', 'fwd', 'pool', s, 3, s2_S_plan(2, 20, 40, 12, 16), '16-wide outputs on the 64-channel x 16x8 tile, ragged in H')
    s = (2, 96, 48, 20, 24)
    add('s2_up', 'fwd', 'up', s, 3, s2_T_plan(2, 96, 48, 20, 24), 'upsample + conv, 16x8 low-resolution tiles ragged in H and W, two '
        'channel tiles with a ragged one', dists=True)
    s = (2, 40, 12, 6, 48)
    add('s2_up_thin', 'fwd', 'up', s, 3, s2_T_plan(2, 40, 12, 6, 48), '16-channel x 32x8 tile, ragged in H and W, Cout 12')
    s = (2, 24, 72, 20, 24)
    add('s2_up_aff', 'fwd_aff', 'up', s, 3, s2_T_plan(2, 24, 72, 20, 24, aff=True), 'affine on load behind the folded upsample')
    s = (3, 16, 24, 20, 24)
    add('s2_up_as_pool_dgrad', 'dgrad', 'pool', s, 3, s2_T_plan(3, 24, 16, 20, 24), 'the transposed form as a pooled layer\'s input gradient')
    add('s2_wgrad_tile', 'wgrad', 'pool', s, 3, s2_wgrad_plan(3, 16, 24, 20, 24, True), '16-tap weight gradient on 16x4 tiles (width 24 '
        'is no multiple of 32), 30 slots reduced then folded, two low-channel blocks with a ragged one', dists=True)
    # ---- stride-2 rolling kernels (conv_s2_roll.hip, conv_s2_roll_blur.hip, wgrad_roll.hip)
    s = (1, 12, 20, 34, 64)
    add('s2_down_roll', 'fwd', 'pool', s, 3, s2_S_plan(1, 12, 20, 34, 64), '17 steps = strips of 9 + 8, two column blocks, channel '
        'padding on both sides', dists=True, claims=dict(strips=(sr_plan(1, 34, 64)[1:3], (2, 9))))
    s = (2, 24, 10, 34, 64)
    add('s2_up_roll', 'fwd', 'up', s, 3, s2_T_plan(2, 24, 10, 34, 64), '17 steps = strips of 9 + 8, two column blocks, 24 of 32 '
        'channels in, 10 of 16 out', dists=True, claims=dict(strips=(sr_plan(2, 34, 64)[1:3], (2, 9))))
    add('s2_down_roll_as_up_dgrad', 'dgrad', 'up', s, 3, s2_S_plan(2, 10, 24, 34, 64), 'the strided rolling kernel as an up layer\'s '
        'input gradient')
    s = (1, 24, 10, 66, 64)
    add('s2_up_roll_blur_tail', 'up_blur_tail', 'up', s, 3, [('conv_s2_up_roll_blur_kernel<0, true>', sr_plan(1, 66, 64, 16)[3]),
                                                             ('tb_stats_finish_kernel', 1)],
        'up-conv + blur + tail: 33 steps = strips of 17 + 16, two column blocks', dists=True,
        claims=dict(strips=(sr_plan(1, 66, 64, 16)[1:3], (2, 17))))
    s = (1, 10, 24, 66, 64)
    add('s2_pool_dgrad_blur_act', 'pool_dgrad_blur', 'pool', s, 3, [('conv_s2_up_roll_blur_kernel<1, false>', sr_plan(1, 66, 64, 16)[3]),
                                                                    ('tb_sum_finish_kernel', 10)],
        'pooled-conv input gradient + blur + LeakyReLU backward and the bias gradient: strips of 17 + 16 steps', dists=True)
    s = (2, 16, 16, 34, 32)
    p = w2r_plan(2, 16, 16, 34, 32)
    add('s2_wgrad_roll_up', 'wgrad', 'up', s, 3, s2_wgrad_plan(2, 16, 16, 34, 32, False), 'one low-channel block: 17 steps = units of '
        '16 + 1', claims=dict(strips=(p['strips'], 2)))
    s = (3, 24, 40, 12, 64)
    add('s2_wgrad_roll_pool', 'wgrad', 'pool', s, 3, s2_wgrad_plan(3, 24, 40, 12, 64, True), 'two low-channel blocks per workgroup '
        'with a ragged one (40), two column blocks', dists=True)
    s = (2, 24, 10, 34, 64)
    add('s2_wgrad_roll_aff', 'wgrad_aff', 'up', s, 3, s2_wgrad_plan(2, 24, 10, 34, 64, False, aff=True), 'affine on load in the 16-tap '
        'rolling weight gradient')
    # ---- the two largest rows, last
    s = (13, 24, 20, 68, 512)           # 43 MB of x, 36 MB of gy
    p = wr_plan(*s)
    add('wgrad_roll_two_units', 'wgrad', 'plain', s, 3, wg(*s), '208 units over 192 workgroups per channel-tile pair: 16 of them walk two '
        'units; two reduction stages', claims=dict(units_per_wg=(p['units_per_wg'], 2), units=(p['units'], 208)))
    s = (13, 12, 10, 68, 512)           # 22 MB of x
    add('wgrad_roll_aff_wide', 'wgrad_aff', 'plain', s, 3, wg(*s, aff=True), 'affine on load over 8 column blocks and 13 images: the '
        '(s, t) table changes between a workgroup\'s units')
    return collections.OrderedDict((r.name, r) for r in rows)


ROWS = _rows()

# kernels that only run under an environment switch read once per process: (symbol, switch); not run
UNREACHED = [
    ('conv_fwd_roll_kernel', 'GANLAB_ROLL_COL=0'),
    ('conv_fwd_roll_blur_kernel<0>', 'GANLAB_ROLL_HALF=0'),
    ('conv_s2_wgrad_roll_kernel', 'GANLAB_W2R_HALF=0'),
    ('conv_s2_down_kernel / conv_s2_up_kernel at the thin rolling shapes', 'GANLAB_S2_ROLL=0'),
    ('conv_wgrad_kernel / conv_s2_wgrad_kernel at the rolling shapes', 'GANLAB_WGRAD_ROLL=0'),
]
# kernels of the seven files that are no convolution: packing (tests/test_gpu_ops.py), and the toRGB / style pointwise kernels of
# mod.hip - by name against float64 in tests/test_gpu_mod.py (restated in tests/mod_reference.py)
NOT_CONV = ['pack_kernel', 'pack_s2_kernel', 'rm_torgb_prep_kernel', 'rm_torgb_wgrad_kernel', 'in_affine_kernel', 'rm_torgb_fwd_kernel',
            'rm_torgb_cross_kernel', 'rm_torgb_cross_finish_kernel']

# non-finite values: family -> (forward, input-gradient, weight-gradient) row and the poisoned pixel of image 0 - the last row
# and column of a tile of that kernel, in the operand's own resolution
NONFINITE = [
    ('tile_vec_32x8', (7, 31)), ('tile_masked', (7, 31)), ('wgrad_tile_thin', (7, 31)),
    ('s2_up', (7, 15)), ('s2_down_roll_as_up_dgrad', (17, 63)), ('s2_wgrad_roll_up', (31, 15)),
    ('s2_down', (15, 31)), ('s2_up_as_pool_dgrad', (7, 15)), ('s2_wgrad_tile', (7, 31)),
    ('pw_few_to_many', (0, 63)), ('pw_many_to_few_dgrad', (0, 63)), ('pw_cross_sums', (0, 63)),
]


# ==== running a row ==================================================================================================================
def norm(symbol):
    return symbol.replace('(anonymous namespace)::', '').replace(' ', '')


def run(ops, f, T):
    """(outputs on the CPU, [(symbol, workgroups)] launched) of row ``f`` on operands ``T`` (CPU fp32), exact kernels only"""
    from gan_lab_amd import _lib
    Tg = X.to_gpu(T)
    g = f.geom(ops)
    prev = ops.set_x3(False)
    try:
        with torch.no_grad():
            c0 = _lib.launch_count()
            out = f.gpu(ops, f, g, Tg, False)
            torch.cuda.synchronize()
            launches = _lib.launches_since(c0)
    finally:
        ops.set_x3(prev)
    return tuple(v.cpu() for v in out), [(norm(k or ''), n) for k, n in launches]


def plan_found(plan, launches):
    """Are the row's (symbol, workgroups) launches among ``launches`` in order?  (Weight packs and the pool behind an
    element-wise upsampled layer's input gradient stand between them.)"""
    i = 0
    for sym, grid in plan:
        sym = norm(sym)
        while i < len(launches) and not (sym in launches[i][0] and launches[i][1] == grid):
            i += 1
        if i == len(launches):
            return False
        i += 1
    return True
