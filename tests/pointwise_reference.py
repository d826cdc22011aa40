"""Float64 / numpy / torch-CPU restatements of the oldest kernels of the library (csrc/pointwise.hip and the draws of
csrc/cond.hip and csrc/swd.hip): the Philox stream's consumers element by element, the Adam recurrence with a forward error
bound, and the scalar losses, reductions and elementwise ops as float64 ``torch`` expressions that autograd differentiates.

The draws.  A consumer at (seed, offset) reads the four 32-bit words of counters ``offset + j``, j = 0, 1, ... (64-bit wrap,
low word in c[0], high word in c[1], c[2] = c[3] = 0), under the 64-bit key ``seed``.  ``*_counters`` gives the j that a
restated draw reads, as exact Python integers: the stream ledger of ``gan_lab_amd/rng.py`` must step over exactly those.

Perturbed forms (``variant=``) are the mistakes the tests must catch; the tests compare them with the right form on the CPU."""
import math

import numpy as np
import torch

from sample_reference import philox4x32_10

M64 = 2 ** 64 - 1
SWD_DESC = 147
ADA_COUNTERS = 8


# ---- the stream ----------------------------------------------------------------------------------------------------------------
def stream_words(seed, offset, count, drop_high=False):
    """(count, 4) uint64 array: the words of counters (offset + j) mod 2^64, j < count.  ``drop_high``: the mistake of a
    32-bit counter (the high word never reaches the cipher)."""
    ctr = np.uint64(offset & M64) + np.arange(count, dtype=np.uint64)          # wraps modulo 2^64
    if drop_high:
        ctr = ctr & np.uint64(0xFFFFFFFF)
    w = philox4x32_10(ctr, seed & M64)
    return np.stack([np.broadcast_to(np.asarray(x, dtype=np.uint64), ctr.shape) for x in w], axis=1)


def randn_counters(n):
    return (n + 3) // 4


def randn_reference(seed, offset, n, variant=None):
    """Element 4i + 2k is rad cos, element 4i + 2k + 1 is rad sin, of words (2k, 2k + 1) of counter offset + i:
    u1 = fl32(fl32(w) + 1) 2^-32 in (0, 1], u2 = fl32(w') 2^-32, rad = sqrt(-2 ln u1), angle 2 pi u2.  The two integer
    conversions and the addition are exact IEEE fp32 operations and are mirrored; everything after them is float64.
    ``variant``: 'swap' (sin / cos exchanged), 'drop_high' (32-bit counter), 'floor4' (n >> 2 groups: the tail is lost,
    its elements come back as NaN)."""
    n4 = n >> 2 if variant == 'floor4' else (n + 3) >> 2
    out = np.full(4 * ((n + 3) >> 2), np.nan)
    if n4:
        w = stream_words(seed, offset, n4, drop_high=variant == 'drop_high')
        for k in range(2):
            u1 = (w[:, 2 * k].astype(np.float32) + np.float32(1.0)).astype(np.float64) * 2.0 ** -32
            u2 = w[:, 2 * k + 1].astype(np.float32).astype(np.float64) * 2.0 ** -32
            rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * math.pi * u2
            a, b = rad * np.cos(ang), rad * np.sin(ang)
            if variant == 'swap':
                a, b = b, a
            out[2 * k:4 * n4:4], out[2 * k + 1:4 * n4:4] = a, b
    return out[:n]


def randint_counters(n):
    return (n + 3) // 4


def randint_reference(seed, offset, n, high):
    """Element e is word e % 4 of counter offset + e // 4 scaled into [0, high): ((w >> 8) high) >> 24."""
    w = stream_words(seed, offset, randint_counters(n)).reshape(-1)[:n]
    return (((w >> np.uint64(8)) * np.uint64(high)) >> np.uint64(24)).astype(np.int64)


def swd_positions_counters(n_images, n_per_image):
    return n_images * ((2 * n_per_image + 3) // 4)


def swd_positions_reference(seed, offset, n_images, n_per_image, size):
    """(n_images, n_per_image, 2): image i takes ceil(2n / 4) counters from offset + i ceil(2n / 4); word e of its block is
    coordinate e of its (n, 2) rows, 3 + (((w >> 8) (S - 6)) >> 24) in [3, S - 4]."""
    per = (2 * n_per_image + 3) // 4
    w = stream_words(seed, offset, n_images * per).reshape(n_images, 4 * per)[:, :2 * n_per_image]
    v = ((w >> np.uint64(8)) * np.uint64(size - 6)) >> np.uint64(24)
    return (3 + v.astype(np.int64)).reshape(n_images, n_per_image, 2)


def swd_directions_counters(n_dirs):
    return SWD_DESC * n_dirs


def swd_directions_reference(seed, offset, n_dirs):
    """(n_dirs, 147) float64: element e of direction d is sqrt(-2 ln u1) cos(2 pi u2) of words 0 and 1 of counter
    offset + 147 d + e with the 24-bit uniforms u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24; rows scaled to unit norm."""
    w = stream_words(seed, offset, SWD_DESC * n_dirs)
    u1 = ((w[:, 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w[:, 1] >> np.uint64(8)).astype(np.float64)
    z = (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2 * 2.0 ** -24)).reshape(n_dirs, SWD_DESC)
    return z / np.sqrt((z * z).sum(axis=1, keepdims=True))


# Counters per draw of every consumer of the process stream (arguments as ``gan_lab_amd.rng`` takes them).  trunc_randn,
# diffaug_params and ada_params are restated in sample_reference.stream_uniforms (word i % 4 of counter offset + i // 4), in
# test_gpu_diffaug (counters offset + 2n, offset + 2n + 1) and in test_gpu_ada (offset + 8n .. offset + 8n + 7).
CONSUMED = {
    'randn': lambda n: randn_counters(n),
    'trunc_randn': lambda n: (n + 3) // 4,
    'randint': lambda n: randint_counters(n),
    'augment_params': lambda n: 2 * n,
    'ada_params': lambda n: ADA_COUNTERS * n,
    'swd_positions': lambda n_images, n_per_image: swd_positions_counters(n_images, n_per_image),
    'swd_directions': lambda n_dirs: swd_directions_counters(n_dirs),
}


def counter_range(offset, count):
    """The counters offset .. offset + count - 1 modulo 2^64, as a set of exact integers."""
    return {(offset + j) & M64 for j in range(count)}


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24           # unit roundoff of fp32


def f32(x):
    """The float32 nearest to ``x``, as a Python float: what a kernel receives for a scalar argument."""
    return float(np.float32(x))


def adam_reference(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, variant=None, err=None):
    """One step of ``adam_kernel``'s recurrence in float64 (scalars as the kernel receives them: float32 values):
        g' = g + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
    -> (p', m', v').  ``variant``: 'swap_betas', 'swap_bc', 'wd_on_p' (decoupled decay: p shrinks by lr wd p, g untouched).
    ``err``: dict(p, m, v) of running bounds on |fp32 kernel - this|, advanced by one step (a forward error analysis with
    u = 2^-24 per fp32 operation; FMA contraction only removes roundings):
        g':  2 u (|g| + |wd p|) + wd e_p  (0 when wd = 0: g' is g)
        m':  b1 e_m + (1 - b1) e_g + 3 u (|b1 m| + |(1 - b1) g'|)
        v':  b2 e_v + (1 - b2) 2 |g'| e_g + 4 u (b2 v + (1 - b2) g'^2)
        step = m' s / den with s = lr / bc1 (1 rounding), den = sqrt(v') rsqrt(bc2) + eps (sqrt 1, rsqrt 2, product 1, sum 1),
        one product and one quotient: 8 u |step| + (s / den) e_m + |step| e_v / (2 v') (sqrt halves the relative error of v';
        the term vanishes with v')
        p':  e_p + e_step + u |p'|."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    if variant == 'swap_betas':
        b1, b2 = b2, b1
    if variant == 'swap_bc':
        bc1, bc2 = bc2, bc1
    gi = g + wd * p if (wd != 0.0 and variant != 'wd_on_p') else g
    mi = b1 * m + (1.0 - b1) * gi
    vi = b2 * v + (1.0 - b2) * gi * gi
    s = lr / bc1
    den = np.sqrt(vi) / math.sqrt(bc2) + eps
    step = s * mi / den
    pn = p - step
    if variant == 'wd_on_p':
        pn = pn - lr * wd * p
    if err is not None:
        u = EPS32
        eg = 2 * u * (np.abs(g) + np.abs(wd * p)) + wd * err['p'] if wd != 0.0 else np.zeros_like(g)
        em = b1 * err['m'] + (1.0 - b1) * eg + 3 * u * (np.abs(b1 * m) + np.abs((1.0 - b1) * gi))
        ev = b2 * err['v'] + (1.0 - b2) * 2 * np.abs(gi) * eg + 4 * u * (b2 * v + (1.0 - b2) * gi * gi)
        rel_v = np.divide(ev, 2.0 * vi, out=np.zeros_like(vi), where=vi > 0)
        es = 8 * u * np.abs(step) + (s / den) * em + np.abs(step) * rel_v
        err['p'], err['m'], err['v'] = err['p'] + es + u * np.abs(pn), em, ev
    return pn, mi, vi


def adam_run(p, grads, lr, b1, b2, eps, wd, variant=None):
    """``len(grads)`` steps from zero moments -> (p, m, v, err).  The bias corrections are 1 - beta^t of the betas as given
    (Python floats, as ``optim.FusedAdam`` computes them) and only then rounded to float32, like every other scalar."""
    bcs = [(f32(1 - b1 ** t), f32(1 - b2 ** t)) for t in range(1, len(grads) + 1)]
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    p = np.asarray(p, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    err = dict(p=np.zeros_like(p), m=np.zeros_like(p), v=np.zeros_like(p))
    for g, (bc1, bc2) in zip(grads, bcs):
        p, m, v = adam_reference(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, variant, err)
    return p, m, v, err


def adam_inputs(n, steps=5, seed=41):
    """Parameters and ``steps`` gradients (float32 values): normal draws with, at elements 5 mod 7 / 3 mod 11, exact zeros / entries
    near 1e-12 in EVERY step - there v stays 0 or ~1e-27 and ``eps`` decides the step."""
    gen = np.random.default_rng(seed + n)
    p = gen.standard_normal(n).astype(np.float32)
    grads = []
    for _ in range(steps):
        g = gen.standard_normal(n).astype(np.float32)
        g[5::7] = 0.0
        g[3::11] = (1e-12 * (1.0 + gen.random(g[3::11].shape))).astype(np.float32)
        grads.append(g)
    return p, grads


# ---- losses, reductions and elementwise ops as float64 torch expressions ---------------------------------------------------------
def bce_logits_mean(x, target):
    """mean(log(1 + exp(x)) - x t), the kernel's max(x, 0) - x t + log(1 + exp(-|x|)); written with ``logaddexp`` because
    autograd differentiates max and |.| to a subgradient at x = 0, where the loss is smooth (sigmoid(0) - t)."""
    return (torch.logaddexp(x, torch.zeros_like(x)) - x * target).mean()


def hinge_mean(x, a, b):
    """mean(relu(a + b x)); the gradient on the kink is 0 (``torch.relu``)."""
    return torch.relu(a + b * x).mean()


def chnorm_penalty(g, gamma, scale):
    """scale sum_{n, hw} (||g[n, :, hw]||_2 - gamma)^2; the gradient at a zero vector is 0 (``torch.norm``)."""
    return scale * ((g.norm(2, dim=1) - gamma) ** 2).sum()


def mbstd_stat(x, gs, eps=1e-8):
    """(B / gs,): for the group of samples g gs .. g gs + gs - 1, the mean over features of sqrt(unbiased variance + eps)."""
    y = x.reshape(x.shape[0] // gs, gs, -1)
    d = y - y.mean(dim=1, keepdim=True)
    return torch.sqrt((d * d).sum(dim=1) / (gs - 1) + eps).mean(dim=1)


def sum_all(x, scale=1.0):
    return scale * x.sum()


def sumsq_all(x, scale=1.0):
    return scale * (x * x).sum()


def axpby(x, y, a, b):
    return a * x + b * y


def lerp_rows(a, b, t):
    w = t.reshape(-1, *([1] * (a.dim() - 1)))
    return w * a + (1.0 - w) * b


def chan_affine(x, scale=None, shift=None):
    shape = (1, -1) + (1,) * (x.dim() - 2)
    y = x if scale is None else x * scale.reshape(shape)
    return y if shift is None else y + shift.reshape(shape)


def fd_gradient(fn, x, h=1e-6):
    """Central finite differences of the scalar ``fn`` at the float64 tensor ``x``."""
    g = torch.zeros_like(x)
    flat, gf = x.detach().clone().reshape(-1), g.reshape(-1)
    with torch.no_grad():
        for i in range(flat.numel()):
            keep = flat[i].item()
            flat[i] = keep + h
            hi = fn(flat.reshape(x.shape)).item()
            flat[i] = keep - h
            lo = fn(flat.reshape(x.shape)).item()
            flat[i] = keep
            gf[i] = (hi - lo) / (2 * h)
    return g
