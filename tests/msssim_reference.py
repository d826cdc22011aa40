"""Numpy restatement of multi-scale structural similarity (MS-SSIM; Wang, Simoncelli and Bovik 2003) between pairs of images, as
the ProGAN paper uses it to judge sample diversity and as DESIGN.md 4.8 defines it.  A test helper: plain numpy, no GPU, nothing
of the package imported.  ``dtype=np.float64`` is the definition; ``dtype=np.float32`` runs the same steps in the kernel's number
format and is the yardstick of the GPU tests (what fp32 arithmetic alone costs, whatever the order of the sums).

    window   side S: s = min(11, S) taps, sigma = 1.5 s / 11, g[k] ~ exp(-(k - (s-1)/2)^2 / (2 sigma^2)), sum 1 (float64, then
             rounded to ``dtype``); applied along x, then along y, valid mode: the output side is S - s + 1
    level    mu_a, mu_b = g*a, g*b; s_aa = g*(a a) - mu_a^2, s_bb likewise, s_ab = g*(a b) - mu_a mu_b
             v1 = 2 s_ab + C2, v2 = s_aa + s_bb + C2, cs = v1 / v2, ssim = (2 mu_a mu_b + C1) v1 / ((mu_a^2 + mu_b^2 + C1) v2)
             CS_i, SSIM_i = max(mean over channels and pixels, 0)
    next     the aligned 2x2 mean ((x00 + x01) + (x10 + x11)) / 4
    pair     prod_{i<4} CS_i^w_i x SSIM_4^w_4, five levels; the metric is the mean over pairs
"""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LEVELS = len(WEIGHTS)
MAX_WINDOW = 11


def window(side):
    """The float64 Gaussian window of a level of side ``side``."""
    s = min(MAX_WINDOW, int(side))
    sigma = 1.5 * s / MAX_WINDOW
    k = np.arange(s, dtype=np.float64)
    g = np.exp(-(k - (s - 1) / 2.) ** 2 / (2. * sigma * sigma))
    return g / g.sum()


def blur(x, g):
    """``g (x) g`` over the last two axes in valid mode: along x first, then along y, taps in order."""
    s = len(g)
    w = x.shape[-1] - s + 1
    t = g[0] * x[..., :, 0:w]
    for k in range(1, s):
        t = t + g[k] * x[..., :, k:k + w]
    h = t.shape[-2] - s + 1
    out = g[0] * t[..., 0:h, :]
    for k in range(1, s):
        out = out + g[k] * t[..., k:k + h, :]
    return out


def pool(x):
    """The next level: the aligned 2x2 mean, summed in this order."""
    return ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + (x[..., 1::2, 0::2] + x[..., 1::2, 1::2])) * x.dtype.type(0.25)


def constants(data_range=2.0):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def level_maps(a, b, data_range=2.0):
    """(cs, ssim) maps of one level, each (P, 3, O, O), in the dtype of ``a``."""
    dt = a.dtype.type
    c1, c2 = (dt(v) for v in constants(data_range))
    g = window(a.shape[-1]).astype(a.dtype)
    mu_a, mu_b = blur(a, g), blur(b, g)
    s_aa = blur(a * a, g) - mu_a * mu_a
    s_bb = blur(b * b, g) - mu_b * mu_b
    s_ab = blur(a * b, g) - mu_a * mu_b
    v1 = dt(2) * s_ab + c2
    v2 = s_aa + s_bb + c2
    cs = v1 / v2
    ssim = ((dt(2) * mu_a * mu_b + c1) * v1) / ((mu_a * mu_a + mu_b * mu_b + c1) * v2)
    return cs, ssim


def pyramid(x, levels=LEVELS):
    out = [np.asarray(x)]
    for _ in range(levels - 1):
        out.append(pool(out[-1]))
    return out


def raw_table(a, b, data_range=2.0, dtype=np.float64):
    """(P, 5, 2) per-pair, per-level means of (cs, ssim) BEFORE the clamp.  The maps are computed in ``dtype``; their means are
    always accumulated in float64 (the kernel's partial sums are fp64 too)."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    if a.shape != b.shape or a.ndim != 4 or a.shape[1] != 3 or a.shape[2] != a.shape[3] or a.shape[2] < 16 or \
            a.shape[2] & (a.shape[2] - 1):
        raise ValueError(f'msssim reference: needs two (P, 3, R, R) batches, R a power of two >= 16, got {a.shape}, {b.shape}')
    out = np.empty((a.shape[0], LEVELS, 2), dtype=np.float64)
    for i in range(LEVELS):
        cs, ssim = level_maps(a, b, data_range)
        out[:, i, 0] = cs.mean(axis=(1, 2, 3), dtype=np.float64)
        out[:, i, 1] = ssim.mean(axis=(1, 2, 3), dtype=np.float64)
        if i + 1 < LEVELS:
            a, b = pool(a), pool(b)
    return out


def table(a, b, data_range=2.0, dtype=np.float64):
    """(P, 5, 2): (CS_i, SSIM_i), clamped below at 0."""
    return np.maximum(raw_table(a, b, data_range, dtype), 0.)


def combine(tab):
    """Per-pair MS-SSIM of a (P, 5, 2) clamped table, float64."""
    w = np.asarray(WEIGHTS)
    return np.prod(tab[:, :LEVELS - 1, 0] ** w[:LEVELS - 1], axis=1) * tab[:, LEVELS - 1, 1] ** w[LEVELS - 1]


def per_pair(a, b, data_range=2.0, dtype=np.float64):
    return combine(table(a, b, data_range, dtype))


def msssim(a, b, data_range=2.0, dtype=np.float64):
    """{'msssim', 'pairs', 'per_level'} like ``MultiScaleSSIM.result()``."""
    tab = table(a, b, data_range, dtype)
    return {'msssim': float(np.mean(combine(tab))), 'pairs': int(tab.shape[0]),
            'per_level': [[float(v) for v in tab[:, :LEVELS - 1, 0].mean(axis=0)], float(tab[:, LEVELS - 1, 1].mean())]}


def of_set(x, data_range=2.0, dtype=np.float64):
    """The metric of an image set: pairs are images (2j, 2j + 1), in order."""
    x = np.asarray(x)
    return msssim(x[0::2], x[1::2], data_range, dtype)


def sample_pairs(kind, pairs, res, seed):
    """The tests' three kinds of pairs, float32: 'noise' (two independent unit-variance noise images), 'smooth' (two smooth
    images, the same few low frequencies with different phases, plus a little noise each) and 'near' (noise a, b = a + 0.02
    noise: the only kind whose every CS_i stays far from the clamp)."""
    rng = np.random.default_rng(seed)
    shape = (pairs, 3, res, res)
    if kind == 'noise':
        a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    elif kind == 'near':
        a = rng.standard_normal(shape)
        b = a + 0.02 * rng.standard_normal(shape)
    elif kind == 'smooth':
        t = np.arange(res) / res
        imgs = []
        for _ in range(2):
            acc = np.zeros(shape)
            for f in (1, 2, 3):
                py, px = rng.uniform(0, 2 * np.pi, (2,) + shape[:2] + (1, 1))
                acc += np.sin(2 * np.pi * f * t[:, None] + py) * np.cos(2 * np.pi * f * t[None, :] + px) / f
            imgs.append(0.5 * acc + 0.1 * rng.standard_normal(shape))
        a, b = imgs
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
