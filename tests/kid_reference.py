"""float64 restatement of gan_lab_amd/kid.py's definitions: the full kernel matrices, numpy.

  k(x, y) = (gamma x.y + coef0)^3
  mmd2    = sum_{i != i'} k(r_i, r_i') / (n (n - 1)) + sum_{j != j'} k(g_j, g_j') / (m (m - 1)) - 2 sum_{i, j} k(r_i, g_j) / (n m)
  kid     = mmd2 of the whole sets; the block statistics are the mmd2 of B = min(n, m) // block pairs of contiguous blocks, their
            mean (added in block order) and their standard deviation (n - 1 denominator).
Within a set the term i' == i is left out by INDEX: a duplicate row elsewhere counts.  Sums of many terms use math.fsum (the
exactly rounded sum); on small integer rows with gamma a power of two every term and every sum is exact anyway.
"""
import math

import numpy as np


def kernel(a, b, gamma, coef0=1.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    t = gamma * (a @ b.T) + coef0
    return t * t * t


def row_sums(real, fake, gamma, coef0=1.0):
    """{'real_real' (n,), 'fake_fake' (m,), 'real_fake' (n,)} float64."""
    out = {}
    for name, x in (('real_real', real), ('fake_fake', fake)):
        k = kernel(x, x, gamma, coef0)
        k[np.arange(len(x)), np.arange(len(x))] = 0.0           # the row itself, by index
        out[name] = np.array([math.fsum(row) for row in k])
    out['real_fake'] = np.array([math.fsum(row) for row in kernel(real, fake, gamma, coef0)])
    return out


def mmd2(real, fake, gamma, coef0=1.0):
    n, m = len(real), len(fake)
    s = row_sums(real, fake, gamma, coef0)
    rr, ff, rf = (math.fsum(s[p]) for p in ('real_real', 'fake_fake', 'real_fake'))
    return rr / (n * (n - 1)) + ff / (m * (m - 1)) - 2.0 * rf / (n * m)


def kid(real, fake, block, gamma=None, coef0=1.0):
    n, m = len(real), len(fake)
    gamma = 1.0 / real.shape[1] if gamma is None else gamma
    nb = min(n, m) // block
    per_block = [mmd2(real[b * block:(b + 1) * block], fake[b * block:(b + 1) * block], gamma, coef0) for b in range(nb)]
    mean = std = None
    if nb:
        total = per_block[0]
        for v in per_block[1:]:
            total = total + v
        mean = total / nb
    if nb > 1:
        total = (per_block[0] - mean) * (per_block[0] - mean)
        for v in per_block[1:]:
            total = total + (v - mean) * (v - mean)
        std = math.sqrt(total / (nb - 1))
    return {'kid': mmd2(real, fake, gamma, coef0), 'kid_block_mean': mean, 'kid_block_std': std, 'blocks': nb, 'block': block,
            'n_real': n, 'n_fake': m}


def integer_rows(n, d, lo, hi, seed):
    """(n, d) float32 rows with integer entries in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)
