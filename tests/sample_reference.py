"""Float64 / numpy / torch-CPU restatements for the sampling side of the ResNet GAN (gan_lab_amd/sampling.py; csrc/sample.hip):
the truncated normal (CDF, variance, inverse-CDF map, Kolmogorov-Smirnov distance), the project's Philox4x32-10 stream and its
open-interval uniform, the moving average with BigGAN's start rule, and cumulative BatchNorm statistics."""
import math

import numpy as np
import torch

SQRT2 = math.sqrt(2.0)
KS_ALPHA = 1e-6


def ks_bound(n, alpha=KS_ALPHA):
    """The Kolmogorov (DKW) bound: P(sup |F_n - F| > eps) <= 2 exp(-2 n eps^2) = alpha."""
    return math.sqrt(math.log(2.0 / alpha) / (2.0 * n))


def _erf(x):
    return torch.special.erf(torch.as_tensor(np.asarray(x, dtype=np.float64))).numpy()


def _erfinv(y):
    return torch.special.erfinv(torch.as_tensor(np.asarray(y, dtype=np.float64))).numpy()


def trunc_cdf(x, t):
    """F(x) = (erf(x / sqrt 2) + erf(t / sqrt 2)) / (2 erf(t / sqrt 2)) on [-t, t]."""
    p = math.erf(t / SQRT2)
    return (_erf(np.asarray(x, dtype=np.float64) / SQRT2) + p) / (2.0 * p)


def trunc_var(t):
    """1 - 2 t phi(t) / (2 Phi(t) - 1)."""
    phi = math.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
    return 1.0 - 2.0 * t * phi / math.erf(t / SQRT2)


def trunc_icdf(u, t):
    """x = sqrt 2 erfinv((2u - 1) erf(t / sqrt 2)), float64."""
    return SQRT2 * _erfinv((2.0 * np.asarray(u, dtype=np.float64) - 1.0) * math.erf(t / SQRT2))


def ks_distance(x, t):
    """sup_x |F_n(x) - F(x)| of the sample ``x`` against the truncated normal's CDF."""
    x = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    n = x.size
    f = trunc_cdf(x, t)
    i = np.arange(n, dtype=np.float64)
    return float(max(np.max((i + 1.0) / n - f), np.max(f - i / n)))


def philox4x32_10(ctr, seed):
    """Philox4x32-10 (Salmon et al. 2011) on counter (ctr, 0) with the 64-bit key ``seed`` -> 4 words."""
    m = 0xFFFFFFFF
    c = [ctr & m, (ctr >> 32) & m, 0, 0]
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & m, p1 & m, ((p0 >> 32) ^ c[3] ^ k1) & m, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c


def stream_uniforms(seed, offset, n):
    """The open-interval uniform of elements 0 .. n-1 of a draw at (seed, offset): element i is word i % 4 of counter
    offset + i // 4, u = ((word >> 9) + 1/2) 2^-23 in (0, 1)."""
    seed, words = seed & (2 ** 64 - 1), []
    for g in range((n + 3) // 4):
        words += philox4x32_10((offset + g) & (2 ** 64 - 1), seed)
    k = np.asarray(words[:n], dtype=np.int64) >> 9
    return (k.astype(np.float64) + 0.5) * 2.0 ** -23


def ema_replay(initial, snapshots, decay, start):
    """The averaged value after each update: ``avg_0 = initial``; update number j (1-based, after snapshot j was taken)
    ``avg_j = d_j avg_{j-1} + (1 - d_j) snapshot_j`` with ``d_j = 0`` while ``j < start`` (a copy) and ``decay`` from then on."""
    avg = np.asarray(initial, dtype=np.float64).copy()
    for j, s in enumerate(snapshots, 1):
        d = 0.0 if j < start else float(decay)
        s = np.asarray(s, dtype=np.float64)
        avg = s.copy() if d == 0.0 else d * avg + (1.0 - d) * s
    return avg


def cumulative_bn_stats(inputs):
    """running_mean, running_var, num_batches_tracked of ``torch.nn.BatchNorm2d(momentum=None)`` (float64, CPU) after it saw
    ``inputs`` (a list of (N, C, H, W) tensors) in train mode: the plain average of the batch mean / unbiased batch variance."""
    bn = torch.nn.BatchNorm2d(inputs[0].shape[1], momentum=None, affine=False).double().train()
    with torch.no_grad():
        for x in inputs:
            bn(x.detach().double().cpu())
    return bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)
