"""Numpy restatement of the radial power-spectrum metric as DESIGN.md 4.9 defines it.  A test helper: no GPU, nothing of the
package imported.  ``profiles`` (float64, full ``np.fft.fft2``, no Hermitian shortcut) is the definition; ``profiles_fp32`` runs
the same steps in the kernel's number format (``torch.fft.fft2`` on a CPU complex64 tensor, bin sums in float64 like the kernel's)
and is the yardstick of the GPU tests: what an fp32 transform alone costs, whatever its factorisation.

    window   'hann': w[i] = 0.5 - 0.5 cos(2 pi i / R) (periodic); 'none': w = 1; W = (sum_i w[i]^2 / R)^2
    power    P[u, v] = 1/3 sum_c |fft2(x_c w w^T)[u, v]|^2 / (R^2 W)
    bins     signed frequencies ku, kv in [-R/2, R/2); bin k iff (2k-1)^2 <= 4 (ku^2 + kv^2) < (2k+1)^2, i.e. k = the number of
             j >= 1 with (2j-1)^2 <= 4 (ku^2 + kv^2): integers only.  Bins 0 .. R/2 are kept.
    A[k]     the mean of P over bin k;  S[k] = the mean of A_n[k] over the images;  dB[k] = 10 log10(max(S[k], 1e-30))
    spectrum sqrt(mean_{k=1..R/2} (dB_fake[k] - dB_real[k])^2);  hf: the same over k = R/4+1 .. R/2
"""
import numpy as np

DB_FLOOR = 1e-30
WINDOWS = ('hann', 'none')


def window(res, kind='hann'):
    """(w as float64, W)."""
    if kind == 'hann':
        w = 0.5 - 0.5 * np.cos(2. * np.pi * np.arange(res) / res)
    elif kind == 'none':
        w = np.ones(res)
    else:
        raise ValueError(kind)
    return w, float((w * w).sum() / res) ** 2


def bin_index(res):
    """(R, R) int array in fft order: the bin of every coefficient (values above R/2 are the dropped corners)."""
    k = np.arange(res, dtype=np.int64)
    k = np.where(k < res // 2, k, k - res)                       # [-R/2, R/2)
    s4 = 4 * (k[:, None] ** 2 + k[None, :] ** 2)
    thresholds = (2 * np.arange(1, 2 * res, dtype=np.int64) - 1) ** 2
    return np.searchsorted(thresholds, s4, side='right')


def bin_counts(res):
    return np.bincount(bin_index(res).ravel())[:res // 2 + 1]


def _radial(power, res):
    """(N, R, R) float64 power -> (N, R/2 + 1) bin means."""
    idx = bin_index(res).ravel()
    keep = idx <= res // 2
    cnt = np.bincount(idx[keep], minlength=res // 2 + 1).astype(np.float64)
    flat = power.reshape(len(power), -1)
    return np.stack([np.bincount(idx[keep], weights=p[keep], minlength=res // 2 + 1) / cnt for p in flat])


def profiles(x, kind='hann'):
    """Per-image profiles A_n[k] of a (N, 3, R, R) array: (N, R/2 + 1) float64.  The definition."""
    x = np.asarray(x, dtype=np.float64)
    res = x.shape[-1]
    w, W = window(res, kind)
    f = np.fft.fft2(x * w[:, None] * w[None, :])
    power = (f.real ** 2 + f.imag ** 2).sum(axis=1) / (3. * res * res * W)
    return _radial(power, res)


def profiles_fp32(x, kind='hann'):
    """The same steps with the window product and the transform in fp32 (torch, CPU)."""
    import torch
    x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    res = x.shape[-1]
    w64, W = window(res, kind)
    w = torch.as_tensor(w64.astype(np.float32))
    f = torch.fft.fft2((x * w[None, None, None, :]) * w[None, None, :, None])
    assert f.dtype == torch.complex64
    power = (f.real * f.real + f.imag * f.imag).to(torch.float64).sum(dim=1).numpy() / (3. * res * res * W)
    return _radial(power, res)


def decibels(profile_rows):
    """(N, bins) per-image profiles -> (S, dB) of the set."""
    s = np.asarray(profile_rows, dtype=np.float64).mean(axis=0)
    return s, 10. * np.log10(np.maximum(s, DB_FLOOR))


def distance(fake_rows, real_rows):
    """{'spectrum', 'hf', 'fake_db', 'real_db'} from the per-image profiles of the two sets."""
    _, fd = decibels(fake_rows)
    _, rd = decibels(real_rows)
    nb = len(fd)
    res = 2 * (nb - 1)
    d2 = (fd - rd) ** 2
    return {'spectrum': float(np.sqrt(d2[1:].mean())), 'hf': float(np.sqrt(d2[res // 4 + 1:].mean())), 'fake_db': fd,
            'real_db': rd}


def tone(res, ku, kv, channel=0):
    """One (3, R, R) image: cos(2 pi (ku i + kv j) / R) in ``channel`` (i the row, j the column), zero elsewhere."""
    i = np.arange(res)
    x = np.zeros((3, res, res), dtype=np.float32)
    x[channel] = np.cos(2. * np.pi * ((ku * i[:, None] + kv * i[None, :]) % res) / res).astype(np.float32)
    return x


def sample(kind, n, res, seed):
    """(n, 3, res, res) float32 test images.
    'noise'    white Gaussian noise, unit variance
    'natural'  white noise shaped by 1/r in amplitude (r the radius in cycles; DC kept at the r = 1 level), scaled to max |x| = 1:
               the 1/f^2 power law of natural images
    'tone'     image m is ``tone(res, ku, kv, m % 3)`` with (ku, kv) = (1 + m % (res/2 - 1), 1 + (3 m) % (res/2 - 1))"""
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.standard_normal((n, 3, res, res)).astype(np.float32)
    if kind == 'natural':
        k = np.fft.fftfreq(res) * res
        r = np.sqrt(k[:, None] ** 2 + k[None, :] ** 2)
        x = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, 3, res, res))) / np.maximum(r, 1.)).real
        return (x / np.abs(x).max()).astype(np.float32)
    if kind == 'tone':
        h = res // 2 - 1
        return np.stack([tone(res, 1 + m % h, 1 + (3 * m) % h, m % 3) for m in range(n)])
    raise ValueError(kind)
