"""float64 restatement of gan_lab_amd/frechet.py's definitions, numpy.

  sum  = sum_i (x_i - c),  gram = sum_i (x_i - c)(x_i - c)^T                                  (c: the pivot)
  mean = c + sum / n,      cov  = (gram - sum sum^T / n) / (n - 1)  = numpy.cov(x, rowvar=False)
  fd   = |mu_r - mu_f|^2 + tr C_r + tr C_f - 2 tr (C_r C_f)^(1/2),
  tr (C_r C_f)^(1/2) = sum sqrt(max(eigvalsh(S C_f S), 0)) with S the symmetric PSD root of C_r (similar matrices).
"""
import numpy as np


def pivoted_sums(rows, pivot):
    """(sum (D,), gram (D, D)) about ``pivot``; the difference is taken in float64 (equal to the fp32 difference whenever that
    one is exact, as for small integers)."""
    y = np.asarray(rows, dtype=np.float64) - np.asarray(pivot, dtype=np.float64)[None, :]
    return y.sum(axis=0), y.T @ y


def moments(rows):
    """(mean, cov) of the rows, two-pass in float64, n - 1 denominator."""
    x = np.asarray(rows, dtype=np.float64)
    mean = x.mean(axis=0)
    y = x - mean[None, :]
    return mean, (y.T @ y) / (x.shape[0] - 1)


def psd_root(c):
    lam, u = np.linalg.eigh(np.asarray(c, dtype=np.float64))
    return (u * np.sqrt(np.maximum(lam, 0.0))) @ u.T


def distance(mean_r, cov_r, mean_f, cov_f):
    mean_r, mean_f = np.asarray(mean_r, dtype=np.float64), np.asarray(mean_f, dtype=np.float64)
    cov_r, cov_f = np.asarray(cov_r, dtype=np.float64), np.asarray(cov_f, dtype=np.float64)
    s = psd_root(cov_r)
    a = s @ cov_f @ s
    cross = np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (a + a.T)), 0.0)).sum()
    diff = mean_r - mean_f
    mean_term = float(diff @ diff)
    trace_term = float(np.trace(cov_r) + np.trace(cov_f) - 2.0 * cross)
    return {'fd': mean_term + trace_term, 'mean_term': mean_term, 'trace_term': trace_term}


def frechet(real, fake):
    out = distance(*moments(real), *moments(fake))
    out.update(n_real=len(real), n_fake=len(fake))
    return out


def integer_rows(n, d, lo, hi, seed):
    """(n, d) float32 rows with integer entries in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)


def offset_rows(n, d, seed, offset=100.0, scale=1.0):
    """float32 rows ``offset + correlated noise``: z A with A (d, d) standard normal times ``scale`` / 2 (variances around
    scale^2 d / 4) - images with a large common offset, where E[xx^T] - mu mu^T cancels catastrophically in fp32."""
    rng = np.random.default_rng(seed)
    a = 0.5 * scale * rng.standard_normal((d, d))
    return (offset + rng.standard_normal((n, d)) @ a).astype(np.float32)
