"""float64 restatement of gan_lab_amd/prdc.py's definitions: brute force over all pairs, numpy.

Real rows r_i, generated rows g_j; squared Euclidean distances throughout, ``<=`` counts as inside.
  rad_r[i]  = k-th smallest |r_i - r_i'|^2 over i' != i (self excluded by INDEX: a duplicate row elsewhere counts)
  precision = share of j with some i: |g_j - r_i|^2 <= rad_r[i]          recall = share of i with some j: |r_i - g_j|^2 <= rad_g[j]
  density   = #{(j, i): |g_j - r_i|^2 <= rad_r[i]} / (k M)               coverage = share of i with min_j |r_i - g_j|^2 <= rad_r[i]
  nearest real of g_j = argmin_i |g_j - r_i|^2, the lowest index of a tie.
"""
import numpy as np


def sqdist(a, b, rows_per_block=16):
    """(len(a), len(b)) float64 squared distances, as sums of squared differences (exact for small integers, exactly 0 for
    duplicates)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    for i in range(0, a.shape[0], rows_per_block):
        diff = a[i:i + rows_per_block, None, :] - b[None, :, :]
        out[i:i + rows_per_block] = np.einsum('ijk,ijk->ij', diff, diff)
    return out


def knn_lists(x, k, d=None):
    """(n, k): the k smallest squared distances of every row to the other rows, ascending."""
    d = sqdist(x, x) if d is None else d.copy()
    n = d.shape[0]
    assert 1 <= k < n
    d = d.copy()
    d[np.arange(n), np.arange(n)] = np.inf          # the row itself, by index
    return np.sort(d, axis=1)[:, :k]


def cross(d, radii, radius_of):
    """Of a (queries, keys) distance matrix: (count of keys inside per query, smallest distance, its lowest index)."""
    radii = np.asarray(radii, dtype=np.float64)
    inside = d <= (radii[None, :] if radius_of == 'key' else radii[:, None])
    return inside.sum(axis=1), d.min(axis=1), d.argmin(axis=1)


def prdc(real, fake, k, parts=False):
    d_rr, d_ff, d_fr = sqdist(real, real), sqdist(fake, fake), sqdist(fake, real)
    d_rf = np.ascontiguousarray(d_fr.T)
    n, m = d_rf.shape
    lists_r, lists_f = knn_lists(real, k, d_rr), knn_lists(fake, k, d_ff)
    rad_r, rad_f = lists_r[:, -1], lists_f[:, -1]
    c_fr, min_fr, arg_fr = cross(d_fr, rad_r, 'key')
    c_rf, min_rf, arg_rf = cross(d_rf, rad_f, 'key')
    c_cov, _, _ = cross(d_rf, rad_r, 'query')
    out = {'precision': int((c_fr > 0).sum()) / m, 'recall': int((c_rf > 0).sum()) / n,
           'density': int(c_fr.sum()) / (k * m), 'coverage': int((c_cov > 0).sum()) / n, 'k': k, 'n_real': n, 'n_fake': m}
    if not parts:
        return out
    return out, dict(d_rr=d_rr, d_ff=d_ff, d_fr=d_fr, d_rf=d_rf, lists_r=lists_r, lists_f=lists_f, rad_r=rad_r, rad_f=rad_f,
                     c_fr=c_fr, min_fr=min_fr, arg_fr=arg_fr, c_rf=c_rf, min_rf=min_rf, arg_rf=arg_rf, c_cov=c_cov)


def integer_rows(n, d, lo, hi, seed):
    """(n, d) float32 rows with integer entries in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)


def manifold_rows(n_real, n_fake, d, seed):
    """Rows on a 4-dimensional manifold of R^d: t @ A + 0.01 noise with A (4, d) scaled by 1/2; reals t ~ N(0, I), fakes
    t ~ N(0.8, 0.7^2 I).  float32."""
    rng = np.random.default_rng(seed)
    a = 0.5 * rng.standard_normal((4, d))
    real = rng.standard_normal((n_real, 4)) @ a + 0.01 * rng.standard_normal((n_real, d))
    fake = (0.8 + 0.7 * rng.standard_normal((n_fake, 4))) @ a + 0.01 * rng.standard_normal((n_fake, d))
    return real.astype(np.float32), fake.astype(np.float32)
