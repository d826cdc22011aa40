"""The perceptual path length's three ops and ``path_length`` (gan_lab_amd/ppl.py, csrc/ppl.hip) restated in plain
torch and numpy on the CPU, parameterised by dtype: float64 is the truth the GPU tests measure against, float32 the yardstick - the
same formulas with every operation rounded to fp32, which is what a plain implementation would give.  Nothing here imports the
package."""
import numpy as np
import torch

PARALLEL = 2.0 ** -30          # |bh - d ah|^2 below this: the rows count as parallel / antipodal


# ---- the uniform draw -------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, seed):
    """Philox4x32-10 (Salmon et al. 2011) on the counter (ctr low, ctr high, 0, 0) under the 64-bit key ``seed`` -> 4 words."""
    m = 0xFFFFFFFF
    c = [ctr & m, (ctr >> 32) & m, 0, 0]
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & m, p1 & m, ((p0 >> 32) ^ c[3] ^ k1) & m, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c


def uniforms(seed, offset, n):
    """(n,) float64: row i's draw is (word 0 of counter offset + i >> 8) 2^-24 in [0, 1) - exact in fp32."""
    seed &= 2 ** 64 - 1
    return np.array([(philox4x32_10((offset + i) & (2 ** 64 - 1), seed)[0] >> 8) * 2.0 ** -24 for i in range(n)])


def substream(seed, k):
    return (int(seed) * 0x9E3779B97F4A7C15 + (int(k) + 1) * 0xD1B54A32D192ED03 + 0x50504C) & (2 ** 64 - 1)


# ---- the three ops ------------------------------------------------------------------------------------------------------------
def endpoints(a, b, t, eps, mode, dtype=torch.float64):
    """(2, N, D) in ``dtype``: the points at ``t`` (N,) and ``t + eps`` of the paths from the rows of a to the rows of b."""
    a, b = a.detach().cpu().to(dtype), b.detach().cpu().to(dtype)
    t = torch.as_tensor(np.asarray(t), dtype=dtype)
    ts = torch.stack([t, t + torch.tensor(eps, dtype=dtype)]).unsqueeze(-1)          # (2, N, 1)
    if mode == 'lerp':
        return a + (b - a) * ts
    assert mode == 'slerp'
    d_len = a.shape[1]
    root = torch.tensor(float(d_len), dtype=dtype).sqrt()
    na, nb = (a * a).sum(1, keepdim=True).sqrt(), (b * b).sum(1, keepdim=True).sqrt()
    ah = torch.where(na > 0, a / torch.where(na > 0, na, torch.ones_like(na)), a)
    bh = torch.where(nb > 0, b / torch.where(nb > 0, nb, torch.ones_like(nb)), torch.zeros_like(b))
    d = (ah * bh).sum(1, keepdim=True).clamp(-1, 1)
    c = bh - d * ah
    nc2 = (c * c).sum(1, keepdim=True)
    flat = (nc2 < PARALLEL) | (na <= 0) | (nb <= 0)
    ch = c / torch.where(flat, torch.ones_like(nc2), nc2).sqrt()
    p = ts * torch.acos(d)
    r = ah * torch.cos(p) + ch * torch.sin(p)
    out = r / (r * r).sum(-1, keepdim=True).sqrt() * root
    return torch.where(flat, (ah * root).expand_as(out), out)


def row_sqdist(x, y, dtype=torch.float64):
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    return ((x - y) ** 2).sum(1)


def virtual_index(n, q):
    """The position of quantile q among n sorted values: the float64 product (n - 1) q, one rounding."""
    return np.float64(n - 1) * np.float64(q)


def trimmed_mean(v, q_lo=0.01, q_hi=0.99):
    """{'mean', 'lo', 'hi', 'kept', 'nonfinite'} of the values ``v``: lo = sorted[floor(i(q_lo))], hi = sorted[ceil(i(q_hi))], kept
    = #{lo <= v <= hi}, mean = the float64 mean of those, summed in ascending order."""
    v = np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.float32)
    bad = int((~np.isfinite(v)).sum())
    if bad:
        return {'mean': float('nan'), 'lo': float('nan'), 'hi': float('nan'), 'kept': 0, 'nonfinite': bad}
    s = np.sort(v)
    n = len(s)
    lo = s[min(max(int(np.floor(virtual_index(n, q_lo))), 0), n - 1)]
    hi = s[min(max(int(np.ceil(virtual_index(n, q_hi))), 0), n - 1)]
    keep = s[(s >= lo) & (s <= hi)].astype(np.float64)
    return {'mean': float(np.sum(keep) / len(keep)), 'lo': float(lo), 'hi': float(hi), 'kept': len(keep), 'nonfinite': 0}


# ---- path_length --------------------------------------------------------------------------------------------------------------
def pyramid_mse(x, y, weights):
    """sum_l weights[l] mean(d_l^2), d_0 = x - y, d_{l+1} the 2x2 mean of d_l; (N,) in the dtype of x."""
    d, total = x - y, 0
    for l, w in enumerate(weights):
        if l:
            d = torch.nn.functional.avg_pool2d(d, 2)
        total = total + w * (d * d).mean(dim=(1, 2, 3))
    return total


def path_length(synth, a, b, mode, sampling='full', epsilon=1e-4, weights=None, embed=None, trim=(1, 99), seed=0,
                dtype=torch.float64):
    """``ppl.path_length`` in ``dtype`` on the CPU, all pairs at once: ``synth`` / ``embed`` must accept ``dtype`` tensors."""
    n = a.shape[0]
    t = uniforms(substream(seed, 1), 0, n) if sampling == 'full' else np.zeros(n)
    ends = endpoints(a, b, t, epsilon, mode, dtype)
    x0, x1 = synth(ends[0]), synth(ends[1])
    if embed is None:
        if weights is None:
            weights = (1.0,) * min(6, int(x0.shape[2]).bit_length())
        dist = pyramid_mse(x0, x1, weights)
    else:
        dist = row_sqdist(embed(x0).flatten(1), embed(x1).flatten(1), dtype)
    dist32 = dist.to(torch.float32)
    out = trimmed_mean(dist32, trim[0] / 100, trim[1] / 100)
    return {'ppl': out['mean'] / (epsilon * epsilon), 'lo': out['lo'], 'hi': out['hi'], 'kept': out['kept'], 'distances': dist}
