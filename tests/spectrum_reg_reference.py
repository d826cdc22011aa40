"""Torch restatement of the power-spectrum regulariser as DESIGN.md 4.9b defines it.  A test helper: no GPU, nothing of the package
imported.  Everything runs in the ``dtype`` asked for: float64 is the definition (full ``torch.fft.fft2``, no Hermitian shortcut);
float32 runs the same steps - window product, transform, bin sums, logarithms, the inverse transform of the backward - in fp32 on the
CPU and is the yardstick of the GPU tests: what fp32 arithmetic alone costs, whatever the factorisation of the transform.

    window   'hann': w[i] = 0.5 - 0.5 cos(2 pi i / R) (periodic); 'none': w = 1; W = (sum_i w[i]^2 / R)^2
    power    y = x w[i] w[j], F_c = DFT2(y_c), P[u, v] = 1/3 sum_c |F_c[u, v]|^2 / (R^2 W)
    bins     signed frequencies ku, kv in [-R/2, R/2); bin k iff (2k-1)^2 <= 4 (ku^2 + kv^2) < (2k+1)^2; bins 0 .. R/2 are kept
    A_n[k]   the mean of P_n over bin k (members_k coefficients);  S[k] = mean_n A_n[k]
    band     'all': k = 1 .. R/2;  'hf': k = R/4+1 .. R/2
    L        mean_{k in B} (ln max(S[k], 1e-30) - ln max(T[k], 1e-30))^2
backward, with gL the cotangent of L:
    gS[k]    gL 2 (ln S[k] - ln T[k]) / (|B| S[k]) for k in B with S[k] > 1e-30, else 0
    G[u, v]  gS[bin(u, v)] / (N members_bin 3 R^2 W), 0 outside every bin
    dy_c     2 R^2 Re(IDFT2(G o F_c));  dx_c[i, j] = dy_c[i, j] w[i] w[j];  T receives nothing
"""
import math

import torch

FLOOR = 1e-30
WINDOWS = ('hann', 'none')
BANDS = ('all', 'hf')


def window(res, kind, dtype=torch.float64):
    """(w in ``dtype``, rounded once from float64; W as a Python float)."""
    if kind == 'hann':
        w = 0.5 - 0.5 * torch.cos(2. * math.pi * torch.arange(res, dtype=torch.float64) / res)
    elif kind == 'none':
        w = torch.ones(res, dtype=torch.float64)
    else:
        raise ValueError(kind)
    return w.to(dtype), float((w * w).sum() / res) ** 2


def bin_index(res):
    """(R, R) int64 in fft order: the bin of every coefficient, by counting the thresholds (2j-1)^2, j >= 1, that 4 (ku^2 + kv^2)
    reaches; values above R/2 are the dropped corners."""
    k = torch.arange(res, dtype=torch.int64)
    k = torch.where(k < res // 2, k, k - res)
    s4 = 4 * (k[:, None] ** 2 + k[None, :] ** 2)
    j = torch.arange(1, 2 * res, dtype=torch.int64)
    return (s4[:, :, None] >= ((2 * j - 1) ** 2)[None, None, :]).sum(dim=2)


def band_bins(res, band):
    if band == 'all':
        return list(range(1, res // 2 + 1))
    if band == 'hf':
        return list(range(res // 4 + 1, res // 2 + 1))
    raise ValueError(band)


def _binning(res, dtype):
    """(M, members): the (R/2 + 1, R R) 0/1 matrix of bin membership in ``dtype`` and the member counts."""
    idx = bin_index(res).reshape(-1)
    nb = res // 2 + 1
    m = (idx[None, :] == torch.arange(nb)[:, None]).to(dtype)
    return m, m.sum(dim=1)


def spectra(x, kind='hann', dtype=torch.float64):
    """F (N, 3, R, R) complex of the windowed images, with w and W."""
    x = torch.as_tensor(x).to(dtype)
    res = x.shape[-1]
    w, W = window(res, kind, dtype)
    return torch.fft.fft2((x * w[None, None, None, :]) * w[None, None, :, None]), w, W


def profiles(x, kind='hann', dtype=torch.float64):
    """(N, R/2 + 1) per-image profiles A_n[k]."""
    f, _, W = spectra(x, kind, dtype)
    res = f.shape[-1]
    power = (f.real * f.real + f.imag * f.imag).sum(dim=1) / (3. * res * res * W)
    m, members = _binning(res, power.dtype)
    return power.reshape(len(power), -1) @ m.t() / members


def set_profile(x, kind='hann', dtype=torch.float64):
    return profiles(x, kind, dtype).mean(dim=0)


def loss_of_profile(s, target, band):
    res = 2 * (len(s) - 1)
    b = band_bins(res, band)
    d = torch.log(s[b].clamp_min(FLOOR)) - torch.log(target.to(s.dtype)[b].clamp_min(FLOOR))
    return (d * d).mean()


def loss(x, target, band='all', kind='hann', dtype=torch.float64):
    """L as a 0-dim tensor of ``dtype``; differentiable by torch.autograd when ``x`` requires grad."""
    return loss_of_profile(set_profile(x, kind, dtype), torch.as_tensor(target), band)


def loss_and_grad(x, target, band='all', kind='hann', grad_out=1.0, dtype=torch.float64):
    """(L, dx) by the hand-written backward of the module docstring, every step in ``dtype``."""
    x = torch.as_tensor(x).detach().to(dtype)
    target = torch.as_tensor(target).to(dtype)
    n, res = x.shape[0], x.shape[-1]
    f, w, W = spectra(x, kind, dtype)
    power = (f.real * f.real + f.imag * f.imag).sum(dim=1) / (3. * res * res * W)
    m, members = _binning(res, dtype)
    s = (power.reshape(n, -1) @ m.t() / members).mean(dim=0)
    b = band_bins(res, band)
    d = torch.log(s.clamp_min(FLOOR)) - torch.log(target.clamp_min(FLOOR))
    L = (d[b] * d[b]).mean()
    gs = torch.zeros_like(s)
    gs[b] = grad_out * 2. * d[b] / (len(b) * s[b])
    gs = torch.where(s > FLOOR, gs, torch.zeros_like(gs))
    per_bin = gs / (n * members * 3. * res * res * W)
    g = (per_bin[:, None] * m).sum(dim=0).reshape(res, res)           # 0 in the corners: they belong to no row of m
    dy = 2. * res * res * torch.fft.ifft2(g[None, None] * f).real
    return L, (dy * w[None, None, None, :]) * w[None, None, :, None]


class Loss(torch.autograd.Function):
    """L with the hand-written backward, for ``torch.autograd.gradcheck`` in float64."""

    @staticmethod
    def forward(ctx, x, target, band, kind):
        L, dx = loss_and_grad(x, target, band, kind, 1.0, x.dtype)
        ctx.save_for_backward(dx)
        return L

    @staticmethod
    def backward(ctx, gout):
        return gout * ctx.saved_tensors[0], None, None, None


def dft_matrix_profiles(x, kind='hann'):
    """Per-image profiles by brute force in float64: the DFT as a dense (R, R) matrix on both axes, bins by a Python loop."""
    x = torch.as_tensor(x).to(torch.float64)
    n, _, res, _ = x.shape
    w, W = window(res, kind)
    i = torch.arange(res, dtype=torch.float64)
    ang = -2. * math.pi * (i[:, None] * i[None, :]) / res
    d = torch.complex(torch.cos(ang), torch.sin(ang))
    y = (x * w[None, None, None, :] * w[None, None, :, None]).to(torch.complex128)
    f = d[None, None] @ y @ d.t()[None, None]
    power = (f.abs() ** 2).sum(dim=1) / (3. * res * res * W)
    out = torch.zeros(n, res // 2 + 1, dtype=torch.float64)
    cnt = torch.zeros(res // 2 + 1, dtype=torch.float64)
    for u in range(res):
        for v in range(res):
            ku, kv = (u if u < res // 2 else u - res), (v if v < res // 2 else v - res)
            r4 = 4 * (ku * ku + kv * kv)
            k = 0
            while (2 * k + 1) ** 2 <= r4:
                k += 1
            if k <= res // 2:
                out[:, k] += power[:, u, v]
                cnt[k] += 1
    return out / cnt


def smooth_noisy(n, res, seed, noise=0.1):
    """(n, 3, res, res) float32 test images: a few low-frequency waves per channel plus white noise of std ``noise``, so that every
    bin of the profile is far above the floor."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(res, dtype=torch.float64) / res
    x = torch.zeros(n, 3, res, res, dtype=torch.float64)
    for m in range(n):
        for c in range(3):
            a, b = 1 + (m + c) % 3, 1 + (2 * m + c) % 2
            x[m, c] = 0.5 * torch.sin(2. * math.pi * (a * i[:, None] + b * i[None, :]) + 0.3 * c) + 0.25 * torch.cos(
                2. * math.pi * b * i[:, None]) + 0.1 * (m - c)
    x = x + noise * torch.randn(n, 3, res, res, generator=g, dtype=torch.float64)
    return x.to(torch.float32)


def ema(profiles_seq, decay):
    """T after observing the set profiles in order: the first copies, then T <- decay T + (1 - decay) S.  float64."""
    t = None
    for s in profiles_seq:
        s = torch.as_tensor(s, dtype=torch.float64)
        t = s.clone() if t is None else decay * t + (1. - decay) * s
    return t
