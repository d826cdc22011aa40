"""Float64 restatement of ADA's filter, noise and cutout groups (csrc/ada_filter.hip) on the CPU: the ext row of
a sample from its 16 Philox words, the filter as a gather by the reflection map followed by two grouped ``conv2d`` (so it is
defined at every size, also where torch's own reflect pad refuses a halo of 21), and the whole of
``cutout(noise(filter(x)))``.  Everything is a pure function of torch tensors, differentiable in ``x``: the adjoint the
tests compare against is autograd's.  With ``dtype=torch.float32`` the same code is ATen's fp32 composition, whose error
the tests measure in the same unit as the kernel's."""
import math

import numpy as np
import torch
import torch.nn.functional as F

TAPS, HALF = 43, 21
FILTER, NOISE, CUTOUT = 8, 16, 32


def reflect_map(n):
    """r(i) for i = -21 .. n + 20: m = i mod 2(n - 1), r = m if m < n else 2(n - 1) - m."""
    i = torch.arange(-HALF, n + HALF)
    per = 2 * (n - 1)
    m = i % per
    return torch.where(m < n, m, per - m)


def taps(g, bank):
    """h = fp32(sum_b g_b F[b]), summed in float64: (N, 4) gains, (4, 43) bank -> (N, 43) float64 holding fp32 values."""
    return (g.double() @ bank.double()).float().double()


def fir(x, h):
    """The separable filter of an (N, 3, H, W) batch with per-sample taps (N, 43), in x's dtype: rows first, then columns."""
    n, c, hh, ww = x.shape
    xp = x[:, :, reflect_map(hh)][:, :, :, reflect_map(ww)].reshape(1, n * c, hh + 2 * HALF, ww + 2 * HALF)
    w = h.to(x.dtype).repeat_interleave(c, dim=0)
    y = F.conv2d(xp, w.view(n * c, 1, 1, TAPS), groups=n * c)
    y = F.conv2d(y, w.view(n * c, 1, TAPS, 1), groups=n * c)
    return y.reshape(n, c, hh, ww)


def keep_mask(ext, h, w):
    """(N, 1, H, W) float64: 0 inside the cutout rectangle of a row whose gate bit 5 is set, 1 elsewhere."""
    j, i = torch.arange(w).view(1, 1, 1, w), torch.arange(h).view(1, 1, h, 1)
    e = ext.double()
    col = lambda k: e[:, k].view(-1, 1, 1, 1)  # noqa: E731
    on = ((ext[:, 9].long() & CUTOUT) != 0).view(-1, 1, 1, 1)
    inside = on & (j >= col(5)) & (j < col(6)) & (i >= col(7)) & (i < col(8))
    return (~inside).double()


def sigma(ext):
    """(N,) float64: the noise scale of a row, which counts only with gate bit 4."""
    return torch.where((ext[:, 9].long() & NOISE) != 0, ext[:, 4].double(), torch.zeros(()).double())


def apply(x, ext, noise, bank, dtype=torch.float64):
    """cutout(noise(filter(x))) under the (N, 16) ext rows; the gate mask decides what acts: samples whose band gates are all
    closed are not filtered, sigma counts with bit 4 and the rectangle with bit 5."""
    x = x.to(dtype)
    filt = (ext[:, 9].long() & 15) != 0
    y = x
    if filt.any():
        y = torch.where(filt.view(-1, 1, 1, 1), fir(x, taps(ext[:, :4], bank)), x)
    if noise is not None:
        y = y + sigma(ext).to(dtype).view(-1, 1, 1, 1) * noise.to(dtype)
    return y * keep_mask(ext, x.shape[2], x.shape[3]).to(dtype)


def unit(x, ext, bank):
    """2^-24 (|h| * |h| * |x|) at every pixel, in float64 (|x| itself where the sample is not filtered)."""
    filt = ((ext[:, 9].long() & 15) != 0).view(-1, 1, 1, 1)
    a = x.double().abs()
    return 2.0 ** -24 * torch.where(filt, fir(a, taps(ext[:, :4], bank).abs()), a)


def adjoint(g, ext, bank, dtype=torch.float64):
    """F^T (mask o g) by autograd through ``apply``."""
    x = torch.zeros_like(g, dtype=dtype).requires_grad_(True)
    y = apply(x, ext, None, bank, dtype)
    return torch.autograd.grad(y, x, g.to(dtype))[0]


def adjoint_unit(g, ext, bank):
    """The forward's unit transposed: 2^-24 (|F|^T |mask o g|)."""
    x = torch.zeros_like(g, dtype=torch.float64).requires_grad_(True)
    filt = ((ext[:, 9].long() & 15) != 0).view(-1, 1, 1, 1)
    y = torch.where(filt, fir(x, taps(ext[:, :4], bank).abs()), x) * keep_mask(ext, g.shape[2], g.shape[3])
    return 2.0 ** -24 * torch.autograd.grad(y, x, g.double().abs())[0]


def restated_row(words, h, w, p, mask):
    """The ext row of one sample from its 16 Philox words: u(k) = (word k >> 8) 2^-24, fp64 Box-Muller on
    ((word a >> 8) + 1) 2^-24 and u(a + 1).  Returns (bits, [j0, j1, i0, i1], raw z (4, fp32), cx, cy, g (4, float64),
    sigma (float64)): raw values rounded to fp32, g and sigma composed from them in float64."""
    f = np.float32
    u = [(wd >> 8) * 2.0 ** -24 for wd in words]
    p = float(f(p))

    def normal(k):
        r, a = math.sqrt(-2.0 * math.log(((words[k] >> 8) + 1) * 2.0 ** -24)), 2.0 * math.pi * u[k + 1]
        return r * math.cos(a), r * math.sin(a)

    def clamp3(z):
        return min(max(z, -3.0), 3.0)
    band = [bool(mask & FILTER) and u[b] < p for b in range(4)]
    g_noise, g_cut = bool(mask & NOISE) and u[4] < p, bool(mask & CUTOUT) and u[5] < p
    cx, cy = f(u[6]), f(u[7])
    z = [f(clamp3(v)) for v in normal(8) + normal(10)]
    zn = f(clamp3(normal(12)[0]))
    e = np.array([10.0, 1.0, 1.0, 1.0]) / 13.0
    g = np.ones(4)
    for i in range(4):
        t = np.ones(4)
        if band[i]:
            t[i] = 2.0 ** float(z[i])
        g *= t / math.sqrt(float((e * t * t).sum()))
    sigma = 0.1 * abs(float(zn)) if g_noise else 0.0

    def bounds(n, c):
        inside = [k for k in range(n) if abs((k + 0.5) / n - float(c)) < 0.25]
        return [inside[0], inside[-1] + 1] if inside else [0, 0]
    rect = bounds(w, cx) + bounds(h, cy) if g_cut else [0, 0, 0, 0]
    bits = sum(int(b) << k for k, b in enumerate(band)) | int(g_noise) << 4 | int(g_cut) << 5
    return bits, rect, z, cx, cy, g, sigma
