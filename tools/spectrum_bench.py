#!/usr/bin/env python3
"""Time the per-image radial power-spectrum profiles (gan_lab_amd/spectrum.py) next to the same profiles composed from
``torch.fft.rfft2`` and torch binning on the same GPU, and print a small demonstration of the two distances.

    timeout -k 10 600 python tools/spectrum_bench.py [--res 256 1024] [--images 64] [--reps 7] [--out profiles/spectrum_bench.txt]

One process.  Per resolution both paths are warmed once and then timed alternating, median over ``--reps``; times are device
times (events).  The torch side is rfft2 of the windowed batch, |F|^2 summed over channels in fp64, and one ``index_add_`` into
the bins with the half-spectrum weights; it walks the images in chunks of ``--torch-chunk`` so that its temporaries fit.  'bytes
moved' is what the fused path reads and writes per image (the image once, the half spectrum written by the row pass and read by
the column pass, the per-tile bin sums) against one read of the image.

The demonstration scores a set of 1/f images against a second draw of the same process and against the same set after a nearest
2x down- and up-sampling, the artifact the 'hf' band is there to catch."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median_pair(f_hip, f_torch, reps):
    """Interleaved A/B: warm both once, then ``reps`` alternating runs; medians."""
    f_hip(), f_torch()
    th, tt = [], []
    for _ in range(reps):
        th.append(timed(f_hip)[0])
        tt.append(timed(f_torch)[0])
    return statistics.median(th), statistics.median(tt)


def torch_tables(res, dev):
    """(window (R,), bin of every rfft2 coefficient (R, R/2 + 1) with the dropped corners sent to a spill bin, weights / count)."""
    w = (0.5 - 0.5 * torch.cos(2. * torch.pi * torch.arange(res, dtype=torch.float64) / res)).float().to(dev)
    ku = torch.arange(res, dtype=torch.int64)
    ku = torch.where(ku < res // 2, ku, ku - res)
    kv = torch.arange(res // 2 + 1, dtype=torch.int64)
    s4 = 4 * (ku[:, None] ** 2 + kv[None, :] ** 2)
    thresholds = (2 * torch.arange(1, 2 * res, dtype=torch.int64) - 1) ** 2
    idx = torch.searchsorted(thresholds, s4, right=True).clamp_(max=res // 2 + 1)
    wt = torch.full((res // 2 + 1,), 2., dtype=torch.float64)
    wt[0] = wt[-1] = 1.
    wt = wt[None, :].expand(res, -1)
    cnt = torch.zeros(res // 2 + 2, dtype=torch.float64).index_add_(0, idx.reshape(-1), wt.reshape(-1))
    return w, idx.reshape(-1).to(dev), (wt / cnt[idx]).reshape(-1).to(dev)


def torch_profiles(x, tables):
    w, idx, wt = tables
    res = x.shape[-1]
    f = torch.fft.rfft2((x * w[None, None, None, :]) * w[None, None, :, None])
    p = (f.real * f.real + f.imag * f.imag).double().sum(dim=1).reshape(len(x), -1) * wt
    out = torch.zeros((len(x), res // 2 + 2), dtype=torch.float64, device=x.device).index_add_(1, idx, p)
    return out[:, :res // 2 + 1] / (3. * res * res * (9. / 64.))


def one_over_f(n, res, seed, dev):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    k = torch.fft.fftfreq(res) * res
    r = torch.sqrt(k[:, None] ** 2 + k[None, :] ** 2).clamp_(min=1.)
    x = torch.fft.ifft2(torch.fft.fft2(torch.randn(n, 3, res, res, generator=gen, dtype=torch.float64)) / r).real
    return (x / x.abs().max()).float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--torch-chunk', type=int, default=16)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from gan_lab_amd import ops, spectrum
    dev = torch.device('cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# spectrum_bench: {a.images} images, window hann, {a.reps} alternating repetitions, medians')
    say(f'{"res":<6}{"HIP us/img":>12}{"torch us/img":>14}{"torch/HIP":>11}{"moved MB/img":>14}{"x one read":>12}{"HIP GB/s":>10}'
        f'{"max rel diff":>14}')
    gen = torch.Generator(device='cuda').manual_seed(0)
    for res in a.res:
        spectrum.check_res(res)
        n = a.images
        x = torch.empty((n, 3, res, res), device=dev).normal_(generator=gen)
        chunk = spectrum._chunk(res, n)
        ws, scratch = ops.spectrum_workspace(n, res, dev), ops.spectrum_scratch(chunk, res, dev)
        tables = torch_tables(res, dev)

        def hip():
            spectrum._run(x, res, 'hann', ws, 0, n, scratch, chunk)

        def composed():
            return torch.cat([torch_profiles(x[i:i + a.torch_chunk], tables) for i in range(0, n, a.torch_chunk)])
        h, t = median_pair(hip, composed, a.reps)
        diff = float(((ws - composed()).abs() / ws).max())
        per_image = ops.spectrum_scratch_bytes(2, res) - ops.spectrum_scratch_bytes(1, res)
        half = 3 * res * (res // 2 + 1) * 8
        moved = 3 * res * res * 4 + 2 * half + 2 * (per_image - half) + (res // 2 + 1) * 8
        say(f'{res:<6}{1e3 * h / n:>12.2f}{1e3 * t / n:>14.2f}{t / h:>11.2f}{moved / 1e6:>14.3f}{moved / (3 * res * res * 4):>12.2f}'
            f'{moved * n / 1e6 / h:>10.0f}{diff:>14.2e}')

    say('# demonstration: 8 images at 64x64, 1/f amplitude; spectrum / spectrum hf in dB')
    a_set, b_set = one_over_f(8, 64, 1, dev), one_over_f(8, 64, 2, dev)
    resampled = a_set[:, :, ::2, ::2].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).contiguous()

    def score(fake, real):
        f, r = spectrum.PowerSpectrum(64, 8), spectrum.PowerSpectrum(64, 8)
        f.feed(fake)
        r.feed(real)
        return spectrum.distance(f, r)
    for name, fake in (('a second draw of the same process', b_set), ('the set after nearest 2x down-up sampling', resampled)):
        d = score(fake, a_set)
        say(f'{name:<44}{d["spectrum"]:>8.2f}{d["hf"]:>8.2f}')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
