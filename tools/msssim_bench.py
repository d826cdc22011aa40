#!/usr/bin/env python3
"""Time one MS-SSIM evaluation (gan_lab_amd/msssim.py) level by level, next to the same stage composed from torch ops on the
same GPU (grouped ``F.conv2d`` for the separable window, ``F.avg_pool2d`` for the next level, fp64 means).

    timeout -k 10 600 python tools/msssim_bench.py --res 128 --pairs 4096 [--reps 7] [--out profiles/msssim_bench.txt]
    timeout -k 10 600 python tools/msssim_bench.py --res 1024 --pairs 512

One process.  The five levels are first run once through the HIP path (warm-up, and it leaves every level's input on the device);
each level is then timed on that data, HIP and torch alternating, median over ``--reps``.  The torch side walks the pairs in
chunks (``--torch-chunk-mb`` of one image batch per chunk) so that its ~15 full-size temporaries fit; the HIP side runs all pairs
in one launch.  Times are device times (events), in ms.  'min GB' is what the level must move at least: both images read once
(2 P 3 S^2 4 bytes) and, except at the last level, a quarter of that written for the next level.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def window(side, dev):
    s = min(11, side)
    k = torch.arange(s, dtype=torch.float64)
    g = torch.exp(-(k - (s - 1) / 2.) ** 2 / (2. * (1.5 * s / 11) ** 2))
    return (g / g.sum()).float().to(dev)


def torch_level(a, b, g, c1, c2, last):
    """One level composed from torch ops: (sum of cs, sum of ssim) per pair in fp64, and the pooled images."""
    s = g.numel()
    kx, ky = g.view(1, 1, 1, s).expand(15, 1, 1, s).contiguous(), g.view(1, 1, s, 1).expand(15, 1, s, 1).contiguous()
    q = torch.cat([a, b, a * a, b * b, a * b], dim=1)
    q = F.conv2d(F.conv2d(q, kx, groups=15), ky, groups=15)
    mu_a, mu_b, aa, bb, ab = q.split(3, dim=1)
    s_aa, s_bb, s_ab = aa - mu_a * mu_a, bb - mu_b * mu_b, ab - mu_a * mu_b
    v1, v2 = 2. * s_ab + c2, s_aa + s_bb + c2
    cs = v1 / v2
    ssim = (2. * mu_a * mu_b + c1) * v1 / ((mu_a * mu_a + mu_b * mu_b + c1) * v2)
    out = cs.double().sum(dim=(1, 2, 3)), ssim.double().sum(dim=(1, 2, 3))
    return out if last else out + (F.avg_pool2d(a, 2), F.avg_pool2d(b, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--pairs', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--torch-chunk-mb', type=int, default=256)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from gan_lab_amd import msssim, ops
    dev = torch.device('cuda')
    res, n = msssim.check_res(a.res), a.pairs
    c1, c2 = msssim.constants(2.0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.empty((2 * n, 3, res, res), device=dev)
    for i in range(0, 2 * n, 64):                              # drawn in slices: no second full-size temporary
        x[i:i + 64].normal_(generator=gen)
    x[1::2].mul_(0.25).add_(x[0::2])                           # pairs that are alike but not equal
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# msssim_bench: {res}x{res}, {n} pairs, data range 2.0, {a.reps} alternating repetitions, medians')
    ws = ops.msssim_workspace(n, res, dev)
    pooled = msssim._pooled_buffers(n, res, dev)
    levels = [(x[0::2], x[1::2])] + [(p[0::2], p[1::2]) for p in pooled]
    msssim._run_levels(levels[0][0], levels[0][1], res, c1, c2, ws, 0, n, pooled)       # warm-up; fills every level
    torch.cuda.synchronize()
    say(f'{"level":<7}{"side":>6}{"HIP ms":>11}{"torch ms":>11}{"torch/HIP":>11}{"min GB":>9}{"HIP GB/s":>10}')
    tot_h = tot_t = tot_b = 0.
    for lv in range(msssim.LEVELS):
        side, last = res >> lv, lv == msssim.LEVELS - 1
        la, lb = levels[lv]
        na, nb = (None, None) if last else levels[lv + 1]
        g = window(side, dev)
        chunk = max(1, min(n, (a.torch_chunk_mb << 20) // (3 * side * side * 4)))

        def hip():
            ops.msssim_level(la, lb, lv, res, c1, c2, ws, 0, n, na, nb)

        def composed():
            for i in range(0, n, chunk):
                torch_level(la[i:i + chunk], lb[i:i + chunk], g, c1, c2, last)
        h, t = median_pair(hip, composed, a.reps)
        nbytes = 2 * n * 3 * side * side * 4 * (1. if last else 1.25)
        say(f'{lv:<7}{side:>6}{h:>11.3f}{t:>11.3f}{t / h:>11.2f}{nbytes / 1e9:>9.3f}{nbytes / 1e6 / h:>10.0f}')
        tot_h, tot_t, tot_b = tot_h + h, tot_t + t, tot_b + nbytes
    say(f'{"total":<7}{"":>6}{tot_h:>11.3f}{tot_t:>11.3f}{tot_t / tot_h:>11.2f}{tot_b / 1e9:>9.3f}{tot_b / 1e6 / tot_h:>10.0f}')
    table = torch.empty((n, msssim.LEVELS, 2), dtype=torch.float64, device=dev)
    values, out = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(6, dtype=torch.float64, device=dev)
    ops.msssim_finish(ws, n, res, table, values, out)
    t_fin = statistics.median(timed(lambda: ops.msssim_finish(ws, n, res, table, values, out))[0] for _ in range(a.reps))
    say(f'finish (per-pair table, products, means): {t_fin:.3f} ms')
    # a complete evaluation as a learner runs it: feeds of 64 images, then result()
    ms = msssim.MultiScaleSSIM(res, 2 * n)

    def evaluate():
        ms.reset()
        for i in range(0, 2 * n, 64):
            ms.feed(x[i:i + 64])
        return ms.result()
    evaluate()
    t_all, result = timed(evaluate)
    say(f'measured end to end (HIP): {2 * n // 64 + (2 * n % 64 > 0)} feeds of 64 images + result() {t_all:.2f} ms; msssim '
        f'{result["msssim"]:.6f} (one-launch path {float(out[0]):.6f})')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
