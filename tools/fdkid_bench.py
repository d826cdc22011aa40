#!/usr/bin/env python3
"""Time the Frechet moment accumulation and the three KID passes (gan_lab_amd/frechet.py, gan_lab_amd/kid.py; csrc/frechet.hip,
csrc/kid.hip) against their ATen compositions, each with its error against float64, and the host-side solve of the distance.

    timeout -k 10 600 python tools/fdkid_bench.py [--n 10000] [--dim 3072] [--batch 64] [--reps 3] [--out FILE]

Rows: reals ``0.5 + 0.25 randn``, fakes ``0.45 + 0.3 randn`` (images are not centred).  Moments: the rows of the real set fed in
batches of ``--batch`` into zeroed accumulators (kernel), against ATen ``X.T @ X`` of the whole set in fp32 and in fp64; error:
the covariance against float64 two-pass.  KID: the three row-sum passes (kernel), against ATen ``mm`` + ``pow`` + ``sum`` in fp32;
error: the worst relative row-sum error of ``--err-rows`` rows against float64.  Host: ``frechet.distance`` at D = 768 and D =
``--dim`` (wall clock, one run each)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--dim', type=int, default=3072)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--err-rows', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gan_lab_amd import frechet, ops
    n, d = args.n, args.dim
    gen = torch.Generator(device='cuda').manual_seed(0)
    real = 0.5 + 0.25 * torch.randn(n, d, device='cuda', generator=gen)
    fake = 0.45 + 0.3 * torch.randn(n, d, device='cuda', generator=gen)
    out = {'n': n, 'dim': d, 'batch': args.batch, 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}

    # ---- moments -----------------------------------------------------------------------------------------------------------
    pivot = real[:args.batch].mean(dim=0)
    s, g = torch.zeros(d, dtype=torch.float64, device='cuda'), torch.zeros(d, d, dtype=torch.float64, device='cuda')

    def kernel_moments():
        s.zero_()
        g.zero_()
        for lo in range(0, n, args.batch):
            ops.moments_accum(real[lo:lo + args.batch], pivot, s, g)

    real64 = real.double()
    mom = {'kernel_ms': timed(kernel_moments, args.reps), 'aten_fp32_ms': timed(lambda: real.T @ real, args.reps),
           'aten_fp64_ms': timed(lambda: real64.T @ real64, args.reps)}
    mean64 = real64.mean(dim=0)
    y = real64 - mean64
    cov64 = (y.T @ y) / (n - 1)
    kernel_moments()
    cov = (g - torch.outer(s, s) / n) / (n - 1)
    mu32 = real.mean(dim=0)
    cov32 = (((real.T @ real) / n - torch.outer(mu32, mu32)) * (n / (n - 1))).double()
    mom['cov_err'] = {'kernel': float((cov - cov64).abs().max()), 'aten_fp32': float((cov32 - cov64).abs().max()),
                      'scale': float(cov64.abs().max())}
    mom = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in mom.items()}
    out['moments'] = mom
    print(f'moments, {n} x {d} in batches of {args.batch}: kernel {mom["kernel_ms"]} ms, ATen X.T @ X fp32 {mom["aten_fp32_ms"]} ms, '
          f'fp64 {mom["aten_fp64_ms"]} ms; covariance error (scale {mom["cov_err"]["scale"]:.3g}): kernel '
          f'{mom["cov_err"]["kernel"]:.2e}, ATen fp32 E[xx^T] - mu mu^T {mom["cov_err"]["aten_fp32"]:.2e}')
    del real64, y, cov64, cov32, cov

    # ---- KID ---------------------------------------------------------------------------------------------------------------
    gamma = 1.0 / d
    sums = [torch.empty(n, dtype=torch.float64, device='cuda') for _ in range(3)]

    def kernel_kid():
        ops.kid_rowsums(real, real, gamma, exclude_diag=True, out=sums[0])
        ops.kid_rowsums(fake, fake, gamma, exclude_diag=True, out=sums[1])
        ops.kid_rowsums(real, fake, gamma, out=sums[2])

    def aten_pass(a, b, diag):
        k = (gamma * (a @ b.T) + 1.0).pow(3)
        if diag:
            k.fill_diagonal_(0.0)
        return k.sum(dim=1)

    def aten_kid():
        return aten_pass(real, real, True), aten_pass(fake, fake, True), aten_pass(real, fake, False)

    kd = {'kernel_ms': round(timed(kernel_kid, args.reps), 3), 'aten_fp32_ms': round(timed(aten_kid, args.reps), 3)}
    kd['kernel_tflops'] = round(3 * 2.0 * d * n * n / kd['kernel_ms'] / 1e9, 2)
    e = min(args.err_rows, n)
    want = (gamma * (real[:e].double() @ fake.double().T) + 1.0).pow(3).sum(dim=1)
    kernel_kid()
    kd['rowsum_rel_err'] = {'kernel': float(((sums[2][:e] - want).abs() / want.abs()).max()),
                            'aten_fp32': float(((aten_pass(real, fake, False)[:e].double() - want).abs() / want.abs()).max())}
    out['kid'] = kd
    print(f'KID, three passes over {n} x {n} x {d}: kernel {kd["kernel_ms"]} ms ({kd["kernel_tflops"]} TFLOP/s), ATen mm + pow + sum '
          f'fp32 {kd["aten_fp32_ms"]} ms; worst relative row-sum error: kernel {kd["rowsum_rel_err"]["kernel"]:.2e}, ATen fp32 '
          f'{kd["rowsum_rel_err"]["aten_fp32"]:.2e}')

    # ---- the host solve ------------------------------------------------------------------------------------------------------
    out['host_solve_s'] = {}
    for dim in sorted({768, d}):
        ev = frechet.Frechet(dim)
        ev.feed_real(real[:2 * dim, :dim].contiguous())
        ev.feed_fake(fake[:2 * dim, :dim].contiguous())
        moments = [t.cpu() for t in ev.moments('real') + ev.moments('fake')]
        t0 = time.perf_counter()
        frechet.distance(*moments)
        out['host_solve_s'][str(dim)] = round(time.perf_counter() - t0, 3)
        print(f'host solve of the distance at D = {dim}: {out["host_solve_s"][str(dim)]} s')
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
