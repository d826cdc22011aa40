#!/usr/bin/env python3
"""Time the five passes of k-NN precision / recall / density / coverage (gan_lab_amd/prdc.py; csrc/prdc.hip) against the ATen
composition, and report the radii's error against float64.

    timeout -k 10 600 python tools/prdc_bench.py [--n 10000] [--m 10000] [--dim 3072] [--k 5] [--reps 5] [--out FILE]

Rows are the 4-dimensional-manifold sets of tests/prdc_reference.py (reals t ~ N(0, I), fakes t ~ N(0.8, 0.7^2 I)).  Kernel path:
the two k-NN passes and the three cross passes, each timed with events (median over ``--reps``), norms included.  ATen
composition: per pass ``|q|^2 + |k|^2 - 2 q k^T`` through ``mm`` into an (N, M) matrix, then ``topk`` (k-NN, the diagonal set to
inf) or a comparison and ``min`` (cross).  Error: the kernel's and ATen's k-th radii of ``--err-rows`` real rows against a float64
evaluation on the GPU, in units of 2^-24 (|q|^2 + |k|^2)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


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


def aten_sq(a, b):
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).clamp_min_(0)


def aten_knn(x, k):
    d = aten_sq(x, x)
    d.fill_diagonal_(float('inf'))
    return d.topk(k, dim=1, largest=False).values


def aten_cross(q, keys, rad, radius_of):
    d = aten_sq(q, keys)
    inside = d <= (rad[None, :] if radius_of == 'key' else rad[:, None])
    dmin, imin = d.min(dim=1)
    return inside.sum(1), dmin, imin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--m', type=int, default=10000)
    ap.add_argument('--dim', type=int, default=3072)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--err-rows', type=int, default=512)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import prdc_reference as ref
    from gan_lab_amd import ops
    real, fake = (torch.from_numpy(a).cuda() for a in ref.manifold_rows(args.n, args.m, args.dim, seed=0))
    k = args.k
    passes = {}
    rad_r = ops.prdc_knn(real, k)[:, k - 1].contiguous()
    rad_f = ops.prdc_knn(fake, k)[:, k - 1].contiguous()
    passes['knn real'] = (lambda: ops.prdc_knn(real, k), lambda: aten_knn(real, k))
    passes['knn fake'] = (lambda: ops.prdc_knn(fake, k), lambda: aten_knn(fake, k))
    passes['fake in real (precision, density, nearest real)'] = (lambda: ops.prdc_cross(fake, real, rad_r, 'key'),
                                                                 lambda: aten_cross(fake, real, rad_r, 'key'))
    passes['real in fake (recall)'] = (lambda: ops.prdc_cross(real, fake, rad_f, 'key'),
                                       lambda: aten_cross(real, fake, rad_f, 'key'))
    passes['real covered (coverage)'] = (lambda: ops.prdc_cross(real, fake, rad_r, 'query'),
                                         lambda: aten_cross(real, fake, rad_r, 'query'))
    out = {'n': args.n, 'm': args.m, 'dim': args.dim, 'k': k, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'passes': {}}
    for name, (kernel, aten) in passes.items():
        row = {'kernel_ms': round(timed(kernel, args.reps), 3), 'aten_ms': round(timed(aten, args.reps), 3)}
        out['passes'][name] = row
        print(f'{name}: kernel {row["kernel_ms"]} ms, ATen {row["aten_ms"]} ms')
    out['kernel_ms'] = round(sum(r['kernel_ms'] for r in out['passes'].values()), 3)
    out['aten_ms'] = round(sum(r['aten_ms'] for r in out['passes'].values()), 3)
    flops = 2.0 * args.dim * (args.n * args.n + args.m * args.m + 3.0 * args.n * args.m)
    out['kernel_tflops'] = round(flops / out['kernel_ms'] / 1e9, 2)
    # the radii of the first rows against float64 (an (err_rows, N) float64 matrix on the device)
    e = min(args.err_rows, args.n)
    d64 = torch.cdist(real[:e].double(), real.double()).pow(2)
    d64[torch.arange(e), torch.arange(e)] = float('inf')
    want, idx = d64.topk(k, dim=1, largest=False)
    n2 = (real.double() ** 2).sum(1)
    unit = 2.0 ** -24 * (n2[:e] + n2[idx[:, k - 1]])
    out['radius_err_units'] = {'kernel': round(float(((rad_r[:e].double() - want[:, k - 1]).abs() / unit).max()), 2),
                               'aten': round(float(((aten_knn(real, k)[:e, k - 1].double() - want[:, k - 1]).abs() / unit).max()), 2)}
    print(f'all five passes: kernel {out["kernel_ms"]} ms ({out["kernel_tflops"]} TFLOP/s), ATen {out["aten_ms"]} ms; radius error '
          f'kernel {out["radius_err_units"]["kernel"]} / ATen {out["radius_err_units"]["aten"]} units of 2^-24 (|q|^2 + |k|^2)')
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
