#!/usr/bin/env python3
"""Measure consistency regularisation of the ResNet GAN (gan_lab_amd/consistency.py; csrc/cr.hip): what each term costs a critic
and a generator step, and the three kernels against their ATen compositions.

    timeout -k 10 300 python tools/cr_bench.py [--batch 64] [--iters 10] [--reps 20] [--out profiles/cr_bench.json]

1. The kernels at the config-5 geometry (batch x 3 x 64 x 64 images, batch scores): ``ops.cr_transform`` against a per-image
   ``torch.roll`` + ``flip`` + border fill, ``ops.cr_msd`` / ``ops.cr_imsd`` forward + backward against ``((a - b) ** 2).mean()``
   under autograd; device time (events), median over ``--reps``, and launches of this library per call.
2. ``d_step`` and ``g_step`` of the ResNet GAN at 64x64 (the default wgan + wgan-gp) with every term off, each term on alone,
   and all four on: wall time with a device synchronisation, one warm-up, the median of ``--iters``, and this library's launches
   per step.  The row with the terms off is the code path of the commit before the feature."""
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(run, reps):
    run()
    torch.cuda.synchronize()
    return round(statistics.median(timed(run) for _ in range(reps)), 4)


def wall_ms(run, iters):
    run()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        run()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3)


def aten_transform(x, table):
    out = torch.zeros_like(x)
    h, w = x.shape[2:]
    for n, (flip, dx, dy, _) in enumerate(table):
        src = x[n].flip(-1) if flip else x[n]
        out[n, :, max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = \
            src[:, max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def bench_kernels(args, ops, _lib):
    n = args.batch
    x = torch.randn(2 * n, 3, 64, 64, device='cuda')
    table = ops.cr_params(2 * n, 8, True, 1, 0, 'cuda')
    host_table = table.cpu().tolist()
    a, b = torch.randn(n, device='cuda', requires_grad=True), torch.randn(n, device='cuda', requires_grad=True)
    both = x.clone().requires_grad_(True)

    def fwd_bwd(fn, leaves):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward()
        return run

    rows = {}
    for name, ours, aten in (
            ('cr_transform', lambda: ops.cr_transform(x, table), lambda: aten_transform(x, host_table)),
            ('cr_msd fwd+bwd', fwd_bwd(lambda: ops.cr_msd(a, b), (a, b)), fwd_bwd(lambda: ((a - b) ** 2).mean(), (a, b))),
            ('cr_imsd fwd+bwd', fwd_bwd(lambda: ops.cr_imsd(both), (both,)),
             fwd_bwd(lambda: ((both[:n] - both[n:]) ** 2).mean(), (both,)))):
        n0 = _lib.launch_count()
        ours()
        rows[name] = {'library_launches': _lib.launch_count() - n0, 'kernel_ms': median_ms(ours, args.reps),
                      'aten_ms': median_ms(aten, args.reps)}
        print(f'{name}: {rows[name]}')
    return rows


def learner(args, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=64, res_dataset=64, batch_size=args.batch,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=0, **kw)
    L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    return L


def bench_steps(args, _lib):
    real = torch.rand(args.batch, 3, 64, 64, device='cuda') * 2 - 1
    rows = {}
    for name, kw in (('off', {}), ('cr_real=10', dict(cr_real=10.)), ('cr_fake=10', dict(cr_fake=10.)),
                     ('cr_latent_d=5', dict(cr_latent_d=5.)), ('cr_latent_g=0.5', dict(cr_latent_g=0.5)),
                     ('all (10, 10, 5, 0.5)', dict(cr_real=10., cr_fake=10., cr_latent_d=5., cr_latent_g=0.5))):
        L = learner(args, **kw)

        def d_step():
            L.d_step(real)
            torch.cuda.synchronize()

        def g_step():
            L.g_step()
            torch.cuda.synchronize()

        rows[name] = {}
        for what, step, frozen in (('d_step', d_step, True), ('g_step', g_step, False)):
            L.set_requires_grad_disc(frozen)
            step()
            n0 = _lib.launch_count()
            step()
            rows[name][what] = {'library_launches': _lib.launch_count() - n0, 'ms': wall_ms(step, args.iters)}
        print(f'ResNet GAN 64x64, batch {args.batch}, {name}: {rows[name]}')
        del L
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gan_lab_amd import _lib, ops
    out = {'batch': args.batch, 'iters': args.iters, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'kernels': bench_kernels(args, ops, _lib), 'steps': bench_steps(args, _lib)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
