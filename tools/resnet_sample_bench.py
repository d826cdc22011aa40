#!/usr/bin/env python3
"""Measure the sampling side of the ResNet GAN (gan_lab_amd/sampling.py; csrc/sample.hip): what the averaged generator costs a
generator step, and what ``learner.generate`` costs with and without truncation and standing statistics.

    timeout -k 10 300 python tools/resnet_sample_bench.py [--batch 64] [--iters 10] [--reps 20] [--out profiles/resnet_sample_bench.json]

1. The draw: ``ops.trunc_randn`` against ``ops.randn`` at 2^20 and at batch x len_latent elements, and ``ops.ewma_many`` over
   the BatchNorm buffers of the 64-pixel generator; device time (events), median over ``--reps``.
2. ``g_step`` of the ResNet GAN at 64x64 (SAGAN recipe, ``cgan='projection'``, ``hier_latent`` + ``shared_embed``) with
   ``use_ewma_gen`` off and on: wall time with a device synchronisation, one warm-up, the median of ``--iters``, and this
   library's launches per step.  The row with the option off is the code path of the commit before the option: the same row of
   this script run on that commit is the comparison on the same box.
3. ``generate(n=batch)`` on the averaged generator: untruncated, ``truncation=0.5``, and with standing statistics
   (``config.standing_stat_batches`` = 16 batches) in front."""
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


def learner(args, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=64, res_dataset=64, batch_size=args.batch,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=0, cgan='projection', num_classes=10,
                      spectral_norm=True, loss='hinge', gradient_penalty=None, hier_latent=True, shared_embed=128, **kw)
    L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    L.set_requires_grad_disc(False)
    return L


def bench_draws(args, ops):
    rows = {}
    for n in (1 << 20, args.batch * 128):
        rows[f'n={n}'] = {'randn_ms': median_ms(lambda: ops.randn((n,), 1, 0, 'cuda'), args.reps),
                          'trunc_randn_ms': median_ms(lambda: ops.trunc_randn((n,), 0.5, 1, 0, 'cuda'), args.reps)}
    L = learner(args, use_ewma_gen=True)
    table = L.gen_ema._buffer_table()
    rows['ewma_many'] = {'segments': table.n, 'floats': sum(a.numel() for a, _ in table.pairs),
                         'ms': median_ms(lambda: ops.ewma_many(table, 0.9999), args.reps)}
    print(f'draws: {rows}')
    return rows


def bench_step(args):
    from gan_lab_amd import _lib
    rows = {}
    for name, kw in (('use_ewma_gen off', {}), ('use_ewma_gen on', dict(use_ewma_gen=True))):
        L = learner(args, **kw)

        def step():
            L.g_step()
            torch.cuda.synchronize()

        step()
        n0 = _lib.launch_count()
        step()
        rows[name] = {'library_launches': _lib.launch_count() - n0, 'g_step_ms': wall_ms(step, args.iters)}
        print(f'ResNet GAN 64x64, batch {args.batch}, g_step, {name}: {rows[name]}')
        del L
        torch.cuda.empty_cache()
    return rows


def bench_generate(args):
    L = learner(args, use_ewma_gen=True)
    L.g_step()
    rows = {}
    for name, kw in (('untruncated', dict(truncation=None)), ('truncation 0.5', dict(truncation=0.5)),
                     ('truncation 0.5 + standing statistics (16 batches)', dict(truncation=0.5, standing_stats=True))):
        def run():
            L.generate(n=args.batch, **kw)
            torch.cuda.synchronize()

        rows[name] = {'generate_ms': wall_ms(run, args.iters)}
        print(f'generate(n={args.batch}), {name}: {rows[name]}')
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gan_lab_amd import ops
    out = {'batch': args.batch, 'iters': args.iters, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'draws': bench_draws(args, ops), 'g_step': bench_step(args), 'generate': bench_generate(args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
