#!/usr/bin/env python3
"""Time class conditioning (gan_lab_amd/conditional.py; csrc/cond.hip) against its ATen composition and against the unconditional
iteration.

    timeout -k 10 300 python tools/cond_bench.py [--reps 20] [--batch 64] [--classes 10] [--iters 5] [--out profiles/cond_bench.json]

1. Conditional BatchNorm, forward + backward, at the norm shapes of the 64-pixel generator: ``ops.cond_batch_norm`` against
   ``F.batch_norm`` without affine, then the two gathers and the affine, under autograd.
2. The projection, forward + backward, at the 64-pixel critic's feature width (F = 8192) and the 32-pixel one's (F = 128):
   ``ops.class_projection`` against ``(W[l] * f).sum(1)``.
3. One main iteration (1 generator step, ``num_disc_iters`` critic steps) of the ResNet GAN at 64x64, batch 64, with
   ``cgan='projection'`` against the same iteration with ``cgan=None``: wall time with a device synchronisation, one warm-up, then
   the median of ``--iters``.
Device time (events), median over ``--reps``, for 1 and 2."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (C, H) of the 64-pixel generator's norms at fmap 64: the first and the last norm of the stack and one in between
NORM_SHAPES = {'block 1 in (512 ch, 4x4)': (512, 4), 'block 3 out (128 ch, 32x32)': (128, 32), 'final (64 ch, 64x64)': (64, 64)}
PROJ_SHAPES = {'resnet64 critic (F 8192)': 8192, 'resnet32 critic (F 128)': 128}


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
    return statistics.median(timed(run) for _ in range(reps))


def aten_cbn(x, weight, bias, labels):
    xhat = F.batch_norm(x, None, None, None, None, True, 0.0, 1e-5)
    return F.relu(xhat * weight[labels][:, :, None, None] + bias[labels][:, :, None, None])


def bench_norm(args, ops):
    rows = {}
    g = torch.Generator().manual_seed(0)
    for name, (c, h) in NORM_SHAPES.items():
        x = torch.randn(args.batch, c, h, h, generator=g).cuda().requires_grad_(True)
        weight = (torch.randn(args.classes, c, generator=g) * 0.1 + 1).cuda().requires_grad_(True)
        bias = (torch.randn(args.classes, c, generator=g) * 0.1).cuda().requires_grad_(True)
        labels = torch.randint(0, args.classes, (args.batch,), generator=g, dtype=torch.int32).cuda()
        gy = torch.randn(args.batch, c, h, h, generator=g).cuda()
        rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
        long_labels = labels.long()
        fused = median_ms(lambda: torch.autograd.grad(ops.cond_batch_norm(x, weight, bias, labels, rm, rv, True, act_slope=0.0),
                                                      (x, weight, bias), gy), args.reps)
        aten = median_ms(lambda: torch.autograd.grad(aten_cbn(x, weight, bias, long_labels), (x, weight, bias), gy), args.reps)
        rows[name] = {'C': c, 'H': h, 'fused_fwd_bwd_ms': round(fused, 4), 'aten_fwd_bwd_ms': round(aten, 4)}
        print(f'cond. BatchNorm + ReLU, {name}: fused {fused:.3f} ms, ATen composition {aten:.3f} ms')
    return rows


def bench_proj(args, ops):
    rows = {}
    g = torch.Generator().manual_seed(1)
    for name, nf in PROJ_SHAPES.items():
        f = torch.randn(args.batch, nf, generator=g).cuda().requires_grad_(True)
        W = (torch.randn(args.classes, nf, generator=g) / nf ** 0.5).cuda().requires_grad_(True)
        base = torch.randn(args.batch, generator=g).cuda().requires_grad_(True)
        labels = torch.randint(0, args.classes, (args.batch,), generator=g, dtype=torch.int32).cuda()
        cot = torch.randn(args.batch, generator=g).cuda()
        long_labels = labels.long()
        fused = median_ms(lambda: torch.autograd.grad(ops.class_projection(f, W, labels, base), (f, W, base), cot), args.reps)
        aten = median_ms(lambda: torch.autograd.grad(base + (W[long_labels] * f).sum(1), (f, W, base), cot), args.reps)
        rows[name] = {'F': nf, 'fused_fwd_bwd_ms': round(fused, 4), 'aten_fwd_bwd_ms': round(aten, 4)}
        print(f'projection, {name}: fused {fused:.3f} ms, ATen (W[l] * f).sum(1) {aten:.3f} ms')
    return rows


def bench_iteration(args):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    rows = {}
    g = torch.Generator().manual_seed(2)
    reals = (torch.rand(args.batch, 3, 64, 64, generator=g) * 2 - 1).cuda()
    labels = torch.randint(0, args.classes, (args.batch,), generator=g, dtype=torch.int32).cuda()
    for name, kw in (('cgan=None', {}), ("cgan='projection'", {'cgan': 'projection', 'num_classes': args.classes})):
        cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=64, res_dataset=64, batch_size=args.batch,
                          num_iters_save_model=10 ** 9, log_every=0, random_seed=0, **kw)
        L = GANLearner(cfg)
        L.gen_model.train()
        L.disc_model.train()

        def iteration():
            L.set_requires_grad_disc(False)
            L.g_step()
            L.set_requires_grad_disc(True)
            for _ in range(cfg.num_disc_iters):
                L.d_step(reals, labels=labels if kw else None)
            torch.cuda.synchronize()

        iteration()
        times = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            iteration()
            times.append((time.perf_counter() - t0) * 1e3)
        rows[name] = {'iteration_ms': round(statistics.median(times), 3), 'num_disc_iters': cfg.num_disc_iters}
        print(f'ResNet GAN 64x64, batch {args.batch}, {name}: {rows[name]["iteration_ms"]:.1f} ms per main iteration')
        del L
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gan_lab_amd import ops
    out = {'batch': args.batch, 'classes': args.classes, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'cond_batch_norm': bench_norm(args, ops), 'projection': bench_proj(args, ops), 'iteration': bench_iteration(args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
