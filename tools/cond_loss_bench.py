#!/usr/bin/env python3
"""Measure the classifier-based class conditioning of the ResNet GAN (gan_lab_amd/conditional.py; csrc/cond_loss.hip): the loss
ops against their ATen compositions, and what each mode costs a critic and a generator step.

    timeout -k 10 600 python tools/cond_loss_bench.py [--batch 64] [--iters 10] [--reps 20] [--out profiles/cond_loss_bench.json]

1. ``ops.class_cross_entropy`` and ``ops.class_contrastive`` (2C and D2D-CE), forward + backward, at N = 64, 256, 2048 with
   E = 512 and K = 10 / 1000, against the composition ``F.normalize`` + ``mm`` + masks + ``logsumexp`` (``F.cross_entropy``)
   under autograd: device time (events), median over ``--reps``; the forward launches of this library per call (the backward
   runs on autograd's thread, which the library's per-thread counter does not see: 3 for the contrastive op, 1 for the
   cross-entropy, by construction); and the relative error of the loss and of dh against the composition in float64.
2. ``d_step`` and ``g_step`` of the ResNet GAN at 64x64 (the default wgan + wgan-gp, K = 10) per ``cgan`` mode, ``'projection'``
   first: wall time with a device synchronisation, one warm-up, the median of ``--iters``, and this library's launches per step
   on the calling thread.
A failed step raises; the exit status is that of the interpreter."""
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


def aten_contrastive(h, proxy, labels, mode, tau, mp, mn):
    y = labels.long()
    hh, ph = F.normalize(h, dim=1, eps=1e-12), F.normalize(proxy, dim=1, eps=1e-12)
    s, S = (hh * ph[y]).sum(1), hh @ hh.t()
    same = y[:, None] == y[None, :]
    eye = torch.eye(len(y), dtype=torch.bool, device=h.device)
    if mode == '2c':
        u, A = s / tau, (S / tau).masked_fill(eye, float('-inf'))
        D = torch.logsumexp(torch.cat((u[:, None], A), 1), 1)
        M = torch.logsumexp(torch.cat((u[:, None], A.masked_fill(~same, float('-inf'))), 1), 1)
        return (D - M).mean()
    u = (s - mp).clamp(max=0) / tau
    A = ((S - mn).clamp(min=0) / tau).masked_fill(same, float('-inf'))
    return (torch.logsumexp(torch.cat((u[:, None], A), 1), 1) - u).mean()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def bench_ops(args, ops, _lib):
    rows = {}
    tau, mp, mn = 0.5, 0.98, 0.02
    for n in (64, 256, 2048):
        for k in (10, 1000):
            g = torch.Generator().manual_seed(n + k)
            proxy0 = torch.randn(k, 512, generator=g)
            labels = torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
            h0 = torch.randn(n, 512, generator=g) + 0.7 * proxy0[labels.long()]
            z0 = torch.randn(n, k, generator=g) * 3
            h, proxy, z = (t.cuda().requires_grad_(True) for t in (h0, proxy0, z0))
            lab = labels.cuda()
            h64, p64 = (t.double().requires_grad_(True) for t in (h0, proxy0))

            def fwd_bwd(fn, leaves):
                def run():
                    for t in leaves:
                        t.grad = None
                    fn().backward()
                return run

            cases = [('ce', lambda: ops.class_cross_entropy(z, lab), lambda: F.cross_entropy(z, lab.long()), (z,), None)]
            for mode in ('2c', 'd2d'):
                cases.append((mode, lambda mode=mode: ops.class_contrastive(h, proxy, lab, mode=mode, temperature=tau,
                                                                            margin_pos=mp, margin_neg=mn),
                              lambda mode=mode: aten_contrastive(h, proxy, lab, mode, tau, mp, mn), (h, proxy), mode))
            for name, ours, aten, leaves, mode in cases:
                n0 = _lib.launch_count()
                loss = ours()
                row = {'forward_launches': _lib.launch_count() - n0,
                       'kernel_ms': median_ms(fwd_bwd(ours, leaves), args.reps),
                       'aten_ms': median_ms(fwd_bwd(aten, leaves), args.reps)}
                if mode is not None:
                    want = aten_contrastive(h64, p64, labels, mode, tau, mp, mn)
                    dh64, = torch.autograd.grad(want, h64)
                    dh, = torch.autograd.grad(loss, h)
                    row.update(loss_err=rel(loss, want), dh_err=rel(dh, dh64))
                else:
                    row.update(loss_err=rel(loss, F.cross_entropy(z0.double(), labels.long())))
                rows[f'{name} N={n} K={k}'] = row
                print(f'{name} N={n} E=512 K={k}: {row}')
    return rows


def learner(args, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=64, res_dataset=64, batch_size=args.batch,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=0, num_classes=10, **kw)
    L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    return L


def bench_steps(args, _lib):
    real = torch.rand(args.batch, 3, 64, 64, device='cuda') * 2 - 1
    labels = torch.randint(0, 10, (args.batch,), dtype=torch.int32, device='cuda')
    rows = {}
    for mode in ('projection', 'contra', 'reacgan'):
        L = learner(args, cgan=mode)

        def d_step():
            L.d_step(real, labels=labels)
            torch.cuda.synchronize()

        def g_step():
            L.g_step()
            torch.cuda.synchronize()

        rows[mode] = {}
        for what, step, frozen in (('d_step', d_step, True), ('g_step', g_step, False)):
            L.set_requires_grad_disc(frozen)
            step()
            n0 = _lib.launch_count()
            step()
            rows[mode][what] = {'library_launches': _lib.launch_count() - n0, 'ms': wall_ms(step, args.iters)}
        print(f'ResNet GAN 64x64, batch {args.batch}, cgan={mode}: {rows[mode]}')
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
           'ops': bench_ops(args, ops, _lib), 'steps': bench_steps(args, _lib)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
