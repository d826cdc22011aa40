#!/usr/bin/env python3
"""Measure BigGAN's generator conditioning (gan_lab_amd/hier_latent.py; csrc/hier.hip): errors against float64, time and launch
counts against its ATen composition and against the generator step without it.

    timeout -k 10 300 python tools/hier_bench.py [--reps 20] [--batch 64] [--classes 10] [--embed 128] [--iters 5]
                                                 [--out profiles/hier_bench.json]

1. Errors: the batched modulation (forward, dz, d shared, every dW) and ``ops.mod_batch_norm`` (y, gx, d gain, d shift) at the
   64-pixel generator's full width against the float64 run of tests/hier_reference.py, next to the fp32 CPU run's own error.
2. The batched modulation of the 64-pixel generator (8 norms, 16 jobs, T = 2 * sum C, D = chunk + E), forward + backward:
   ``ops.hier_modulate`` against embedding, cat and two ``F.linear`` per norm under autograd; device time and kernel launches.
3. ``ops.mod_batch_norm``, forward + backward, at three norm shapes of that generator against ``F.batch_norm`` without affine
   followed by the per-sample affine and ReLU.
4. The generator step (``g_step``) of the ResNet GAN at 64x64 with the SAGAN recipe and ``cgan='projection'``: options off (class
   tables) against ``hier_latent`` + ``shared_embed``; wall time with a device synchronisation, one warm-up, then the median of
   ``--iters``; and this library's launches per step.
Device time (events), median over ``--reps``, for 2 and 3.  ATen launches are counted with the profiler's kernel events."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

# C of the 16 norms' inputs of the 64-pixel generator at fmap 64, len_latent 128: block b has norms of (ni, nf)
BLOCK_CHANNELS = ((512, 512), (512, 256), (256, 128), (128, 64))
NORM_SHAPES = {'block 1 in (512 ch, 4x4)': (512, 4), 'block 3 out (128 ch, 32x32)': (128, 32), 'block 4 out (64 ch, 64x64)': (64, 64)}


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


def kernel_launches(run):
    """Device kernels one call of ``run`` launches, whoever launched them."""
    from torch.profiler import ProfilerActivity, profile
    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
               and 'memset' not in e.name.lower())


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _jobs(args, g):
    import hier_reference as ref
    first, chunks = ref.chunk_layout(128, 4)
    jobs = []
    for (ca, cb), (zo, zl) in zip(BLOCK_CHANNELS, chunks):
        for c in (ca, cb):
            for one in (1.0, 0.0):
                jobs.append((torch.randn(c, zl + args.embed, generator=g) * 0.05, zo, zl, 1.0, one))
    return jobs


def bench_modulation(args, ops):
    import hier_reference as ref
    g = torch.Generator().manual_seed(0)
    jobs = _jobs(args, g)
    z = torch.randn(args.batch, 128, generator=g)
    shared = torch.randn(args.classes, args.embed, generator=g)
    labels = torch.randint(0, args.classes, (args.batch,), generator=g, dtype=torch.int32)
    T = sum(j[0].shape[0] for j in jobs)
    cot = torch.randn(args.batch, T, generator=g)
    want = ref.modulation_with_grads(z, jobs, shared, labels, cot, torch.float64)
    cpu = ref.modulation_with_grads(z, jobs, shared, labels, cot, torch.float32)
    zc, sc = z.cuda().requires_grad_(True), shared.cuda().requires_grad_(True)
    Ws = [j[0].cuda().requires_grad_(True) for j in jobs]
    lc, cc = labels.cuda(), cot.cuda()
    table = ops.HierTable([dict(w=W, z_off=j[1], z_len=j[2], scale=j[3], one=j[4]) for W, j in zip(Ws, jobs)], 128, sc)

    def fused():
        return (lambda out: (out,) + torch.autograd.grad(out, [zc, sc] + Ws, cc))(ops.hier_modulate(table, zc, lc))

    def aten():
        e = F.embedding(lc.long(), sc)
        outs = [j[4] + j[3] * F.linear(torch.cat((zc[:, j[1]:j[1] + j[2]], e), dim=1), W) for W, j in zip(Ws, jobs)]
        out = torch.cat(outs, dim=1)
        return (out,) + torch.autograd.grad(out, [zc, sc] + Ws, cc)

    got = fused()
    names = ['out', 'dz', 'dshared'] + [f'dW{i}' for i in range(len(jobs))]
    errs = {n: (rel_err(a, b), rel_err(c, b)) for n, a, b, c in zip(names, got, want, cpu)}
    worst_w = max((errs[n] for n in names[3:]), key=lambda t: t[0])
    rows = {'T': T, 'D': jobs[0][0].shape[1], 'jobs': len(jobs),
            'rel_err_gpu_cpu': {'out': errs['out'], 'dz': errs['dz'], 'dshared': errs['dshared'], 'worst dW': worst_w},
            'fused_ms': round(median_ms(fused, args.reps), 4), 'aten_ms': round(median_ms(aten, args.reps), 4),
            'fused_launches': kernel_launches(fused), 'aten_launches': kernel_launches(aten)}
    print(f'modulation, {len(jobs)} jobs, N {args.batch}, T {T}, D {rows["D"]}: fused {rows["fused_ms"]:.3f} ms / '
          f'{rows["fused_launches"]} launches, ATen {rows["aten_ms"]:.3f} ms / {rows["aten_launches"]} launches; '
          f'errors (gpu, cpu) {rows["rel_err_gpu_cpu"]}')
    return rows


def bench_norm(args, ops):
    import hier_reference as ref
    rows = {}
    g = torch.Generator().manual_seed(1)
    for name, (c, h) in NORM_SHAPES.items():
        x = torch.randn(args.batch, c, h, h, generator=g)
        flat = torch.randn(args.batch, 2 * c, generator=g) * 0.1
        flat[:, :c] += 1
        gy = torch.randn(args.batch, c, h, h, generator=g)
        xc, fc, gc = x.cuda().requires_grad_(True), flat.cuda().requires_grad_(True), gy.cuda()
        rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()

        def fused():
            y = ops.mod_batch_norm(xc, fc[:, :c], fc[:, c:], rm, rv, True, act_slope=0.0)
            return (y,) + torch.autograd.grad(y, (xc, fc), gc)

        def aten():
            xhat = F.batch_norm(xc, None, None, None, None, True, 0.0, 1e-5)
            y = F.relu(xhat * fc[:, :c, None, None] + fc[:, c:, None, None])
            return (y,) + torch.autograd.grad(y, (xc, fc), gc)

        rows[name] = {'fused_ms': round(median_ms(fused, args.reps), 4), 'aten_ms': round(median_ms(aten, args.reps), 4)}
        if h <= 32:          # the float64 reference of the largest map is slow on the host and says nothing new
            want = ref.mod_batch_norm_with_grads(x, flat[:, :c], flat[:, c:], gy, torch.float64)
            cpu = ref.mod_batch_norm_with_grads(x, flat[:, :c], flat[:, c:], gy, torch.float32)
            y = ops.mod_batch_norm(xc, fc[:, :c], fc[:, c:], rm, rv, True)
            gx, gf = torch.autograd.grad(y, (xc, fc), gc)
            got = (y, gx, gf[:, :c], gf[:, c:])
            rows[name]['rel_err_gpu_cpu'] = {n: (rel_err(a, b), rel_err(cc, b))
                                             for n, a, b, cc in zip(('y', 'gx', 'dgain', 'dshift'), got, want, cpu)}
        print(f'mod_batch_norm, {name}: {rows[name]}')
    return rows


def bench_step(args):
    from gan_lab_amd import _lib
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    rows = {}
    base = dict(cgan='projection', num_classes=args.classes, spectral_norm=True, loss='hinge', gradient_penalty=None)
    for name, kw in (('options off (class tables)', {}), ('hier_latent + shared_embed', dict(hier_latent=True,
                                                                                             shared_embed=args.embed))):
        cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=64, res_dataset=64, batch_size=args.batch,
                          num_iters_save_model=10 ** 9, log_every=0, random_seed=0, **base, **kw)
        L = GANLearner(cfg)
        L.gen_model.train()
        L.disc_model.train()
        L.set_requires_grad_disc(False)

        def step():
            L.g_step()
            torch.cuda.synchronize()

        step()
        n0 = _lib.launch_count()
        step()
        launches = _lib.launch_count() - n0
        times = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            step()
            times.append((time.perf_counter() - t0) * 1e3)
        rows[name] = {'g_step_ms': round(statistics.median(times), 3), 'library_launches': launches,
                      'all_kernel_launches': kernel_launches(step),
                      'generator_parameters': sum(p.numel() for p in L.gen_model.parameters())}
        print(f'ResNet GAN 64x64, batch {args.batch}, g_step, {name}: {rows[name]}')
        del L
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--embed', type=int, default=128)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gan_lab_amd import ops
    out = {'batch': args.batch, 'classes': args.classes, 'embed': args.embed, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'modulation': bench_modulation(args, ops), 'mod_batch_norm': bench_norm(args, ops),
           'g_step': bench_step(args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
