#!/usr/bin/env python3
"""Measure latent-space projection (gan_lab_amd/project.py; csrc/project.hip).

    timeout -k 10 540 python tools/project_bench.py [--reps 10] [--res 1024] [--out profiles/project_bench.json]

1. ``ops.pyramid_mse`` forward + gradient against the ATen ``avg_pool2d`` composition under autograd, six levels, at
   8 x 3 x 1024^2 and 16 x 3 x 256^2: device time (events), this library's launches per call.
2. A projection iteration of StyleGAN at ``--res`` (synthesis -> pyramid_mse -> gradient to the dlatents -> project_step, with
   its exploration-noise draw) for N = 1 and 4, against the generator's forward plus its input-gradient backward alone (the same
   synthesis with a sum for a loss): wall time with a device synchronisation.
Each pair is timed in alternation - one run of one, one of the other, ``--reps`` times - and the medians are reported."""
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


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(first, second, reps, clock):
    """Medians of ``first`` and ``second`` timed alternately (two warm-ups each)."""
    for _ in range(2):
        first()
        second()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(clock(first))
        b.append(clock(second))
    return round(statistics.median(a), 4), round(statistics.median(b), 4)


def bench_loss(args, ops, _lib):
    weights = [1.] * 6
    rows = {}
    for shape in ((8, 3, 1024, 1024), (16, 3, 256, 256)):
        x = torch.randn(shape, device='cuda', requires_grad=True)
        t = torch.randn(shape, device='cuda')
        ones = torch.ones(shape[0], device='cuda')

        def ours():
            loss, _ = ops.pyramid_mse(x, t, weights)
            return torch.autograd.grad(loss, x, grad_outputs=ones)[0]

        def aten():
            d, loss = x - t, 0.
            for w in weights:
                loss = loss + w * (d * d).mean(dim=(1, 2, 3))
                d = F.avg_pool2d(d, 2)
            return torch.autograd.grad(loss, x, grad_outputs=ones)[0]

        n0 = _lib.launch_count()
        ours()
        launches = _lib.launch_count() - n0
        ms_ours, ms_aten = interleaved(ours, aten, args.reps, event_ms)
        rows['x'.join(map(str, shape))] = {'library_launches': launches, 'kernel_ms': ms_ours, 'aten_ms': ms_aten}
        print(f'pyramid_mse fwd + gradient {shape}: {rows["x".join(map(str, shape))]}')
        del x, t
        torch.cuda.empty_cache()
    return rows


def bench_iteration(args, ops, _lib):
    from gan_lab_amd import project
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    cfg = make_config('stylegan', dev='cuda', pin_memory=False, res_samples=args.res, res_dataset=args.res, init_res=args.res,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=0)
    gen = StyleGANLearner(cfg).gen_model.eval()
    for p in gen.parameters():
        p.requires_grad_(False)
    layers, d = len(gen.gen_layers), gen.len_dlatent
    maps = [torch.randn(1, 1, 4 * 2 ** (k // 2), 4 * 2 ** (k // 2), device='cuda') for k in range(layers)]
    weights = (1.,) * ops.pyramid_max_levels(args.res)
    hyper = ops.check_project_schedule(1000, {})
    rows = {}
    for n in (1, 4):
        target = torch.randn(n, 3, args.res, args.res, device='cuda')
        w_opt = torch.randn(n, d, device='cuda')
        m, v = torch.zeros_like(w_opt), torch.zeros_like(w_opt)
        step = torch.zeros(1, dtype=torch.int32, device='cuda')
        w_std = torch.ones((), device='cuda')
        w_in = torch.empty(n, layers, d, device='cuda', requires_grad=True)
        ones = torch.ones(n, device='cuda')
        ops.project_step(w_opt, None, m, v, step, torch.zeros_like(w_opt), w_std, w_in.detach(), hyper)

        def iteration():
            loss, _ = ops.pyramid_mse(gen.synthesis(w_in, noise=maps), target, weights)
            grad, = torch.autograd.grad(loss, w_in, grad_outputs=ones)
            noise = ops.randn(tuple(w_opt.shape), project._substream(0, 2), 0, 'cuda')
            ops.project_step(w_opt, grad, m, v, step, noise, w_std, w_in.detach(), hyper)

        def generator_only():
            img = gen.synthesis(w_in, noise=maps)
            torch.autograd.grad(img, w_in, grad_outputs=target)

        n0 = _lib.launch_count()
        iteration()
        mid = _lib.launch_count()
        generator_only()
        launches = (mid - n0, _lib.launch_count() - mid)
        ms_it, ms_gen = interleaved(iteration, generator_only, args.reps, wall_ms)
        rows[f'N={n}'] = {'iteration_ms': ms_it, 'generator_fwd_bwd_ms': ms_gen, 'overhead_ms': round(ms_it - ms_gen, 4),
                          'library_launches': {'iteration': launches[0], 'generator_fwd_bwd': launches[1]}}
        print(f'StyleGAN {args.res}x{args.res} projection iteration, N = {n}: {rows[f"N={n}"]}')
        del target
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('project_bench measures on the GPU; there is no CPU path')
    from gan_lab_amd import _lib, ops
    out = {'reps': args.reps, 'res': args.res, 'device': torch.cuda.get_device_name(0),
           'pyramid_mse': bench_loss(args, ops, _lib), 'iteration': bench_iteration(args, ops, _lib)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
