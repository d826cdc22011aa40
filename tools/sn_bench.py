#!/usr/bin/env python3
"""Time spectral normalisation of the ResNet GAN critic (gan_lab_amd/spectral_norm.py, csrc/spectral.hip).

    timeout -k 10 600 python tools/sn_bench.py [--reps 20] [--iters 5] [--skip-steps] [--out profiles/sn_bench.json]

Part 1 - the kernels alone, on the layer set of the full-width 64-pixel critic (config #5): ``refresh(iterate=True)``,
``refresh(iterate=False)`` and ``backward()``, device time (events), median over ``--reps``, with the bytes each call moves
(the weights W are N floats in all: an iterating refresh reads W three times and writes W_sn once, the other reads it twice;
the backward reads g_sn twice, W_sn once and reads and writes the gradient arena) and the bandwidth that implies.

Part 2 - config #5's main iteration (1 generator + 5 critic iterations at batch 64, through ``learner.train()`` like
bench.py) in four settings: the BASELINE loss (WGAN + WGAN-GP) with spectral_norm off and on, and hinge without a gradient
penalty with spectral_norm off and on.  One warm-up iteration, then the median wall time of ``--iters`` iterations each."""
import argparse
import contextlib
import io
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


def kernels(reps):
    from gan_lab_amd.optim import ParamArena
    from gan_lab_amd.resnetgan.architectures import Discriminator64PixResnet
    from gan_lab_amd.spectral_norm import SpectralNorm
    d = Discriminator64PixResnet(spectral_norm=True).cuda()
    arena = ParamArena(d.named_parameters(), 'cuda')
    sn = SpectralNorm(d, arena)
    n = sum(sn.sizes)
    sn.gflat.normal_()
    out = {'layers': len(sn.names), 'weights': n, 'shapes': [list(s) for s in sn.shapes]}
    for name, fn, passes in (('refresh_iterate', lambda: sn.refresh(True), 4), ('refresh', lambda: sn.refresh(False), 3),
                             ('backward', sn.backward, 5)):
        fn()
        ms = statistics.median(timed(fn) for _ in range(reps))
        out[name] = {'ms': round(ms, 4), 'bytes': 4 * n * passes, 'GB_per_s': round(4 * n * passes / ms / 1e6, 1)}
    return out


def step_ms(iters, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    from gan_lab_amd.utils.data_utils import SyntheticImageLoader
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, batch_size=64, res_samples=64, res_dataset=64,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=1234, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        L = GANLearner(cfg)
    dl = SyntheticImageLoader(1 << 22, 64, 64, device='cuda')
    times = []
    for i in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            L.train(dl, num_main_iters=1)
        torch.cuda.synchronize()
        if i:
            times.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(times), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--skip-steps', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    res = {'kernels_64px_critic': kernels(a.reps)}
    print(json.dumps(res['kernels_64px_critic']), flush=True)
    if not a.skip_steps:
        res['config5_main_iteration_ms'] = {}
        for name, kw in (('wgan+wgan-gp', {}), ('wgan+wgan-gp, spectral_norm', {'spectral_norm': True}),
                         ('hinge, no penalty', {'loss': 'hinge', 'gradient_penalty': None}),
                         ('hinge, no penalty, spectral_norm', {'loss': 'hinge', 'gradient_penalty': None, 'spectral_norm': True})):
            res['config5_main_iteration_ms'][name] = step_ms(a.iters, **kw)
            print(name, res['config5_main_iteration_ms'][name], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
