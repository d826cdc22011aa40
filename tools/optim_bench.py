#!/usr/bin/env python3
"""Times one update of a StyleGAN-1024 generator-sized arena per fused optimiser against ``torch.optim`` (foreach) on the same
tensor shapes, and prints the effective bandwidth of each.

    python tools/optim_bench.py [--floats N] [--tensors K] [--iters I]

The arena is ``--floats`` fp32 values (default 26.2e6, the parameter count of the 1024-pixel StyleGAN generator) cut into
``--tensors`` parameters (default 150) for torch; the fused optimisers see them as one run.  Traffic per update: reads of p, g and
every state buffer plus writes of p and every state buffer, 4 bytes each.  Optimistic Adam has no torch counterpart: its row
compares with torch's Adam, which moves one buffer less."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--floats', type=int, default=26_200_000)
    ap.add_argument('--tensors', type=int, default=150)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args(argv)
    from gan_lab_amd import optim
    each = max(args.floats // args.tensors // 4 * 4, 4)
    n = each * args.tensors
    rows = [('adam', optim.FusedAdam, dict(betas=(0., .99)), torch.optim.Adam, dict(betas=(0., .99)), 2),
            ('rmsprop', optim.FusedRMSprop, dict(alpha=.99), torch.optim.RMSprop, dict(alpha=.99), 1),
            ('rmsprop+momentum', optim.FusedRMSprop, dict(alpha=.99, momentum=.9), torch.optim.RMSprop, dict(alpha=.99, momentum=.9), 2),
            ('sgd', optim.FusedSGD, dict(), torch.optim.SGD, dict(), 0),
            ('momentum', optim.FusedSGD, dict(momentum=.9), torch.optim.SGD, dict(momentum=.9), 1),
            ('oadam', optim.FusedOptimisticAdam, dict(betas=(0., .99)), torch.optim.Adam, dict(betas=(0., .99)), 3)]
    print(f'{n} floats in {args.tensors} parameters, {args.iters} timed updates each')
    for name, fused_cls, fkw, torch_cls, tkw, n_state in rows:
        named = [(str(i), torch.nn.Parameter(torch.randn(each, device='cuda'))) for i in range(args.tensors)]
        arena = optim.ParamArena(named, 'cuda')
        arena.gflat.normal_()
        fused = fused_cls(arena.params, lr=1e-3, **fkw)
        t_fused = _time(fused.step, args.iters)
        plain = [torch.nn.Parameter(torch.randn(each, device='cuda')) for _ in range(args.tensors)]
        for p in plain:
            p.grad = torch.randn_like(p)
        ref = torch_cls(plain, lr=1e-3, foreach=True, **tkw)
        t_torch = _time(ref.step, args.iters)
        gb = lambda states: 4.0 * n * (3 + 2 * states) / 1e9      # noqa: E731
        torch_states = n_state if name != 'oadam' else 2
        print(f'{name:18s} fused {t_fused * 1e6:9.1f} us {gb(n_state) / t_fused:8.1f} GB/s | torch foreach {t_torch * 1e6:9.1f} us '
              f'{gb(torch_states) / t_torch:8.1f} GB/s | x{t_torch / t_fused:.2f}')


if __name__ == '__main__':
    main()
