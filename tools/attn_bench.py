#!/usr/bin/env python3
"""Time the fused self-attention core (gan_lab_amd/ops.py: attention; csrc/attention.hip) against the ATen composition.

    timeout -k 10 300 python tools/attn_bench.py [--reps 20] [--batch 64] [--out profiles/attn_bench.json]

At the two network shapes - the 64-pixel networks' block (Dk 16, Dv 64, L 1024, S 256) and the 32-pixel ones' (Dk 32, Dv 128,
L 256, S 64), full width - it runs forward + backward of ``ops.attention`` and of ``bmm -> softmax -> bmm`` under autograd on
the same operands: device time (events), median over ``--reps``, and the bytes each allocates at its peak (the composition
keeps the (N, L, S) map for its backward and builds a second one in it)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {'resnet64 (ni 128, 32x32 map)': (16, 64, 1024, 256), 'resnet32 (ni 256, 16x16 map)': (32, 128, 256, 64)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def composed(q, k, v):
    p = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=2)
    return torch.bmm(v, p.transpose(1, 2))


def measure(fn, q, k, v, d_o, reps):
    def run():
        return torch.autograd.grad(fn(q, k, v), (q, k, v), d_o)
    run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    return statistics.median(timed(run) for _ in range(reps)), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gan_lab_amd import ops
    out = {'batch': args.batch, 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'shapes': {}}
    for name, (dk, dv, l, s) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        a = (3.0 / dk ** 0.5) ** 0.5
        q = (torch.randn(args.batch, dk, l, generator=g) * a).cuda().requires_grad_(True)
        k = (torch.randn(args.batch, dk, s, generator=g) * a).cuda().requires_grad_(True)
        v = torch.randn(args.batch, dv, s, generator=g).cuda().requires_grad_(True)
        d_o = torch.randn(args.batch, dv, l, generator=g).cuda()
        fused_ms, fused_b = measure(ops.attention, q, k, v, d_o, args.reps)
        aten_ms, aten_b = measure(composed, q, k, v, d_o, args.reps)
        row = {'Dk': dk, 'Dv': dv, 'L': l, 'S': s, 'fused_fwd_bwd_ms': round(fused_ms, 4), 'aten_fwd_bwd_ms': round(aten_ms, 4),
               'fused_peak_bytes': fused_b, 'aten_peak_bytes': aten_b, 'map_bytes': args.batch * l * s * 4}
        out['shapes'][name] = row
        print(f'{name}: fused {fused_ms:.3f} ms ({fused_b / 1e6:.1f} MB), ATen bmm/softmax/bmm {aten_ms:.3f} ms '
              f'({aten_b / 1e6:.1f} MB); one (N, L, S) map = {row["map_bytes"] / 1e6:.1f} MB')
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
