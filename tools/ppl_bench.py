#!/usr/bin/env python3
"""Time the three kernels of the perceptual path length (gan_lab_amd/ppl.py; csrc/ppl.hip) against their ATen compositions, and one
evaluation of a full-size StyleGAN against the same number of generator passes alone.

    timeout -k 10 600 python tools/ppl_bench.py [--n 1024] [--dim 512] [--res 1024] [--pairs 32] [--batch 4] [--reps 5] [--out FILE]

Kernels: ``ops.ppl_endpoints`` on (n, dim) rows in both modes against slerp / lerp composed from ATen ops in fp32;
``ops.row_sqdist`` on (n, 3 * 64 * 64) rows against ``((x - y) ** 2).sum(1)`` in fp32 and in fp64; ``ops.trimmed_mean`` on 100000
values against ``torch.sort`` + two index reads + a masked fp64 mean.  Evaluation: ``ppl.generator_path_length`` of a randomly
initialised StyleGAN generator at ``--res`` over ``--pairs`` pairs in batches of ``--batch`` (2 x batch images per generator
call), in W and in Z, against the bare ``z_to_w`` + ``synthesis`` calls on as many rows.  Medians of ``--reps`` runs after one
warm-up, device events.  Writes one JSON line (default profiles/ppl_bench.json)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
    return round(statistics.median(out), 4)


def aten_slerp(a, b, t, eps):
    ah, bh = a / a.norm(dim=1, keepdim=True), b / b.norm(dim=1, keepdim=True)
    d = (ah * bh).sum(1, keepdim=True).clamp(-1, 1)
    c = bh - d * ah
    ch = c / c.norm(dim=1, keepdim=True)
    p = torch.stack([t, t + eps]).unsqueeze(-1) * torch.acos(d)
    r = ah * torch.cos(p) + ch * torch.sin(p)
    return r / r.norm(dim=2, keepdim=True) * math.sqrt(a.shape[1])


def aten_trimmed(v):
    s, n = torch.sort(v)[0], v.numel()
    lo, hi = s[int(math.floor(0.01 * (n - 1)))], s[int(math.ceil(0.99 * (n - 1)))]
    keep = (s >= lo) & (s <= hi)
    return (s.double() * keep).sum() / keep.sum(), lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--dim', type=int, default=512)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ppl_bench.json'))
    args = ap.parse_args()
    from gan_lab_amd import ops, ppl, progressive as P
    from gan_lab_amd.stylegan.architectures import StyleGenerator
    n, d, eps = args.n, args.dim, 1e-4
    g = torch.Generator(device='cuda').manual_seed(0)
    a, b = torch.randn(n, d, device='cuda', generator=g), torch.randn(n, d, device='cuda', generator=g)
    out = {'n': n, 'dim': d, 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}

    t = ops.ppl_endpoints(a, b, eps, 'slerp', 'full', 1, 0)[0]
    out['endpoints'] = {'slerp_kernel_ms': timed(lambda: ops.ppl_endpoints(a, b, eps, 'slerp', 'full', 1, 0), args.reps),
                        'slerp_aten_ms': timed(lambda: aten_slerp(a, b, t, eps), args.reps),
                        'lerp_kernel_ms': timed(lambda: ops.ppl_endpoints(a, b, eps, 'lerp', 'full', 1, 0), args.reps),
                        'lerp_aten_ms': timed(lambda: a + (b - a) * torch.stack([t, t + eps]).unsqueeze(-1), args.reps)}
    print('endpoints', out['endpoints'])

    rows = 3 * 64 * 64
    x, y = torch.randn(n, rows, device='cuda', generator=g), torch.randn(n, rows, device='cuda', generator=g)
    x64, y64 = x.double(), y.double()
    out['row_sqdist'] = {'rows': n, 'width': rows, 'kernel_ms': timed(lambda: ops.row_sqdist(x, y), args.reps),
                         'aten_fp32_ms': timed(lambda: ((x - y) ** 2).sum(1), args.reps),
                         'aten_fp64_ms': timed(lambda: ((x64 - y64) ** 2).sum(1), args.reps)}
    want = ((x64 - y64) ** 2).sum(1)
    out['row_sqdist']['rel_err'] = {'kernel': float(((ops.row_sqdist(x, y).double() - want).abs() / want).max()),
                                    'aten_fp32': float(((((x - y) ** 2).sum(1)).double() - want).abs().div(want).max())}
    print('row_sqdist', out['row_sqdist'])
    del x, y, x64, y64, want

    v = torch.randn(100000, device='cuda', generator=g) ** 2
    out['trimmed_mean'] = {'values': v.numel(), 'kernel_ms': timed(lambda: ops.trimmed_mean(v), args.reps),
                           'aten_ms': timed(lambda: aten_trimmed(v), args.reps)}
    print('trimmed_mean', out['trimmed_mean'])

    # ---- one evaluation of a full-size StyleGAN ---------------------------------------------------------------------------------
    torch.manual_seed(0)
    P.StyleGAN.reset_state()
    gen = StyleGenerator(final_res=args.res, blur_type='binomial')
    for _ in range(int(math.log2(args.res)) - 2):
        gen.increase_scale()
        gen.scale_inc_metadata_updated = False               # no critic here to take the second half of the growth step
    gen.fade_in_phase = False
    gen.alpha = 1
    gen.cuda().eval()
    gen.use_truncation_trick = False
    pairs, batch = args.pairs, args.batch
    z = torch.randn(2 * batch, gen.len_latent, device='cuda', generator=g)
    calls = (pairs + batch - 1) // batch

    def passes():
        with torch.no_grad():
            for k in range(calls):
                maps = ppl.noise_maps(gen, 7, k, 'cuda')
                gen.synthesis(gen.z_to_w(z), noise=maps)

    ev = {'res': args.res, 'pairs': pairs, 'batch': batch, 'generator_calls': calls, 'images_per_call': 2 * batch}
    ev['generator_passes_alone_ms'] = timed(passes, args.reps)
    for space in ('w', 'z'):
        res = {}

        def run():
            res.update(ppl.generator_path_length(gen, pairs, space, batch=batch, seed=0))
        ev[f'evaluation_{space}_ms'] = timed(run, args.reps)
        ev[f'ppl_{space}'] = res['ppl']
    out['evaluation'] = ev
    print('evaluation', ev)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
