"""DiffAugment on the MI355X: the forward / backward kernels (csrc/augment.hip) at 32 x 3 x 1024^2, and the headline step
(StyleGAN 1024^2, batch 32, bench.py's learner) with diffaugment='color,translation,cutout' against off, alternating the
two in one process.  Prints one JSON line per measurement.

    python tools/diffaug_bench.py [--reps 50] [--steps 20] [--warmup 3] [--no-step]

Two byte counts per kernel.  ``bytes``: from shapes - the color part reads its input once more for the per-sample sum (the
backward's masked sum reads all of the cotangent), the apply pass reads the input and writes the output once.  ``bytes_live``:
the apply pass reads only the sources of live pixels (not cut, sourced from inside the image; the kernel skips a 16-byte quad
none of whose pixels is live), counted per pixel from the drawn parameters - the traffic the kernel actually needs, and the
basis of ``tb_per_s_live``."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return times[len(times) // 2], times[0]


def live_fraction(torch, p, h, w, mask):
    """Fraction of output pixels whose value is read from the input (DESIGN.md "DiffAugment": not cut, source inside)."""
    from gan_lab_amd import augment
    n = p.shape[0]
    _, _, ch, cw = augment.sizes(h, w)
    ii = torch.arange(h, device=p.device).view(1, h, 1)
    jj = torch.arange(w, device=p.device).view(1, 1, w)
    live = torch.ones(n, h, w, dtype=torch.bool, device=p.device)
    if mask & augment.TRANSLATION:
        si, sj = ii + p[:, 3].long().view(n, 1, 1), jj + p[:, 4].long().view(n, 1, 1)
        live &= (si >= 0) & (si < h) & (sj >= 0) & (sj < w)
    if mask & augment.CUTOUT:
        r0, c0 = (p[:, 5].long() - ch // 2).view(n, 1, 1), (p[:, 6].long() - cw // 2).view(n, 1, 1)
        live &= ~((ii >= r0) & (ii < r0 + ch) & (jj >= c0) & (jj < c0 + cw))
    return live.float().mean().item()


def kernels(torch, reps, n=32, h=1024):
    from gan_lab_amd import augment, ops, rng
    x = torch.rand(n, 3, h, h, device='cuda') * 2 - 1
    g = torch.randn(n, 3, h, h, device='cuda')
    rng.manual_seed(1)
    p = rng.augment_params(n, h, h)
    plane = x.numel() * 4
    for policy in ('color,translation,cutout', 'translation,cutout', 'color'):
        mask = augment.parse_policy(policy)
        passes = 3 if mask & augment.COLOR else 2
        for direction, fn in (('forward', lambda: ops.k_diffaug(x, p, mask)),
                              ('backward', lambda: ops.k_diffaug(g, p, mask, adjoint=True))):
            med, best = _time_ms(torch, fn, reps)
            nbytes = passes * plane
            live = live_fraction(torch, p, h, h, mask)
            nlive = int((passes - 1 + live) * plane)
            print(json.dumps(dict(what='diffaug_kernel', policy=policy, direction=direction, shape=[n, 3, h, h],
                                  ms_median=round(med, 4), ms_best=round(best, 4), bytes=nbytes,
                                  tb_per_s_median=round(nbytes / (med * 1e-3) / 1e12, 3), live_fraction=round(live, 4),
                                  bytes_live=nlive, tb_per_s_live=round(nlive / (med * 1e-3) / 1e12, 3))), flush=True)


def step(torch, steps, warmup, res=1024, batch=32):
    import bench
    learners = {}
    for policy in (None, 'color,translation,cutout'):
        learners[policy] = bench.build_learner(res, batch, 'cuda', 'f32', 'stylegan', diffaugment=policy)
    real = torch.rand(batch, 3, res, res, device='cuda') * 2 - 1
    times = {k: [] for k in learners}
    for it in range(warmup + steps):
        for policy, L in learners.items():         # alternate off / on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bench.one_step(L, real)
            torch.cuda.synchronize()
            if it >= warmup:
                times[policy].append((time.perf_counter() - t0) * 1e3)
    for policy, ts in times.items():
        ts = sorted(ts)
        q1, q3 = ts[len(ts) // 4], ts[(3 * len(ts)) // 4]
        print(json.dumps(dict(what='diffaug_step', diffaugment=policy, res=res, batch=batch, steps=len(ts),
                              ms_median=round(ts[len(ts) // 2], 2), ms_min=round(ts[0], 2), ms_q1=round(q1, 2),
                              ms_q3=round(q3, 2))), flush=True)
    # the paired difference of consecutive off / on steps (the two alternate): its median and spread
    d = sorted(b - a for a, b in zip(times[None], times['color,translation,cutout']))
    print(json.dumps(dict(what='diffaug_step_difference', ms_median=round(d[len(d) // 2], 3), ms_q1=round(d[len(d) // 4], 3),
                          ms_q3=round(d[(3 * len(d)) // 4], 3), pairs=len(d))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    import torch
    from gan_lab_amd import _lib
    _lib.lib()
    kernels(torch, a.reps)
    if not a.no_step:
        step(torch, a.steps, a.warmup)


if __name__ == '__main__':
    main()
