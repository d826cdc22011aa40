"""ADA on the MI355X: the forward / adjoint kernels (csrc/ada.hip) at 32 x 3 x 1024^2 for the policies blit, geom and
blit,geom,color with rows drawn at p = 1, beside ``ops.k_diffaug`` with 'color,translation,cutout' and a plain ``clone`` of
the batch in the same process; the filter / noise / cutout kernels (csrc/ada_filter.hip) for filter, filter,noise,cutout and
the six-part policy, beside the ATen composition of the filter on the GPU (``F.pad`` reflect + two grouped ``conv2d``);
and the headline step (StyleGAN 1024^2, batch 32, bench.py's learner) with ``--step-policy`` (default 'blit,geom,color')
against off, alternating the two in one process.  Prints one JSON line per measurement (redirect to
profiles/ada_bench.txt).

    python tools/ada_bench.py [--reps 50] [--steps 20] [--warmup 3] [--p 1.0] [--no-step] [--no-kernels]
                              [--step-policy blit,geom,color,filter,noise,cutout]

``bytes`` is one read and one write of the batch - what the forward needs; the adjoint reads every candidate of its
footprint, so its ``x_clone`` ratio is the price of the gather, not a bandwidth figure."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FULL = 'blit,geom,color'
SIX = 'blit,geom,color,filter,noise,cutout'


def _time_ms(torch, fn, reps):
    for _ in range(3):
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


def kernels(torch, reps, p, n=32, h=1024):
    from gan_lab_amd import ada, augment, ops, rng
    x = torch.rand(n, 3, h, h, device='cuda') * 2 - 1
    g = torch.randn(n, 3, h, h, device='cuda')
    nbytes = 2 * x.numel() * 4
    out = torch.empty_like(x)
    base = {}
    rng.manual_seed(1)
    pd = rng.augment_params(n, h, h)
    dmask = augment.parse_policy('color,translation,cutout')
    for what, fn in (('clone', lambda: out.copy_(x)), ('diffaug_forward', lambda: ops.k_diffaug(x, pd, dmask)),
                     ('diffaug_backward', lambda: ops.k_diffaug(g, pd, dmask, adjoint=True))):
        med, best = _time_ms(torch, fn, reps)
        base[what] = med
        print(json.dumps(dict(what=what, shape=[n, 3, h, h], ms_median=round(med, 4), ms_best=round(best, 4), bytes=nbytes,
                              tb_per_s_median=round(nbytes / (med * 1e-3) / 1e12, 3))), flush=True)
    state = torch.tensor([p, 0, 0, 0], dtype=torch.float32, device='cuda')
    for policy in ('blit', 'geom', FULL):
        rows = rng.ada_params(n, h, h, state, ada.parse_policy(policy))
        G = rows[:, 6:10].abs()
        box = ((2 * (G[:, 0] + G[:, 1])).floor() + 1) * ((2 * (G[:, 2] + G[:, 3])).floor() + 1)
        for direction, fn in (('forward', lambda: ops.k_ada(x, rows)), ('adjoint', lambda: ops.k_ada(g, rows, adjoint=True))):
            med, best = _time_ms(torch, fn, reps)
            ref = base['diffaug_forward' if direction == 'forward' else 'diffaug_backward']
            print(json.dumps(dict(what='ada_kernel', policy=policy, p=p, direction=direction, shape=[n, 3, h, h],
                                  ms_median=round(med, 4), ms_best=round(best, 4), bytes=nbytes,
                                  tb_per_s_median=round(nbytes / (med * 1e-3) / 1e12, 3),
                                  x_clone=round(med / base['clone'], 2), x_diffaug=round(med / ref, 2),
                                  adjoint_candidates_mean=round(box.mean().item(), 1),
                                  adjoint_candidates_max=int(box.max().item()))), flush=True)


def ext_kernels(torch, reps, p, n=32, h=1024):
    """The filter / noise / cutout pass alone (``ops.k_ada_ext``) and the whole of ``ops.ada_augment`` under the six-part policy,
    forward and adjoint, with rows drawn at ``p``; ``aten_filter``: the same taps through F.pad + two grouped conv2d."""
    import torch.nn.functional as F
    from gan_lab_amd import ada, ops, rng
    x = torch.rand(n, 3, h, h, device='cuda') * 2 - 1
    g = torch.randn(n, 3, h, h, device='cuda')
    nbytes = 2 * x.numel() * 4
    out = torch.empty_like(x)
    clone, _ = _time_ms(torch, lambda: out.copy_(x), reps)
    state = torch.tensor([p, 0, 0, 0], dtype=torch.float32, device='cuda')
    rng.manual_seed(1)
    d = None
    for policy in ('filter', 'filter,noise,cutout', SIX):
        d = rng.ada_params(n, h, h, state, ada.parse_policy(policy))
        runs = [('ext_forward', lambda: ops.k_ada_ext(x, d.ext, d.noise)),
                ('ext_adjoint', lambda: ops.k_ada_ext(g, d.ext, adjoint=True))]
        if policy == SIX:
            runs += [('forward', lambda: ops.k_ada_ext(ops.k_ada(x, d.params), d.ext, d.noise)),
                     ('adjoint', lambda: ops.k_ada(ops.k_ada_ext(g, d.ext, adjoint=True), d.params, adjoint=True))]
        for direction, fn in runs:
            med, best = _time_ms(torch, fn, reps)
            print(json.dumps(dict(what='ada_ext_kernel', policy=policy, p=p, direction=direction, shape=[n, 3, h, h],
                                  ms_median=round(med, 4), ms_best=round(best, 4), bytes=nbytes,
                                  tb_per_s_median=round(nbytes / (med * 1e-3) / 1e12, 3), x_clone=round(med / clone, 2))),
                  flush=True)
    taps = (d.ext[:, :4].double() @ ops.ada_filter_bank().cuda()).float().repeat_interleave(3, dim=0)

    def aten():
        xp = F.pad(x, (21, 21, 21, 21), mode='reflect').reshape(1, 3 * n, h + 42, h + 42)
        y = F.conv2d(xp, taps.view(3 * n, 1, 1, 43), groups=3 * n)
        return F.conv2d(y, taps.view(3 * n, 1, 43, 1), groups=3 * n)
    med, best = _time_ms(torch, aten, max(3, reps // 5))
    print(json.dumps(dict(what='aten_filter', shape=[n, 3, h, h], ms_median=round(med, 4), ms_best=round(best, 4),
                          x_clone=round(med / clone, 2))), flush=True)


def step(torch, steps, warmup, res=1024, batch=32, policy=FULL):
    import bench
    learners = {}
    for which in (None, policy):
        learners[which] = bench.build_learner(res, batch, 'cuda', 'f32', 'stylegan', ada=which)
    real = torch.rand(batch, 3, res, res, device='cuda') * 2 - 1
    times = {k: [] for k in learners}
    for it in range(warmup + steps):
        for which, L in learners.items():         # alternate off / on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bench.one_step(L, real)
            torch.cuda.synchronize()
            if it >= warmup:
                times[which].append((time.perf_counter() - t0) * 1e3)
    for which, ts in times.items():
        ts = sorted(ts)
        q1, q3 = ts[len(ts) // 4], ts[(3 * len(ts)) // 4]
        print(json.dumps(dict(what='ada_step', ada=which, res=res, batch=batch, steps=len(ts),
                              ms_median=round(ts[len(ts) // 2], 2), ms_min=round(ts[0], 2), ms_q1=round(q1, 2),
                              ms_q3=round(q3, 2), p=None if which is None else learners[which].ada.p)), flush=True)
    # the paired difference of consecutive off / on steps (the two alternate): its median and spread
    d = sorted(b - a for a, b in zip(times[None], times[policy]))
    print(json.dumps(dict(what='ada_step_difference', ms_median=round(d[len(d) // 2], 3), ms_q1=round(d[len(d) // 4], 3),
                          ms_q3=round(d[(3 * len(d)) // 4], 3), pairs=len(d))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--p', type=float, default=1.0, help='augmentation probability of the drawn rows')
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-kernels', action='store_true')
    ap.add_argument('--step-policy', default=FULL, help='the ADA policy of the step that is compared with ada=None')
    a = ap.parse_args()
    import torch
    from gan_lab_amd import _lib
    _lib.lib()
    if not a.no_kernels:
        kernels(torch, a.reps, a.p)
        ext_kernels(torch, a.reps, a.p)
    if not a.no_step:
        step(torch, a.steps, a.warmup, policy=a.step_policy)


if __name__ == '__main__':
    main()
