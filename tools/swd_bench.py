#!/usr/bin/env python3
"""Time one full sliced Wasserstein evaluation (gan_lab_amd/swd.py) stage by stage, next to the same pipeline composed from
torch ops on the same GPU and to the time the generator needs to produce the fake set.

    timeout -k 10 900 python tools/swd_bench.py --res 128 --images 8192 [--batch 64] [--reps 5] [--out profiles/swd_bench.txt]

One process.  Every HIP stage really runs over both complete sets (the printed total is a complete evaluation); per-batch
stages (pyramid, gather) are timed on ``--reps`` batches, HIP and torch interleaved on the same batch, and the median is
scaled to the number of batches; per-level stages (projection, sort, distance) are timed on the full (M, 147) buffers of every
level, HIP and torch interleaved, median over ``--reps`` after one warm-up.  Times are device times (events), in ms.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median_pair(f_hip, f_torch, reps):
    """Interleaved A/B: warm both once, then ``reps`` alternating runs; medians."""
    f_hip(), f_torch()
    th, tt = [], []
    for _ in range(reps):
        th.append(timed(f_hip)[0])
        tt.append(timed(f_torch)[0])
    return statistics.median(th), statistics.median(tt)


# ---- the torch-composed yardstick ----------------------------------------------------------------------------------------
def _kernel(dev, scale):
    f = torch.tensor([1., 4., 6., 4., 1.], device=dev) / 16. * scale
    return (f[:, None] * f[None, :]).expand(3, 1, 5, 5).contiguous()


def torch_pyramid(x, k1, k2):
    gauss = [x]
    while gauss[-1].shape[-1] > 16:
        gauss.append(F.conv2d(F.pad(gauss[-1], (2, 2, 2, 2), mode='reflect'), k1, stride=2, groups=3))
    out = []
    for g0, g1 in zip(gauss[:-1], gauss[1:]):
        z = torch.zeros_like(g0)
        z[:, :, ::2, ::2] = g1
        out.append(g0 - F.conv2d(F.pad(z, (2, 2, 2, 2), mode='reflect'), k2, groups=3))
    return out + [gauss[-1]]


def torch_gather(level, pos):
    n_img, n = pos.shape[:2]
    dev = level.device
    r = torch.arange(-3, 4, device=dev)
    img = torch.arange(n_img, device=dev)[:, None, None, None, None]
    ch = torch.arange(3, device=dev)[None, None, :, None, None]
    yy = pos[:, :, 0].long()[:, :, None, None, None] + r[None, None, None, :, None]
    xx = pos[:, :, 1].long()[:, :, None, None, None] + r[None, None, None, None, :]
    d = level[img, ch, yy, xx].reshape(n_img * n, 147)
    d3 = d.view(-1, 3, 49).double()
    return d, d3.sum(dim=(0, 2)), (d3 * d3).sum(dim=(0, 2))


def torch_project(desc, dirs, stats):
    mean, std = stats[:3].float(), stats[3:].float()
    d = ((desc.view(-1, 3, 49) - mean[None, :, None]) / std[None, :, None]).view(-1, 147)
    return torch.matmul(dirs, d.t())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--images', type=int, default=8192)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-generator', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from gan_lab_amd import ops, swd
    dev = torch.device('cuda')
    res, n_img, bs = a.res, a.images // a.batch * a.batch, a.batch
    n_batches = n_img // bs
    sw = swd.SlicedWasserstein(res, n_img)
    k1, k2 = _kernel(dev, 1.), _kernel(dev, 2.)
    gen = torch.Generator(device='cuda').manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# swd_bench: {res}x{res}, {n_img} + {n_img} images, batch {bs}, {sw.n} neighbourhoods / image, '
        f'{sw.dir_repeats} x {sw.dirs_per_repeat} directions, M = {sw.m} descriptors per set and level')
    # ---- feeds: pyramid + gather, both sets -----------------------------------------------------------------------------
    t_pyr, t_pyr_t, t_gat, t_gat_t, t_feed = [], [], [], [], 0.0
    for which in ('real', 'fake'):
        for b in range(n_batches):
            x = torch.randn(bs, 3, res, res, device=dev, generator=gen)
            x = x + F.avg_pool2d(F.pad(x, (4, 4, 4, 4), mode='reflect'), 9, stride=1) * (3.0 if which == 'real' else 2.0)
            if which == 'real' and 1 <= b <= a.reps:               # batch 0 warms up
                pyr = swd.laplacian_pyramid(x)
                torch_pyramid(x, k1, k2)
                t_pyr.append(timed(lambda: swd.laplacian_pyramid(x))[0])
                t_pyr_t.append(timed(lambda: torch_pyramid(x, k1, k2))[0])
                fed = sw._fed[which]
                pos = [sw.positions(li, fed, bs) for li in range(len(sw.levels))]

                def hip_gather():
                    for li, lv in enumerate(pyr):
                        ops.swd_gather(lv, pos[li], sw._desc[which][li][fed * sw.n:(fed + bs) * sw.n],
                                       sw._part[which][li][fed:fed + bs])

                def torch_gather_all():
                    return [torch_gather(lv, pos[li]) for li, lv in enumerate(pyr)]
                hip_gather(), torch_gather_all()
                t_gat.append(timed(hip_gather)[0])
                t_gat_t.append(timed(torch_gather_all)[0])
                del pyr
            t_feed += timed(lambda: sw._feed(which, x))[0]
    if not t_pyr:
        raise SystemExit('need at least --reps + 1 batches')
    scale = 2 * n_batches
    pyr_h, pyr_t = statistics.median(t_pyr) * scale, statistics.median(t_pyr_t) * scale
    gat_h, gat_t = statistics.median(t_gat) * scale, statistics.median(t_gat_t) * scale
    px = sum(s * s for s in sw.levels)
    # bytes per batch: the pyramid reads every gauss level twice (down, band) and the coarser one once more, writes gauss + bands
    pyr_bytes = scale * bs * 3 * 4 * (px * 4 + (px - res * res) * 1)
    gat_bytes = scale * bs * 4 * (len(sw.levels) * sw.n * 147 * 2)
    # ---- per level: projection, sort, distance --------------------------------------------------------------------------
    t = {k: 0.0 for k in ('proj_h', 'proj_t', 'sort_h', 'sort_t', 'dist_h', 'dist_t')}
    pr, pf, sr, sf = sw._proj
    for li in range(len(sw.levels)):
        stats = {k: ops.swd_stats(sw._part[k][li], sw.n * 49) for k in ('real', 'fake')}
        dirs = sw.directions(0)
        h, tt = median_pair(lambda: (ops.swd_project(sw._desc['real'][li], dirs, stats['real'], out=pr),
                                     ops.swd_project(sw._desc['fake'][li], dirs, stats['fake'], out=pf)),
                            lambda: (torch_project(sw._desc['real'][li], dirs, stats['real']),
                                     torch_project(sw._desc['fake'][li], dirs, stats['fake'])), a.reps)
        t['proj_h'] += h * sw.dir_repeats
        t['proj_t'] += tt * sw.dir_repeats
        h, tt = median_pair(lambda: (ops.swd_sort(pr, out=sr), ops.swd_sort(pf, out=sf)),
                            lambda: (torch.sort(pr, dim=1), torch.sort(pf, dim=1)), a.reps)
        t['sort_h'] += h * sw.dir_repeats
        t['sort_t'] += tt * sw.dir_repeats
        h, tt = median_pair(lambda: ops.swd_distance(sr, sf), lambda: (sr - sf).abs().double().mean(), a.reps)
        t['dist_h'] += h * sw.dir_repeats
        t['dist_t'] += tt * sw.dir_repeats
    t_result, result = timed(sw.result)
    m_bytes = sw.m * 4
    proj_bytes = len(sw.levels) * sw.dir_repeats * 2 * (sw.m * 147 * 4 + sw.dirs_per_repeat * m_bytes)
    sort_bytes = len(sw.levels) * sw.dir_repeats * 2 * sw.dirs_per_repeat * m_bytes * 2
    dist_bytes = len(sw.levels) * sw.dir_repeats * 2 * sw.dirs_per_repeat * m_bytes
    say(f'{"stage":<12}{"HIP ms":>12}{"torch ms":>12}{"torch/HIP":>11}{"min GB moved":>14}{"HIP GB/s":>10}')
    for name, h, tt, nbytes in (('pyramid', pyr_h, pyr_t, pyr_bytes), ('gather', gat_h, gat_t, gat_bytes),
                                ('projection', t['proj_h'], t['proj_t'], proj_bytes), ('sort', t['sort_h'], t['sort_t'], sort_bytes),
                                ('distance', t['dist_h'], t['dist_t'], dist_bytes)):
        say(f'{name:<12}{h:>12.2f}{tt:>12.2f}{tt / h:>11.2f}{nbytes / 1e9:>14.2f}{nbytes / 1e6 / h:>10.0f}')
    say(f'{"sum":<12}{pyr_h + gat_h + t["proj_h"] + t["sort_h"] + t["dist_h"]:>12.2f}'
        f'{pyr_t + gat_t + t["proj_t"] + t["sort_t"] + t["dist_t"]:>12.2f}')
    say(f'measured end to end (HIP): feeds {t_feed:.2f} ms (incl. drawing the centres) + result() {t_result:.2f} ms')
    say(f'result: levels {result["levels"]} swd {[round(v, 3) for v in result["swd"]]} mean {result["mean"]:.3f}')
    # ---- the generator's time for the fake set ----------------------------------------------------------------------------
    if not a.no_generator:
        from gan_lab_amd import progressive as P
        from gan_lab_amd.stylegan.architectures import StyleGenerator
        P.StyleGAN.reset_state()
        g = StyleGenerator(final_res=res, len_latent=512, len_dlatent=512, mapping_num_fcs=8, blur_type='binomial')
        while g.curr_res < res:
            g.increase_scale()
        g.fade_in_phase = False
        g.alpha = 1
        g.cuda().eval()
        gb = min(bs, 16 if res >= 512 else 64)
        z = torch.randn(gb, 512, device=dev)
        with torch.no_grad():
            g(z)
            ts = [timed(lambda: g(z))[0] for _ in range(a.reps)]
        say(f'generator (StyleGAN, full widths, batch {gb}): {statistics.median(ts):.2f} ms / batch -> '
            f'{statistics.median(ts) * n_img / gb:.0f} ms for the {n_img} fake images')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
