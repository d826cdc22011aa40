#!/usr/bin/env python3
"""Time BigGAN's orthogonal regulariser of the ResNet GAN generator (gan_lab_amd/ortho_reg.py, csrc/ortho.hip).

    timeout -k 10 600 python tools/ortho_bench.py [--reps 20] [--iters 5] [--skip-steps] [--out profiles/ortho_bench.json]

On the layer set of the full-width 64-pixel generator (config #5), device time (events), median over ``--reps``:
  (a) the batched ``OrthoReg.apply()`` - 3 launches for all layers;
  (b) the per-layer ATen composition of the same arithmetic in the same form per layer (row form: mm, zero the diagonal, mm,
      add_ ; column form: mm, row norms, mm, addcmul, add_), with the penalty's sum of squares per layer - what the option
      would cost written with torch ops.  It is compared against (a) on the same weights first (max relative difference).
  (c) config #5's generator step (batch 64, ``learner.g_step()``) with ``ortho_reg=1e-4`` against ``ortho_reg=0``: one warm-up
      step, then the median wall time of ``--iters`` steps each."""
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

BETA = 1e-4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def aten_apply(weights, grads, beta):
    """The regulariser with torch ops, layer by layer, in the form the kernels use for the layer.  -> total penalty (device)."""
    total = None
    for w, g in zip(weights, grads):
        r = w.shape[0]
        wm, gm = w.view(r, -1), g.view(r, -1)
        if r == 1:
            continue
        if r <= wm.shape[1]:
            s = wm @ wm.t()
            s.fill_diagonal_(0.)
            gm.add_(s @ wm, alpha=4 * beta)
            pen = (s * s).sum()
        else:
            s = wm.t() @ wm
            q = (wm * wm).sum(dim=1, keepdim=True)
            gm.add_(torch.addcmul(wm @ s, q, wm, value=-1.), alpha=4 * beta)
            pen = (s * s).sum() - (q * q).sum()
        total = pen if total is None else total + pen
    return beta * total


def kernels(reps):
    from gan_lab_amd.optim import ParamArena
    from gan_lab_amd.ortho_reg import OrthoReg
    from gan_lab_amd.resnetgan.architectures import Generator64PixResnet
    torch.manual_seed(0)
    g = Generator64PixResnet().cuda()
    arena = ParamArena(g.named_parameters(), 'cuda')
    reg = OrthoReg(g, arena, BETA)
    weights = [dict(g.named_parameters())[k] for k in reg.names]
    out = {'layers': len(reg.names), 'weights': sum(w.numel() for w in weights), 'shapes': [list(s) for s in reg.shapes],
           'scratch_bytes': 4 * reg.table.scratch.numel(),
           'flops': sum(4.0 * min(r, k) * r * k for r, k in reg.shapes if r > 1)}
    # the two agree
    arena.gflat.zero_()
    reg.apply()
    ours, ours_pen = arena.gflat.clone(), reg.penalty.clone()
    arena.gflat.zero_()
    with torch.no_grad():
        aten_pen = aten_apply([w.data for w in weights], [w.grad for w in weights], BETA)
    out['max_rel_diff_vs_aten'] = float((ours - arena.gflat).abs().max() / arena.gflat.abs().max())
    out['penalty'] = [float(ours_pen), float(aten_pen)]

    def batched():
        reg.apply()

    def aten():
        with torch.no_grad():
            aten_apply([w.data for w in weights], [w.grad for w in weights], BETA)

    for name, fn in (('a_batched_apply', batched), ('b_aten_per_layer', aten)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = statistics.median(timed(fn) for _ in range(reps))
        out[name] = {'ms': round(ms, 4), 'GFLOP_per_s': round(out['flops'] / ms / 1e6, 1)}
    return out


def g_step_ms(iters, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, batch_size=64, res_samples=64, res_dataset=64,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=1234, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    L.set_requires_grad_disc(False)
    times = []
    for i in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.g_step()
        torch.cuda.synchronize()
        if i:
            times.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--skip-steps', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    res = {'kernels_64px_generator': kernels(a.reps)}
    print(json.dumps(res['kernels_64px_generator']), flush=True)
    if not a.skip_steps:
        res['c_config5_g_step_ms'] = {}
        for name, kw in (('ortho_reg=0', {}), ('ortho_reg=1e-4', {'ortho_reg': 1e-4})):
            res['c_config5_g_step_ms'][name] = g_step_ms(a.iters, **kw)
            print(name, res['c_config5_g_step_ms'][name], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
