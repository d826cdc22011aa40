#!/usr/bin/env python3
"""Time the power-spectrum regulariser (``ops.spectrum_loss`` forward + backward; gan_lab_amd/spectrum_reg.py) next
to the same loss composed from ``torch.fft.rfft2`` under autograd on the same GPU, and the generator step of the benchmark's
geometry with and without the term.

    timeout -k 10 900 python tools/spectrum_reg_bench.py [--shapes 32x1024 8x256] [--reps 5] [--step-res 1024] [--step-batch 32]
                                                         [--no-step] [--out profiles/spectrum_reg_bench.json]

One process.  Per shape both paths are warmed once and then timed alternating, median over ``--reps``; times are device times
(events) of one forward + backward.  The torch side is rfft2 of the windowed batch, |F|^2 summed over channels in fp64, one
``index_add_`` into the bins with the half-spectrum weights, the set mean, the logarithms and the band mean, differentiated by
autograd; if it cannot run there (memory, a missing transform) the tool says so and reports only its own time.  The step part
builds bench.py's StyleGAN learner twice, without and with ``spectrum_reg`` (band 'hf'), runs one critic step to give the
regulariser its target and times ``g_step`` alone, median of ``--reps``, synchronised wall time.  Nothing is tuned here and no
speed bar is set: the numbers say what the term costs."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from spectrum_bench import timed, torch_tables  # noqa: E402


def torch_loss(x, target, tables, first):
    """The composed loss of spectrum_bench.torch_profiles' steps, differentiable."""
    w, idx, wt = tables
    res = x.shape[-1]
    f = torch.fft.rfft2((x * w[None, None, None, :]) * w[None, None, :, None])
    p = (f.real * f.real + f.imag * f.imag).double().sum(dim=1).reshape(len(x), -1) * wt
    prof = torch.zeros((len(x), res // 2 + 2), dtype=torch.float64, device=x.device).index_add(1, idx, p)
    s = prof[:, :res // 2 + 1].mean(dim=0) / (3. * res * res * (9. / 64.))
    d = torch.log(s[first:].clamp_min(1e-30)) - torch.log(target[first:].clamp_min(1e-30))
    return (d * d).mean().float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=str, nargs='+', default=['32x1024', '8x256'], help='IMAGESxRES')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step-res', type=int, default=1024)
    ap.add_argument('--step-batch', type=int, default=32)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from gan_lab_amd import ops
    dev = torch.device('cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)
    result = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'band': 'hf', 'window': 'hann', 'ops': [], 'g_step': None}

    print(f'{"shape":<12}{"HIP ms":>10}{"torch ms":>10}{"torch/HIP":>11}{"rel diff L":>12}{"rel L2 dx":>12}', flush=True)
    for shape in a.shapes:
        n, res = (int(v) for v in shape.split('x'))
        x = torch.empty((n, 3, res, res), device=dev).normal_(generator=gen).requires_grad_(True)
        target = ops.spectrum_profile_mean(torch.empty((n, 3, res, res), device=dev).normal_(generator=gen) * 1.5)
        first = res // 4 + 1

        def hip():
            L = ops.spectrum_loss(x, target, 'hf', 'hann')
            return L, torch.autograd.grad(L, x)[0]

        hip()
        row = {'images': n, 'res': res, 'hip_ms': None, 'torch_ms': None, 'note': None}
        try:
            tables = torch_tables(res, dev)

            def composed():
                L = torch_loss(x, target, tables, first)
                return L, torch.autograd.grad(L, x)[0]
            composed()
            th, tt = [], []
            for _ in range(a.reps):
                th.append(timed(hip)[0])
                tt.append(timed(composed)[0])
            (Lh, gh), (Lt, gt) = hip(), composed()
            row.update(hip_ms=statistics.median(th), torch_ms=statistics.median(tt),
                       loss_rel_diff=abs(float(Lh.detach()) - float(Lt.detach())) / abs(float(Lt.detach())),
                       dx_rel_l2=float((gh - gt).norm() / gt.norm()))
            print(f'{shape:<12}{row["hip_ms"]:>10.3f}{row["torch_ms"]:>10.3f}{row["torch_ms"] / row["hip_ms"]:>11.2f}'
                  f'{row["loss_rel_diff"]:>12.2e}{row["dx_rel_l2"]:>12.2e}', flush=True)
        except Exception as exc:      # the composition is the comparison, not the product: report the product alone
            torch.cuda.synchronize()
            row['note'] = f'torch composition did not run: {type(exc).__name__}: {str(exc)[:120]}'
            row['hip_ms'] = statistics.median(timed(hip)[0] for _ in range(a.reps))
            print(f'{shape:<12}{row["hip_ms"]:>10.3f}{"-":>10}{"-":>11}  {row["note"]}', flush=True)
        result['ops'].append(row)
        del x, target

    if not a.no_step:
        import bench
        step = {'res': a.step_res, 'batch': a.step_batch}
        for name, extra in (('off', {}), ('on', {'spectrum_reg': 1.0})):
            torch.cuda.empty_cache()
            L = bench.build_learner(a.step_res, a.step_batch, dev, **extra)
            real = torch.empty((a.step_batch, 3, a.step_res, a.step_res), device=dev).normal_(generator=gen)
            L.set_requires_grad_disc(True)
            L.d_step(real)
            L.set_requires_grad_disc(False)
            L.g_step()
            times = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                L.g_step()
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            step['g_step_ms_' + name] = statistics.median(times)
            del L, real
        step['term_ms'] = step['g_step_ms_on'] - step['g_step_ms_off']
        result['g_step'] = step
        print(f'g_step StyleGAN {a.step_res}^2 batch {a.step_batch}: {step["g_step_ms_off"]:.1f} ms without the term, '
              f'{step["g_step_ms_on"]:.1f} ms with it', flush=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
