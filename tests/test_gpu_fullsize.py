"""Whole-network parity at the BASELINE configurations' FULL channel widths and resolutions:
one D step (adversarial + gradient penalty with its double backward + drift) and one G step of

  * StyleGAN-1024, batch 4 (one minibatch-stddev group), nonsaturating + R1          - BASELINE config #3's network
  * ProGAN-256,   batch 4, WGAN + WGAN-GP (the reference defaults), PixelNorm        - BASELINE config #4's network
  * StyleGAN-128, batch 8, nonsaturating + R1, bf16-compute convolutions             - BASELINE config #2

HIP path vs the CPU oracle (oracle/nets.py, oracle/step.py - pinned against the reference itself by
tests/test_oracle_golden.py) on identical weights, latents, noise and interpolation draws: image, logits, penalty
value, losses and EVERY parameter gradient (gan_lab/progan/learner.py:734-943, gan_lab/resnetgan/learner.py:780-827).

Rule for the gradients (fp32 networks): an entry passes at 1e-3 relative (max-abs over the tensor, scaled by the
tensor's own max or 1e-3 of the network's largest gradient, whichever is larger).  Entries the fp32 CPU oracle and
the HIP path disagree on by more than that sit behind ~40 layers with normalisation gains in between, where two
correct fp32 implementations differ by rounding alone; those are judged against the SAME oracle evaluated in
float64: the HIP result must be as close to the exact answer as the CPU fp32 path is, ENTRY BY ENTRY (no extra noise
factor, nothing borrowed from another layer: ``e_hip <= max(1e-3, 1.5 * e_cpu)``; round 2 also admitted the worst CPU
entry of the whole network - the bias / noise-weight / InstanceNorm-backward sums now keep fp64 partials instead).  One documented fp32 effect is recognised by its signature
and reported rather than failed: a LeakyReLU mask bit that flips on an activation within one rounding of zero
(``_without_tie_channels``) - the excess error must then sit in at most two output channels of that one layer's
weight / bias gradient, with every other channel inside the bar.
What the float64 comparison can and cannot show at 1024^2: the ~60 generator gradients behind the whole of D carry ONE
realisation of the rounding noise amplified on the way (the same relative error on all of them - for the CPU fp32 path
exactly as for the HIP path), so "as close to float64 as the CPU path" compares two random magnitudes on a single draw.
Measured while changing an unrelated kernel in round 2: rounding the mapping network's normalised latents in a
different (more accurate) order moved the median HIP error of those entries from 1.2e-3 to 2.9e-3 against 1.0e-3 for
the CPU path, and one entry across the bar.  tests/test_gpu_nets.py::test_thin16_network_is_as_accurate_as_the_cpu_path
therefore asserts the property statistically (three draws) on a network small enough for it; here the draw is fixed by
the seeds and the kernels are deterministic, so the outcome is reproducible, but a change of summation order anywhere
upstream is a new draw.
The oracle costs minutes of host time per case (the CPU box of the GPU node has the cores for it)."""
import time

import numpy as np
import pytest
import torch

from util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(autouse=True)
def _full_widths():
    from gan_lab_amd import ops, progressive as P
    old = (P.FMAP_BASE, P.FMAP_MAX)
    P.FMAP_BASE, P.FMAP_MAX = 8192, 512
    yield
    P.FMAP_BASE, P.FMAP_MAX = old
    ops.set_compute_dtype('f32')


def _build(kind, res, seed=11, **gen_kwargs):
    from gan_lab_amd import progressive as P
    from gan_lab_amd.progan.architectures import ProDiscriminator, ProGenerator, StyleDiscriminator
    from gan_lab_amd.stylegan.architectures import StyleGenerator
    torch.manual_seed(seed)
    if kind == 'stylegan':
        P.StyleGAN.reset_state()
        g, d = StyleGenerator(final_res=res, blur_type='binomial', **gen_kwargs), StyleDiscriminator(final_res=res,
                                                                                                     blur_type='binomial')
    else:
        P.ProGAN.reset_state()
        g, d = ProGenerator(final_res=res, blur_type='binomial'), ProDiscriminator(final_res=res,
                                                                                   blur_type='binomial')
    for _ in range(int(np.log2(res)) - 2):
        g.increase_scale()
        d.increase_scale()
    g.fade_in_phase = False
    g.alpha = 1
    with torch.no_grad():       # the reference initialises biases / noise weights to zero: make them count
        for k, p in list(g.named_parameters()) + list(d.named_parameters()):
            if k.endswith('bias') or k.endswith('noise_weight'):
                p.normal_(0, 0.3)
            elif k == 'const_input':
                p.normal_(1.0, 0.5)
    sd_g = {k: v.clone() for k, v in g.state_dict().items()}
    sd_d = {k: v.clone() for k, v in d.state_dict().items()}
    return g, d, sd_g, sd_d


def _hip_step(kind, g, d, z, real, noise, loss, gp, eps_interp, dtype):
    """progan/learner.py:734-816 + :857-904 on the product modules (the D(real) forward shared with R1 exactly as
    ProGANLearner.d_step does)."""
    from gan_lab_amd import ops
    from gan_lab_amd.utils import backprop_utils as bp
    g.cuda().eval()
    if kind == 'stylegan':
        g.use_truncation_trick = False
    d.cuda().train()
    gk = dict(noise=[n.cuda() for n in noise]) if kind == 'stylegan' else {}
    with ops.compute_dtype(dtype):
        img = g(z.cuda(), **gk)
        fake = img.detach()
        if gp == 'r1':
            xr = real.cuda().requires_grad_(True)
            d_real, d_fake = d(xr), d(fake)
            gpv = bp.gp_from_output(d_real, xr, 'r1', 10.)
        else:
            d_fake, d_real = d(fake), d(real.cuda())
            gpv = bp.calc_gp(d, gp, fake, real.cuda(), lda=10., gamma=1., eps_interp=eps_interp.cuda())
        loss_d = bp.loss_disc(loss, d_fake, d_real) + gpv + bp.drift_loss(d_real, 0.001)
        loss_d.backward()
        for p in d.parameters():
            p.requires_grad_(False)
        loss_g = bp.loss_gen(loss, d(img))
        loss_g.backward()
    torch.cuda.synchronize()
    return dict(img=img.detach().cpu(), d_real=d_real.detach().cpu(), d_fake=d_fake.detach().cpu(),
                gp=gpv.detach().cpu(), loss_d=loss_d.detach().cpu(), loss_g=loss_g.detach().cpu(),
                gd={k: p.grad.detach().cpu() for k, p in d.named_parameters() if p.grad is not None},
                gg={k: p.grad.detach().cpu() for k, p in g.named_parameters() if p.grad is not None})


def _oracle_step(kind, sd_g, sd_d, z, real, noise, loss, gp, eps_interp, dt=torch.float32, want=('d', 'g'), **cfg_kwargs):
    from oracle import nets, ops as O, step
    cfg = nets.make_cfg(use_pixelnorm=(kind == 'progan'), **cfg_kwargs)
    og = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd_g.items()}
    od = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd_d.items()}
    z, real = z.to(dt), real.to(dt)
    if kind == 'stylegan':
        oimg = nets.stylegen_forward(og, z, [n.to(dt) for n in noise], cfg)
    else:
        oimg = nets.progen_forward(og, z, cfg)
    out = dict(img=oimg.detach())
    if 'd' in want:
        total, parts = step.d_loss(od, cfg, oimg.detach(), real, loss, gp, 10.0, 1.0, 0.001,
                                   eps_interp=None if eps_interp is None else eps_interp.to(dt).view(-1, 1, 1, 1),
                                   return_parts=True)
        total.backward()
        out.update(loss_d=total.detach(), gp=parts['gp'].detach(), d_real=parts['d_real'].detach(),
                   d_fake=parts['d_fake'].detach(),
                   gd={k: v.grad.detach().clone() for k, v in od.items() if v.grad is not None})
    if 'g' in want:
        olg = O.loss_gen(loss, nets.disc_forward({k: v.detach() for k, v in od.items()}, oimg, cfg))
        olg.backward()
        out.update(loss_g=olg.detach(), gg={k: v.grad.detach().clone() for k, v in og.items() if v.grad is not None})
    return out


def _grad_errors(hip, ref, floor_frac=1e-3):
    gmax = max(v.abs().max().item() for v in ref.values())
    out = {}
    for k, r in ref.items():
        if r.abs().max() == 0:
            continue
        scale = max(r.abs().max().item(), floor_frac * gmax)
        out[k] = ((hip[k].double() - r.double()).abs().max() / scale).item()
    return out, gmax


MAX_TIE_CHANNELS = 2


def _without_tie_channels(k, hip, ex, scale):
    """LeakyReLU ties.  ``gz = gy * lrelu'(y)`` takes its mask from the sign of a pre-activation; an element within one
    fp32 rounding of zero gets a different mask bit in two correct fp32 implementations (and in float64).  One flipped
    bit changes gz by 0.8*gy at ONE (sample, channel, pixel): invisible upstream (one of ~10^6 terms of the next
    contraction) but O(1e-2) of THAT output channel's bias gradient and weight-gradient rows, which are sums over only
    B*H*W terms.  Signature: the whole excess error of a conv weight / bias gradient sits in one or two output
    channels.  Returns (error with the worst <= MAX_TIE_CHANNELS output channels left out, those channels)."""
    e = (hip.double() - ex).abs()
    if k.endswith('bias') or k.endswith('noise_weight'):     # one value per output channel of the layer
        per = e.flatten()
    elif k.endswith('conv2d.weight') or k.endswith('linear.weight'):
        per = e.flatten(1).max(dim=1).values
    else:
        return None, []
    if per.numel() < 16:
        return None, []
    # How many flips to expect: two correct fp32 evaluations of a pre-activation differ by ~2e-7 of its scale (tools/
    # flip_probe.py: 2.2e-7 .. 3.4e-7 on both paths), so ~1.6e-7 of a layer's activations sit on the other side of zero - one
    # flip per ~6 M activations, on the CPU fp32 path as on this one (the probe counts 1 - 3 flipped bits per pass through
    # the full-width 128^2 critic on either).  A layer's B * C * H * W activations spread their flips over C channels: up
    # to MAX_TIE_CHANNELS channels per tensor, one more per 128 channels beyond 256 (a 512-channel layer: 4), ONE for a
    # 16-channel layer.
    limit = max(MAX_TIE_CHANNELS, per.numel() // 128) if per.numel() > 16 else 1
    order = per.argsort(descending=True)
    drop = [int(i) for i in order[:limit] if per[i] / scale > TOL]
    keep = torch.ones_like(per, dtype=torch.bool)
    keep[drop] = False
    return (per[keep].max() / scale).item(), drop


def _judge_outliers(tag, bad, hip, cpu, exact, gmax64):
    still, judged, ties = {}, {}, {}
    for k in bad:
        ex = exact[k]
        scale = max(ex.abs().max().item(), 1e-3 * gmax64)
        e_hip = (hip[k].double() - ex).abs().max().item() / scale
        e_cpu = (cpu[k].double() - ex).abs().max().item() / scale
        judged[k] = (e_hip, e_cpu)
    for k, (e_hip, e_cpu) in judged.items():
        bar = max(TOL, 1.5 * e_cpu)        # per entry: no allowance borrowed from another layer's CPU error
        if e_hip > bar:
            scale = max(exact[k].abs().max().item(), 1e-3 * gmax64)
            e_rest, dropped = _without_tie_channels(k, hip[k], exact[k], scale)
            if e_rest is not None and dropped and e_rest <= bar:
                ties[tag + k] = dict(channels=dropped, err_all='%.2e' % e_hip, err_other_channels='%.2e' % e_rest)
            else:
                d = (hip[k].double() - exact[k]).abs()
                per = d.flatten() if d.dim() <= 1 or k.endswith('bias') or k.endswith('noise_weight') else \
                    d.flatten(1).max(dim=1).values
                top = per.flatten().topk(min(3, per.numel()))
                still[tag + k] = (e_hip, e_cpu, 'worst channels (error / scale): ' + ', '.join(
                    '%d: %.1e' % (int(i), float(v) / scale) for v, i in zip(top.values, top.indices)))
    return still, judged, ties


def _assert_ties_are_rare(rep, n_entries):
    """The LeakyReLU tie exemption is a REPORT of flipped mask bits, not a waiver: it may only concern a small part of
    the network.  How often a flip must be expected: two fp32 implementations (and float64) disagree on a pre-activation
    by ~1e-6 of its scale, so about 1e-6 of a layer's activations sit on the other side of zero - 4 x 128 x 128^2 = 8.4 M
    activations at a 128^2 generator layer: a handful of flips per layer and step, each moving ONE channel's bias /
    noise-weight sum (65 k terms of random sign) by ~0.8 / sqrt(65 k) = 3e-3 of its size.  Mid-resolution layers
    therefore show one or two such channels on most draws (on the CPU fp32 path as well, in other channels); what must
    not happen is the exemption carrying a sizeable share of the entries."""
    ties = rep.get('lrelu_tie_channels', {})
    assert len(ties) <= max(2, n_entries // 12), (len(ties), n_entries, ties)


CASES = [('progan', 256, 4, 'wgan', 'wgan-gp')]


@pytest.mark.parametrize('kind,res,b,loss,gp', CASES, ids=['progan256-b4-wgangp'])
def test_full_width_step_vs_oracle(kind, res, b, loss, gp, capsys):
    g, d, sd_g, sd_d = _build(kind, res)
    gen = torch.Generator().manual_seed(2024)
    z = torch.randn(b, 512, generator=gen)
    real = torch.rand(b, 3, res, res, generator=gen) * 2 - 1
    noise = [torch.randn(b, 1, 4 * 2 ** (n // 2), 4 * 2 ** (n // 2), generator=gen)
             for n in range(len(g.gen_layers))] if kind == 'stylegan' else None
    eps_interp = torch.rand(b, generator=gen) if gp == 'wgan-gp' else None
    t0 = time.time()
    hip = _hip_step(kind, g, d, z, real, noise, loss, gp, eps_interp, 'f32')
    t1 = time.time()
    cpu = _oracle_step(kind, sd_g, sd_d, z, real, noise, loss, gp, eps_interp)
    t2 = time.time()
    rep = {k: rel_err(hip[k], cpu[k]) for k in ('img', 'd_real', 'd_fake', 'gp', 'loss_d', 'loss_g')}
    ed, gmax_d = _grad_errors(hip['gd'], cpu['gd'])
    eg, gmax_g = _grad_errors(hip['gg'], cpu['gg'])
    rep['worst_d_grad'] = max(ed.items(), key=lambda kv: kv[1])
    rep['worst_g_grad'] = max(eg.items(), key=lambda kv: kv[1])
    bad_d = [k for k, v in ed.items() if v > TOL]
    bad_g = [k for k, v in eg.items() if v > TOL]
    still = {}
    if bad_d or bad_g:
        want = (('d',) if bad_d else ()) + (('g',) if bad_g else ())
        ex = _oracle_step(kind, sd_g, sd_d, z, real, noise, loss, gp, eps_interp, dt=torch.float64, want=want)
        if bad_d:
            s, j, ties = _judge_outliers('d.', bad_d, hip['gd'], cpu['gd'], ex['gd'],
                                         max(v.abs().max().item() for v in ex['gd'].values()))
            still.update(s)
            rep.setdefault('lrelu_tie_channels', {}).update(ties)
            rep['judged_d'] = {k: ('%.2e' % a, '%.2e' % c) for k, (a, c) in j.items()}
        if bad_g:
            s, j, ties = _judge_outliers('g.', bad_g, hip['gg'], cpu['gg'], ex['gg'],
                                         max(v.abs().max().item() for v in ex['gg'].values()))
            still.update(s)
            rep.setdefault('lrelu_tie_channels', {}).update(ties)
            rep['judged_g'] = {k: ('%.2e' % a, '%.2e' % c) for k, (a, c) in j.items()}
    t3 = time.time()
    rep['seconds'] = dict(hip=round(t1 - t0, 1), oracle_f32=round(t2 - t1, 1), oracle_f64=round(t3 - t2, 1))
    rep['n_entries'] = (len(ed), len(eg))
    with capsys.disabled():
        print(f'\n{kind}-{res} b{b} {loss}+{gp} full width, HIP vs oracle:', rep)
        print('SUMMARY %s-%d-b%d %s+%s: img %.1e d_real %.1e gp %.1e loss_d %.1e loss_g %.1e | worst d %.1e g %.1e (vs fp32 oracle) | '
              'entries > 1e-3: d %d g %d, beyond strict rule %d | ties %d' % (
                  kind, res, b, loss, gp, rep['img'], rep['d_real'], rep['gp'], rep['loss_d'], rep['loss_g'], rep['worst_d_grad'][1],
                  rep['worst_g_grad'][1], sum(v > 1e-3 for v in ed.values()), sum(v > 1e-3 for v in eg.values()), len(still),
                  len(rep.get('lrelu_tie_channels', {}))))
    for k in ('img', 'd_real', 'd_fake', 'gp', 'loss_d', 'loss_g'):
        assert rep[k] <= TOL, (k, rep)
    assert not still, still
    assert len(ed) >= 20 and len(eg) >= 20
    _assert_ties_are_rare(rep, len(ed) + len(eg))


def test_stylegan128_bf16_b8_step_vs_oracle(capsys):
    """BASELINE config #2 at its own size: StyleGAN-128 full width, batch 8, bf16-compute convolutions, against the
    fp32 oracle.  bf16 products (8 mantissa bits, fp32 accumulation) are an extension the reference does not have, so
    the bar is the documented bf16 one (tests/test_gpu_bf16.py): image / losses / R1 within 2e-2, every significant
    parameter gradient with cosine > 0.98 to the fp32 oracle's."""
    kind, res, b = 'stylegan', 128, 8
    g, d, sd_g, sd_d = _build(kind, res)
    gen = torch.Generator().manual_seed(77)
    z = torch.randn(b, 512, generator=gen)
    real = torch.rand(b, 3, res, res, generator=gen) * 2 - 1
    noise = [torch.randn(b, 1, 4 * 2 ** (n // 2), 4 * 2 ** (n // 2), generator=gen) for n in range(len(g.gen_layers))]
    hip = _hip_step(kind, g, d, z, real, noise, 'nonsaturating', 'r1', None, 'bf16')
    cpu = _oracle_step(kind, sd_g, sd_d, z, real, noise, 'nonsaturating', 'r1', None)
    rep = {k: rel_err(hip[k], cpu[k]) for k in ('img', 'd_real', 'd_fake', 'gp', 'loss_d', 'loss_g')}

    def cos(a, r):
        a, r = a.double().flatten(), r.double().flatten()
        return (a @ r / (a.norm() * r.norm()).clamp_min(1e-300)).item()
    worst = (1.0, None)
    for tag, hg, cg in (('d.', hip['gd'], cpu['gd']), ('g.', hip['gg'], cpu['gg'])):
        gmax = max(v.abs().max().item() for v in cg.values())
        for k, r in cg.items():
            if r.abs().max() < 1e-3 * gmax:          # numerically-zero gradients (a bias in front of an InstanceNorm)
                continue
            c = cos(hg[k], r)
            if c < worst[0]:
                worst = (c, tag + k)
    rep['worst_grad_cosine'] = worst
    with capsys.disabled():
        print('\nbf16 StyleGAN-128 b8 step vs fp32 oracle:', rep)
        print('SUMMARY bf16 stylegan-128-b8 (own bar 2e-2 / cosine 0.98): img %.1e gp %.1e loss_d %.1e loss_g %.1e | worst gradient '
              'cosine %.4f (%s)' % (rep['img'], rep['gp'], rep['loss_d'], rep['loss_g'], worst[0], worst[1]))
    assert rep['img'] < 2e-2 and rep['loss_d'] < 1e-2 and rep['loss_g'] < 1e-2 and rep['gp'] < 2e-2, rep
    assert worst[0] > 0.98, rep


# ---------------------------------------------------------------------------------------------------------------
# the code path bench.py times: the LEARNER's d_step / g_step at the headline geometry, full width
# ---------------------------------------------------------------------------------------------------------------
def _host_cpus():
    """CPUs this process may actually use: the affinity mask, capped by the cgroup's CPU quota."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 2)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


class _KernelCensus(object):
    """Counts the kernel symbols dispatched through the C ABI while active: every entry point of the loaded library is
    wrapped so that the launches the call made (``ganlab_launch_count`` / ``ganlab_launch_history``: per calling thread -
    the autograd engine launches the backward from its own thread; an entry point may launch several kernels) are read
    right after it."""

    def __enter__(self):
        from gan_lab_amd import _lib
        self.L, self.saved, self.seen = _lib.lib(), {}, {}
        self.saved_count = self.L.ganlab_launch_count
        for name in _lib.SIGNATURES:
            if name in ('ganlab_last_launch', 'ganlab_launch_count', 'ganlab_launch_history') or name.endswith('_size') or name.endswith('_workspace') or \
                    name.endswith('_supported') or name.endswith('_plan') or name.endswith('_slots'):
                continue
            fn = getattr(self.L, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _lib=_lib):
                before = int(self.saved_count())
                rc = _fn(*a)
                for sym, _ in _lib.launches_since(before):
                    self.seen[sym] = self.seen.get(sym, 0) + 1
                return rc
            setattr(self.L, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.L, name, fn)
        return False

    def count(self, *needles):
        return sum(n for sym, n in self.seen.items() if all(s in sym for s in needles))


LEARNER_CASES = [(1024, 8)]


@pytest.mark.parametrize('res,b', LEARNER_CASES, ids=[f'stylegan{r}-b{b}-learner' for r, b in LEARNER_CASES])
def test_learner_step_full_width_vs_oracle(res, b, capsys, tmp_path):
    """``ProGANLearner.d_step(defer_update=True)`` + ``g_step(d_update_pending=True)`` - flat arenas, FusedAdam,
    ``no_grad_towards``, ``direct_param_grads``, the shared D(real) forward, the deferred D update, train-mode generator
    with mixing regularisation and injected noise, EWMA - on the full-width StyleGAN-1024 (BASELINE config #3's network,
    TWO minibatch-stddev groups), fp32, against ``oracle/step.py FunctionalGAN`` (gan_lab/progan/learner.py:734-943,
    gan_lab/resnetgan/learner.py:780-827) driven with the same latents, noise (``honour_noise_in_training``), mixing cut and
    real batch: losses, logits, R1 value, every gradient in both arenas (per-entry float64 rule of this file), the Adam
    update of every parameter and the EWMA shadow.

    This is the code ``bench.py`` times.  The round-3 fused kernels only dispatch at these sizes - the blur-folded
    rolling-window kernels (<= 16 channels, W % 64 == 0), fromRGB's backward inside the first conv's input gradient
    (``RB_RGB``, only inside ``direct_param_grads``), the thin modulated layer - and had fused == composed evidence only
    (VERDICT r03 weak 2): the census below asserts that each of them actually ran in this step.
    The two oracle evaluations (fp32, float64) run in processes of their own next to the GPU's part
    (tests/oracle_worker.py)."""
    import os
    import subprocess
    import sys
    from gan_lab_amd import ops
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.architectures import StyleAddNoise
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    b = int(os.environ.get('GANLAB_TEST_LEARNER_BATCH', b))
    lr = 1e-3
    torch.manual_seed(31)
    cfg = make_config('stylegan', dev='cuda', pin_memory=False, res_samples=res, res_dataset=res, init_res=res,
                      batch_size=b, bs_dict={r: b for r in (4, 8, 16, 32, 64, 128, 256, 512, 1024)},
                      loss='nonsaturating', gradient_penalty='r1', lda=10., num_iters_save_model=10 ** 9, log_every=0,
                      random_seed=5, cutoff_trunc_trick=4, lr_base=lr)
    L = StyleGANLearner(cfg)
    with torch.no_grad():
        for k, p in list(L.gen_model.named_parameters()) + list(L.disc_model.named_parameters()):
            if k.endswith('bias') or k.endswith('noise_weight'):
                p.normal_(0, 0.3)
            elif k == 'const_input':
                p.normal_(1.0, 0.5)
    L.ewma.flat.copy_(L.arena_g.flat)
    L.beta = L.get_smoothing_ewma_beta(half_life=10.)
    L.gen_model.train()
    L.disc_model.train()
    assert L.arena_g.is_attached() and L.arena_d.is_attached()
    sd_g = {k: v.detach().cpu().clone() for k, v in L.gen_model.state_dict().items()}
    sd_d = {k: v.detach().cpu().clone() for k, v in L.disc_model.state_dict().items()}
    gen = torch.Generator().manual_seed(99)
    nl = len(L.gen_model.gen_layers)
    shapes = [(b, 1, 4 * 2 ** (n // 2), 4 * 2 ** (n // 2)) for n in range(nl)]
    zd, zg = torch.randn(b, 512, generator=gen), torch.randn(b, 512, generator=gen)
    zmix_d, zmix_g = torch.randn(b, 512, generator=gen), torch.randn(b, 512, generator=gen)
    nd = [torch.randn(*s, generator=gen) for s in shapes]
    ng = [torch.randn(*s, generator=gen) for s in shapes]
    real = torch.rand(b, 3, res, res, generator=gen) * 2 - 1
    cut_d, cut_g = 5, nl - 3
    lr_factor = cfg.lr_fctr_dict[res]            # LambdaLR 'resolution dependent' (StyleGAN: 3 at 1024)
    for grp in L.opt_gen.param_groups + L.opt_disc.param_groups:
        grp['lr'] = lr * lr_factor

    # ---- the oracle, fp32 and float64, side by side in two processes ------------------------------------------------
    t0 = time.time()
    torch.save(dict(sd_g=sd_g, sd_d=sd_d, zd=zd, zg=zg, zmix_d=zmix_d, zmix_g=zmix_g, nd=nd, ng=ng, real=real,
                    cut_d=cut_d, cut_g=cut_g, lr=lr, lr_factor=lr_factor, beta=L.beta, loss='nonsaturating', gp='r1',
                    lda=10., eps_drift=.001), tmp_path / 'in.pt')
    # (float64 takes ~3.5x the time of fp32 on the same threads: it gets three quarters of the host's CPU quota)
    ncpu = _host_cpus()
    threads = {'float32': max(1, ncpu // 4), 'float64': max(1, ncpu - max(1, ncpu // 4))}
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'oracle_worker.py')
    procs = {dt: subprocess.Popen([sys.executable, worker, str(tmp_path / 'in.pt'), str(tmp_path / f'{dt}.pt'), dt,
                                   str(threads[dt])]) for dt in ('float32', 'float64')}
    try:
        # ---- the learner's own step ---------------------------------------------------------------------------------
        StyleAddNoise.honour_noise_in_training = True
        taken = [0]
        before = ops.arena_takes()
        try:
            with _KernelCensus() as census:
                L.set_requires_grad_disc(True)
                ld = L.d_step(real.cuda(), zb=zd.cuda(), defer_update=True,
                              gen_kwargs=dict(noise=[n.cuda() for n in nd], _mix=(cut_d, zmix_d.cuda())))
                gd = {k: v.detach().cpu().clone() for k, v in L.arena_d.views_of(L.arena_d.gflat).items()}
                L.set_requires_grad_disc(False)
                lg = L.g_step(zb=zg.cuda(), d_update_pending=True,
                              gen_kwargs=dict(noise=[n.cuda() for n in ng], _mix=(cut_g, zmix_g.cuda())))
                gg = {k: v.detach().cpu().clone() for k, v in L.arena_g.views_of(L.arena_g.gflat).items()}
        finally:
            StyleAddNoise.honour_noise_in_training = False
            taken[0] = ops.arena_takes() - before
        torch.cuda.synchronize()
        t1 = time.time()
        new_g = {k: v.detach().cpu() for k, v in L.gen_model.state_dict().items()}
        new_d = {k: v.detach().cpu() for k, v in L.disc_model.state_dict().items()}
        lag = {k: v.detach().cpu() for k, v in L.lagged_params.items()}
        ld, lg = ld.cpu(), lg.cpu()
        n_params = len(L.arena_d.params) + len(L.arena_g.params)
        del L
        torch.cuda.empty_cache()
        for dt, p in procs.items():
            assert p.wait() == 0, f'the {dt} oracle process failed'
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    cpu, ex = torch.load(tmp_path / 'float32.pt'), torch.load(tmp_path / 'float64.pt')
    t2 = time.time()

    # ---- which kernels ran (the dispatch the bench times) ---------------------------------------------------------------
    must = {'fromRGB backward inside the first conv input gradient (RB_RGB)': ('conv_fwd_roll_blur_kernel<2',),
            'conv + LeakyReLU + blur (critic top, forward)': ('conv_fwd_roll_blur_kernel<1',),
            'upsample + conv + blur + layer tail (generator top, forward)': ('conv_s2_up_roll_blur_kernel<0',),
            'pooled conv input gradient + blur^T + LeakyReLU derivative (critic top, backward)':
                ('conv_s2_up_roll_blur_kernel<1',),
            'thin modulated layer with its tail (generator top)': ('conv_fwd_rollmod_kernel',),
            'rolling-window weight gradient': ('conv_wgrad_roll_kernel',),
            'rolling-window stride-2 weight gradient': ('conv_s2_wgrad_roll2_kernel',),
            # the split-product (3 x bf16) families: x3_ok and its kin route to the exact kernels below their tile gates
            'split-product conv: forward / input gradient (thick plain layers)': ('conv_x3_fwd_kernel',),
            'split-product conv: up-layer forward / pooled-layer input gradient': ('conv_x3_up_kernel',),
            'split-product conv: pooled-layer forward / up-layer input gradient': ('conv_x3_down_kernel',),
            'split-product weight gradient': ('x3w_reduce_kernel',),
            'split-product stride-2 weight gradient': ('x3sw_reduce_kernel',)}
    ran = {what: census.count(*needles) for what, needles in must.items()}
    rep = dict(loss_d=rel_err(ld, cpu['ld']), loss_g=rel_err(lg, cpu['lg']), kernels=ran,
               direct_gradients=f'{taken[0]} of {n_params} parameters')
    ed, _ = _grad_errors(gd, cpu['gd'])
    eg, _ = _grad_errors(gg, cpu['gg'])
    rep['worst_d_grad'] = max(ed.items(), key=lambda kv: kv[1])
    rep['worst_g_grad'] = max(eg.items(), key=lambda kv: kv[1])
    bad_d, bad_g = [k for k, v in ed.items() if v > TOL], [k for k, v in eg.items() if v > TOL]
    still = {}
    if bad_d:        # the critic's own gradients: the strict per-entry rule of this file
        s_, j, ties = _judge_outliers('d.', bad_d, gd, cpu['gd'], ex['gd'],
                                      max(v.abs().max().item() for v in ex['gd'].values()))
        still.update(s_)
        rep.setdefault('lrelu_tie_channels', {}).update(ties)
        rep['judged_d'] = {k: ('%.2e' % a, '%.2e' % c) for k, (a, c) in j.items()}
    if bad_g:
        # Every generator gradient of the G step is J_G^T applied to ONE vector, the critic's input gradient
        # d loss / d image: all ~80 generator entries inherit ONE realisation of its rounding error, on the CPU fp32 path
        # exactly as on the HIP path.  Judged per entry like the critic's: e_hip <= max(TOL, 1.5 e_cpu), both against
        # float64 (the set rule of rounds 3 / 4 - median ratio and worst entry as a fallback - is gone: no entry needs it);
        # the common-mode numbers are reported only.
        s_, j, ties = _judge_outliers('g.', bad_g, gg, cpu['gg'], ex['gg'],
                                      max(v.abs().max().item() for v in ex['gg'].values()))
        still.update(s_)
        rep.setdefault('lrelu_tie_channels', {}).update(ties)
        rep['judged_g'] = {k: ('%.2e' % a, '%.2e' % c) for k, (a, c) in j.items()}
        ratios = sorted(a / max(c, 1e-30) for a, c in j.values())
        rep['g_common_mode'] = dict(median_ratio=round(ratios[len(ratios) // 2], 2), worst_e_hip='%.2e' % max(
            a for a, _ in j.values()), entries_beyond_strict_rule=len(s_), entries=len(j))
    # Adam (beta1 = 0, first step): every element moves by lr * g / (|g| + eps).  Two checks.  (i) The optimiser's own
    # arithmetic: the update the fused kernel made against that formula evaluated in float64 on the gradient IT was given
    # (the arena's) - every element of every parameter, to 1e-3 of the step size plus the parameter's own fp32 spacing.
    # (ii) Against the oracle's update where the gradient's sign and size are certain on both paths - elements above 1e-3
    # of the tensor's largest, above 8x the largest difference between the two fp32 paths on that tensor and above 100 eps
    # (below that the step is not saturated at lr and follows the gradient's rounding) - to 2 % of the step size;
    # prev_torgb / prev_fromrgb are outside the optimiser in the stabilised phase and must not move.
    n_upd, worst_upd, worst_arith = 0, (0.0, None), (0.0, None)
    for tag, new, old, ref, grads, mine in (('g.', new_g, sd_g, cpu['g'], cpu['gg'], gg),
                                            ('d.', new_d, sd_d, cpu['d'], cpu['gd'], gd)):
        for k, v0 in old.items():
            du, du_ref = new[k] - v0, ref[k] - v0
            if du_ref.abs().max() == 0:
                assert du.abs().max() == 0, tag + k
                continue
            gm = mine[k].double()
            want = -(lr * lr_factor) * gm / (gm.abs() + 1e-8)
            # (allowance: 1e-3 of the step + the parameter's own fp32 spacing - the mapping network's weights are ~100)
            allow = 1e-3 * (lr * lr_factor) + 2.4e-7 * v0.double().abs()
            ea = ((du.double() - want).abs() / allow).max().item()
            if ea > worst_arith[0]:
                worst_arith = (ea, tag + k)
            g = grads[k]
            m = g.abs() > max(1e-3 * g.abs().max().item(), 8.0 * (mine[k] - g).abs().max().item(), 1e-6)
            if not bool(m.any()):
                continue
            e = ((du - du_ref)[m].abs().max() / du_ref[m].abs().max()).item()
            n_upd += int(m.sum())
            if e > worst_upd[0]:
                worst_upd = (e, tag + k)
    rep['worst_update_arithmetic'] = worst_arith
    rep['worst_update'] = worst_upd
    worst_lag = max(((lag[k] - cpu['lag'][k]).abs().max().item() / max(cpu['lag'][k].abs().max().item(), 1e-30), k)
                    for k in lag)
    rep['worst_ewma'] = worst_lag
    rep['seconds'] = dict(hip=round(t1 - t0, 1), waited_for_oracle=round(t2 - t1, 1), oracle_f32=round(cpu['seconds'], 1),
                          oracle_f64=round(ex['seconds'], 1), threads=threads)
    with capsys.disabled():
        print(f'\nlearner d_step + g_step, StyleGAN-{res} b{b} full width, vs FunctionalGAN:', rep)
        cm = rep.get('g_common_mode', {})
        # one line the driver's tail keeps (<= 400 bytes)
        print(('SUMMARY learner-%d-b%d: loss_d %.1e loss_g %.1e | worst d %.1e g %.1e (vs fp32 oracle) | entries > 1e-3: d %d g %d, '
               'beyond strict rule %d | g median e_hip/e_cpu %s worst e_hip %s | ties %d | census %s | adam %.2f ewma %.0e')
              % (res, b, rep['loss_d'], rep['loss_g'], rep['worst_d_grad'][1], rep['worst_g_grad'][1],
                 sum(v > 1e-3 for v in ed.values()), sum(v > 1e-3 for v in eg.values()), len(still),
                 cm.get('median_ratio', '-'), cm.get('worst_e_hip', '-'), len(rep.get('lrelu_tie_channels', {})),
                 'ok' if all(n > 0 for n in ran.values()) else 'MISSING', worst_arith[0], worst_lag[0]))
    assert all(n > 0 for n in ran.values()), ran
    assert taken[0] >= 0.6 * n_params, rep['direct_gradients']
    assert rep['loss_d'] <= TOL and rep['loss_g'] <= TOL, rep
    assert not still, still
    _assert_ties_are_rare(rep, len(ed) + len(eg))
    assert len(ed) >= 20 and len(eg) >= 20 and n_upd > 10 ** 6
    assert worst_arith[0] <= 1.0, rep
    assert worst_upd[0] <= 2e-2, rep
    assert worst_lag[0] <= 1e-4, rep
