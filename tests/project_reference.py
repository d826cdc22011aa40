"""Plain-torch statement of what csrc/project.hip and gan_lab_amd/project.py compute, usable in float64 (the reference) and in
float32 (the restatement whose own rounding error sets the tests' bars): the multi-scale loss as an ``avg_pool2d`` chain with
autograd for its gradient, the analytic gradient, the StyleGAN2 projector's schedule, the Adam-and-noise step, the moments of W."""
import math

import torch
import torch.nn.functional as F

SCHEDULE = dict(lr0=0.1, initial_noise_factor=0.05, lr_rampdown_length=0.25, lr_rampup_length=0.05, noise_ramp_length=0.75)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def pyramid(x, t, levels):
    """[d_0, ..., d_{levels-1}]: d_0 = x - t, d_{l+1} the 2x2 mean of d_l."""
    d = [x - t]
    for _ in range(levels - 1):
        d.append(F.avg_pool2d(d[-1], 2))
    return d


def pyramid_terms(x, t, levels):
    """(N, levels): terms[n, l] = mean over (c, h, w) of d_l[n]^2."""
    return torch.stack([(d * d).mean(dim=(1, 2, 3)) for d in pyramid(x, t, levels)], dim=1)


def pyramid_loss(x, t, weights):
    """(N,): loss[n] = sum_l weights[l] * terms[n, l]."""
    w = torch.tensor(list(weights), dtype=x.dtype)
    return (pyramid_terms(x, t, len(weights)) * w).sum(dim=1)


def pyramid_grad_autograd(x, t, weights, upstream=None):
    """d (sum_n upstream[n] loss[n]) / d x by autograd through the pooling chain."""
    x = x.detach().clone().requires_grad_(True)
    loss = pyramid_loss(x, t, weights)
    up = torch.ones_like(loss) if upstream is None else upstream.to(loss.dtype)
    return torch.autograd.grad(loss, x, grad_outputs=up)[0]


def pyramid_grad_analytic(x, t, weights):
    """2 / (C R^2) * sum_l weights[l] * up_l(d_l), up_l the nearest upsampling by 2^l (R_l^2 4^l = R^2)."""
    c, r = x.shape[1], x.shape[2]
    acc = torch.zeros_like(x)
    for l, (w, d) in enumerate(zip(weights, pyramid(x, t, len(weights)))):
        acc = acc + w * d.repeat_interleave(2 ** l, dim=2).repeat_interleave(2 ** l, dim=3)
    return acc * (2.0 / (c * r * r))


def schedule(step, num_steps, w_std, dtype=torch.float64, **hyper):
    """(lr, noise scale) of the StyleGAN2 projector at ``t = step / num_steps``, as 0-dim tensors of ``dtype``."""
    h = dict(SCHEDULE, **hyper)
    one = torch.ones((), dtype=dtype)
    t = one * step / num_steps
    scale = torch.as_tensor(w_std, dtype=dtype) * h['initial_noise_factor'] * torch.clamp(1 - t / h['noise_ramp_length'], min=0) ** 2
    r = torch.clamp((1 - t) / h['lr_rampdown_length'], max=1)
    lr = h['lr0'] * (0.5 - 0.5 * torch.cos(math.pi * r)) * torch.clamp(t / h['lr_rampup_length'], max=1)
    return lr, scale


def project_step(state, grad_ws, noise, w_std, num_steps, **hyper):
    """One update, in the dtype of ``state['w_opt']``.  ``state``: dict(w_opt, m, v, step) with ``step`` a Python int;
    ``w_opt`` (N, D) sums ``grad_ws`` (N, L, D) over L in layer order (W), (N, L, D) takes it as it is (W+).  torch.optim.Adam's
    update (bias-corrected) with the schedule's learning rate at ``step``; then ``step += 1``.  Returns the next forward's input
    ``w_in`` (N, L, D) = w_opt + scale(step) * noise, broadcast over L in W space."""
    w, dtype = state['w_opt'], state['w_opt'].dtype
    layers = grad_ws.shape[1]
    g = grad_ws.to(dtype)
    if w.dim() == 2:
        total = g[:, 0].clone()
        for l in range(1, layers):
            total = total + g[:, l]
        g = total
    lr, _ = schedule(state['step'], num_steps, w_std, dtype, **hyper)
    k = state['step'] + 1
    state['m'] = state['m'] + (g - state['m']) * (1 - BETA1)
    state['v'] = state['v'] * BETA2 + (1 - BETA2) * g * g
    bc1, bc2 = 1 - BETA1 ** k, 1 - BETA2 ** k
    denom = state['v'].sqrt() / math.sqrt(bc2) + EPS
    state['w_opt'] = w - (lr / bc1) * state['m'] / denom
    state['step'] = k
    return w_in(state, noise, w_std, num_steps, layers, **hyper)


def w_in(state, noise, w_std, num_steps, layers, **hyper):
    """w_opt + scale(state['step']) * noise as (N, L, D)."""
    w = state['w_opt']
    _, scale = schedule(state['step'], num_steps, w_std, w.dtype, **hyper)
    out = w + scale * noise.to(w.dtype)
    return out.unsqueeze(1).expand(-1, layers, -1).clone() if out.dim() == 2 else out


def w_moments(ws):
    """(w_avg (D,), w_std 0-dim): the column means and sqrt(sum (w - w_avg)^2 / M) over all entries, two passes."""
    avg = ws.sum(dim=0) / ws.shape[0]
    return avg, (((ws - avg) ** 2).sum() / ws.shape[0]).sqrt()


def rel_err(a, ref):
    """max |a - ref| / max |ref| in float64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()
