"""Projection of images into StyleGAN's latent space (Karras et al. 2020, the StyleGAN2 projector): given images, find the
dlatents whose synthesis reproduces them - one dlatent per image (W) or one per image and layer (W+).  DESIGN.md 4.21.

An iteration is ``StyleGenerator.synthesis`` -> ``ops.pyramid_mse`` -> ``torch.autograd.grad`` to the dlatents only ->
``ops.project_step``.  The generator's forward and backward are the fused kernels the training step uses; the loss with its
gradient, the moments of W and the latent update are csrc/project.hip.  The dlatents, Adam's moments, the iteration count and the
per-step losses stay on the device; the host reads nothing back while the iterations run.

The reconstruction loss is a multi-scale mean squared error in the network's image space: ``sum_l weights[l] * mean(d_l^2)`` with
``d_0 = G(w) - target`` and ``d_{l+1}`` the 2x2 mean of ``d_l`` (the coarse levels pull the layout into place before the fine ones
can).  There is no perceptual network here, and the per-layer noise inputs are held fixed, not optimised.

Everything random - the latents behind ``w_avg``, the noise maps, the exploration noise - is a pure function of ``seed``; the
process's training stream (gan_lab_amd/rng.py) is not touched.
"""
import torch

from . import ops

SPACES = ('w', 'w+')
NOISE_MODES = ('const', 'none')
_MASK = 2 ** 64 - 1
_W_AVG_CHUNK = 4096           # mapped latents per mapping-network call


def _substream(seed, k):
    """Philox key of sub-stream k (0: the latents behind w_avg, 1: the noise maps, 2: the exploration noise) of a projection
    seeded with ``seed``."""
    return (int(seed) * 0x9E3779B97F4A7C15 + (int(k) + 1) * 0xD1B54A32D192ED03 + 0x50524F4A) & _MASK


class Projection(object):
    """What ``project`` returns: ``ws`` (N, L, D) the projected dlatents without the exploration noise, ``images`` (N, 3, R, R)
    their synthesis in [0, 1] image space (not clamped), ``loss`` (steps, N) the per-step losses as a device tensor, ``w_avg`` (D,)
    and ``w_std`` (0-dim) the moments of W the run started from."""
    __slots__ = ('ws', 'images', 'loss', 'w_avg', 'w_std')

    def __init__(self, ws, images, loss, w_avg, w_std):
        self.ws, self.images, self.loss, self.w_avg, self.w_std = ws, images, loss, w_avg, w_std


def _int_arg(name, value, lo):
    if isinstance(value, bool) or not isinstance(value, int) or value < lo:
        raise ValueError(f'project: {name} must be an integer >= {lo} (got {value!r})')
    return value


def check_options(res, steps, space, levels, weights, noise_mode, w_avg_samples, seed, schedule):
    """Validate everything about a projection at resolution ``res`` that does not depend on a tensor; returns ``(weights tuple,
    hyper)``, ``hyper`` the six doubles of ``ops.project_step``.  Every refusal is a ValueError that names the argument."""
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError(f'project: steps must be an integer >= 1 (got {steps!r})')
    if space not in SPACES:
        raise ValueError(f"project: space must be 'w' or 'w+' (got {space!r})")
    if noise_mode not in NOISE_MODES:
        raise ValueError(f"project: noise_mode must be 'const' or 'none' (got {noise_mode!r})")
    _int_arg('w_avg_samples', w_avg_samples, 1)
    if _int_arg('seed', seed, 0) >= 2 ** 63:
        raise ValueError(f'project: seed must be an integer in [0, 2**63) (got {seed!r})')
    top = ops.pyramid_max_levels(res)
    if levels is not None and (isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= top):
        raise ValueError(f'project: levels must be an integer in [1, {top}] at {res}x{res}, or None for all (got {levels!r})')
    if weights is None:
        weights = (1.0,) * (top if levels is None else levels)
    weights = ops.check_pyramid_weights(weights, res, 'project: weights')
    if levels is not None and len(weights) != levels:
        raise ValueError(f'project: weights must hold one value per level, {levels} (got {len(weights)})')
    if not any(w > 0 for w in weights):
        raise ValueError(f'project: weights must not all be zero (got {weights!r})')
    return weights, ops.check_project_schedule(steps, schedule, 'project')


def _latents(gen, count, key, dev):
    """``count`` latents of the generator's distribution from the Philox key ``key`` alone."""
    if gen.latent_distribution == 'normal':
        return ops.randn((count, gen.len_latent), key, 0, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(key & (2 ** 63 - 1))
    return torch.rand(count, gen.len_latent, dtype=torch.float32, device=dev, generator=g)


def project(learner, targets, steps=1000, space='w', levels=None, weights=None, noise_mode='const', time_average=True,
            w_avg_samples=10000, seed=0, **schedule):
    """Project ``targets`` - (N, 3, R, R) in [0, 1] image space at the generator's current resolution - into the latent space of
    ``learner``'s StyleGAN generator (the EWMA one with ``time_average``, else the live one), in eval mode.

    ``w_avg`` and ``w_std`` come from ``w_avg_samples`` mapped latents; every target starts at ``w_avg`` and takes ``steps``
    iterations of Adam under the StyleGAN2 projector's schedule (``**schedule``: ``ops.PROJECT_SCHEDULE``'s keys) in ``space`` 'w'
    or 'w+'.  ``levels`` / ``weights``: the pyramid of ``ops.pyramid_mse`` (None: every level it allows, weight 1 each).
    ``noise_mode`` 'const' fixes one (1, 1, h, w) noise map per layer for all samples and steps, 'none' switches the noise
    inputs off.  Returns a ``Projection``.

    Nothing of the learner changes: the parameters' ``requires_grad`` flags are off for the duration and put back, no weight
    gradient is computed, optimiser state, EWMA, ``w_ewma``, module modes and the training random stream stay as found."""
    from .stylegan.architectures import StyleGenerator
    live = getattr(learner, 'gen_model', None)
    if not isinstance(live, StyleGenerator):
        raise TypeError('project: the learner has no StyleGAN generator (only StyleGAN has a W space)')
    res = int(live.curr_res)
    weights, hyper = check_options(res, steps, space, levels, weights, noise_mode, w_avg_samples, seed, schedule)
    if learner.ds_mean is None or learner.ds_std is None:
        raise ValueError("project: the learner holds no ds_mean / ds_std (the dataset's mean and std map the targets into the "
                         "network's image space); provide them from the data configuration or a pretrained model")
    if live.fade_in_phase:
        raise ValueError('project: not available while fade_in_phase is set (the image then blends two resolutions)')
    if not isinstance(targets, torch.Tensor) or targets.dim() != 4 or targets.shape[0] < 1 or targets.shape[1] != 3 or \
            tuple(targets.shape[2:]) != (res, res):
        raise ValueError(f'project: targets must be (N, 3, {res}, {res}), the current resolution (got '
                         f'{tuple(getattr(targets, "shape", ()))})')
    dev = learner.config.dev

    kept_lagged = learner.gen_model_lagged
    if time_average and kept_lagged is None:
        learner.materialize_lagged_generator().to(dev)       # a private copy of the EWMA shadow: not kept on the learner
    gen = learner.gen_model_lagged if time_average else live
    learner.gen_model_lagged = kept_lagged
    modes = [(mod, mod.training) for mod in gen.modules()]
    switches = (gen._use_noise, gen._use_mixing_reg)
    flags = [(p, p.requires_grad) for p in gen.parameters()]
    try:
        gen.eval()
        if noise_mode == 'none' and gen._trained_with_noise:
            gen.use_noise = False
        for p, _ in flags:
            p.requires_grad_(False)
        return _run(gen, targets, learner.ds_mean, learner.ds_std, dev, steps, space, weights, hyper, noise_mode, w_avg_samples,
                    seed)
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        for mod, mode in modes:
            mod.training = mode
        gen._use_noise, gen._use_mixing_reg = switches


def _run(gen, targets, ds_mean, ds_std, dev, steps, space, weights, hyper, noise_mode, w_avg_samples, seed):
    n, layers, d = targets.shape[0], len(gen.gen_layers), gen.len_dlatent
    std, mean = ds_std.to(dev).float().view(1, -1, 1, 1), ds_mean.to(dev).float().view(1, -1, 1, 1)
    target = ((targets.to(dev).float() - mean) / std).contiguous()

    with torch.no_grad():
        z = _latents(gen, w_avg_samples, _substream(seed, 0), dev)
        w_avg, w_std = ops.w_moments(torch.cat([gen.z_to_w(z[i:i + _W_AVG_CHUNK]) for i in range(0, len(z), _W_AVG_CHUNK)]))

    maps = None
    if noise_mode == 'const' and gen.use_noise:
        maps, offset = [], 0
        for k in range(layers):
            side = 4 * 2 ** (k // 2)
            maps.append(ops.randn((1, 1, side, side), _substream(seed, 1), offset, dev))
            offset += (side * side + 3) // 4

    shape = (n, layers, d) if space == 'w+' else (n, d)
    w_opt = w_avg.expand(shape).contiguous()
    m, v = torch.zeros_like(w_opt), torch.zeros_like(w_opt)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    w_in = torch.empty((n, layers, d), dtype=torch.float32, device=dev, requires_grad=True)
    loss_log = torch.empty((steps, n), dtype=torch.float32, device=dev)
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    per_draw = (w_opt.numel() + 3) // 4

    def explore(k):
        return ops.randn(shape, _substream(seed, 2), k * per_draw, dev)

    ops.project_step(w_opt, None, m, v, step, explore(0), w_std, w_in.detach(), hyper)
    for k in range(steps):
        loss, _ = ops.pyramid_mse(gen.synthesis(w_in, noise=maps), target, weights)
        loss_log[k].copy_(loss.detach())
        grad, = torch.autograd.grad(loss, w_in, grad_outputs=ones)
        ops.project_step(w_opt, grad, m, v, step, explore(k + 1), w_std, w_in.detach(), hyper)

    with torch.no_grad():
        ws = (w_opt if space == 'w+' else w_opt.unsqueeze(1).expand(n, layers, d)).contiguous()
        images = gen.synthesis(ws, noise=maps) * std + mean
    return Projection(ws, images, loss_log, w_avg, w_std)
