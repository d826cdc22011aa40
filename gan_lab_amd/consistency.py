"""Consistency regularisation of the ResNet GAN: bCR (Zhang et al., ICLR 2020, "Consistency Regularization for GANs") and zCR
(Zhao et al. 2020, "Improved Consistency Regularization for GANs"; bCR + zCR = ICR).  DESIGN.md 4.17.

With ``T`` a horizontal flip and an integer shift drawn afresh for every image, ``z' = z + cr_sigma * n`` for a fresh normal ``n``,
``msd`` the mean over the batch of the squared difference of critic scores and ``imsd`` the mean over every element of the squared
difference of images, the critic step adds

    cr_real * msd(D(x), D(T(x))) + cr_fake * msd(D(G(z)), D(T(G(z)))) + cr_latent_d * msd(D(G(z)), D(G(z')))

and the generator step ``- cr_latent_g * imsd(G(z), G(z'))``.  The terms are first order in the critic, so they compose with every
loss and penalty, with spectral normalisation and with a critic's self-attention block; they are per-rank means that join the
loss before the gradient all-reduce, and they carry no state (checkpoints are unchanged).  ``diffaugment`` / ``ada`` are excluded:
which augmentation parameters ``x`` and ``T(x)`` should share is a question of its own.

Only the terms with a positive weight are evaluated, and only their batches produced.  With all four weights at 0 the learner holds
no ``Consistency`` at all: nothing is drawn from the Philox stream, nothing launched.

New kernels (csrc/cr.hip): ``ops.cr_transform`` (one launch over the batch, bit-exact), ``ops.cr_msd`` / ``ops.cr_imsd`` (fp64
accumulation in a fixed order, bitwise reproducible, one launch backward), ``rng.cr_params`` (one Philox counter per image).  The
extra critic and generator passes run on the kernels that are already there.

A zCR generator pass runs ``[z; z']`` as one batch of 2N with the labels repeated: the generator's BatchNorm statistics are then
taken over both halves (one pass instead of two, and the pair is normalised alike, so ``G(z) - G(z')`` measures the latent's
effect alone); in the critic step the adversarial terms therefore see ``G(z)`` normalised with the statistics of the 2N batch.
"""
import math

import torch

from . import ops, rng

WEIGHTS = ('cr_real', 'cr_fake', 'cr_latent_d', 'cr_latent_g')


def _weight(config, name):
    v = getattr(config, name, 0.)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f'config.{name} must be a finite number >= 0 (got {v!r})')
    return float(v)


def validate_config(config):
    """The ``cr_*`` fields of ``config``; raises ValueError.  -> a ``Consistency``, or None with all four weights at 0."""
    w = {name: _weight(config, name) for name in WEIGHTS}
    if not any(w.values()):
        return None
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.cr_real / cr_fake / cr_latent_d / cr_latent_g are ResNet GAN options')
    for other in ('diffaugment', 'ada'):
        if getattr(config, other, None) is not None:
            raise ValueError(f'consistency regularisation (config.cr_*) excludes config.{other}: which augmentation parameters x '
                             f'and T(x) should share is not decided here; set config.{other}=None or the cr_* weights to 0')
    sigma = getattr(config, 'cr_sigma', 0.03)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not math.isfinite(sigma) or \
            ((w['cr_latent_d'] > 0 or w['cr_latent_g'] > 0) and sigma <= 0):
        raise ValueError(f'config.cr_sigma must be a finite number > 0 while cr_latent_d or cr_latent_g is positive (got '
                         f'{sigma!r})')
    res = int(config.res_samples)
    shift = getattr(config, 'cr_shift', None)
    if shift is None:
        shift = res // 8
    if isinstance(shift, bool) or not isinstance(shift, int) or shift < 0 or shift >= res:
        raise ValueError(f'config.cr_shift must be None or an integer in [0, res_samples = {res}) (got {shift!r})')
    flip = getattr(config, 'cr_flip', True)
    if not isinstance(flip, bool):
        raise ValueError(f'config.cr_flip must be a bool (got {flip!r})')
    return Consistency(w['cr_real'], w['cr_fake'], w['cr_latent_d'], w['cr_latent_g'], float(sigma), shift, flip)


def saved_config_fields(cfg):
    """``cfg`` (a dict of config fields) as a checkpoint stores it: with all four weights at 0 no ``cr_*`` field is written, so
    files saved with the feature off are what they were before it existed."""
    if any(cfg.get(name) for name in WEIGHTS):
        return cfg
    return {k: v for k, v in cfg.items() if not k.startswith('cr_')}


class Consistency(object):
    """The weights and draws of the consistency terms of one learner (``validate_config``)."""

    def __init__(self, real, fake, latent_d, latent_g, sigma, shift, flip):
        self.real, self.fake, self.latent_d, self.latent_g = real, fake, latent_d, latent_g
        self.sigma, self.shift, self.flip = sigma, shift, flip

    @property
    def balanced(self):
        """Does the critic step transform a batch (bCR)?"""
        return self.real > 0 or self.fake > 0

    def draw_params(self, n, device):
        """(2n, 4) transform rows, [0, n) for the generated batch and [n, 2n) for the real one: one launch, 2n counters."""
        return rng.cr_params(2 * n, self.shift, self.flip, device)

    def check_params(self, params, n):
        if not isinstance(params, torch.Tensor) or params.dtype != torch.int32 or tuple(params.shape) != (2 * n, 4):
            raise ValueError(f'cr_params must be a ({2 * n}, 4) int32 tensor: rows [0, {n}) for the generated batch, '
                             f'[{n}, {2 * n}) for the real one (got {getattr(params, "dtype", None)}, '
                             f'{tuple(getattr(params, "shape", ()))})')
        return params

    def perturb(self, zb, noise=None):
        """``z' = z + sigma * n``; ``n``: a fresh draw of ``z``'s shape from the process stream unless given (tests)."""
        if noise is None:
            noise = rng.randn(tuple(zb.shape), zb.device)
        elif tuple(noise.shape) != tuple(zb.shape):
            raise ValueError(f'cr_noise must have the shape of the latents {tuple(zb.shape)} (got {tuple(noise.shape)})')
        return ops.k_axpby(noise, zb, self.sigma, 1.0)

    @staticmethod
    def transform(x, params):
        return ops.cr_transform(x.detach(), params)
