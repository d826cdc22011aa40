"""The power-spectrum regulariser of the progressive generators (Durall et al. 2020, "Watch your Up-Convolution": the distance of the
generated images' radial power spectrum from the reals', added to the generator's loss), on the GPU (csrc/spectrum.hip; DESIGN.md
4.9b).  It is the backward half of the 'spectrum' metric (spectrum.py): what a user can do inside this package when ``spectrum hf``
drifts.

With ``S[k]`` the set profile of a batch as spectrum.py defines it (window, power, integer bins, mean over the images), a target
profile ``T[k]`` and a band ``B`` - ``'all'``: k = 1 .. R/2, ``'hf'``: k = R/4+1 .. R/2, the metric's own two bands, DC never -

    L = mean_{k in B} (ln max(S[k], 1e-30) - ln max(T[k], 1e-30))^2

``config.spectrum_reg`` (ProGAN / StyleGAN; float, 0 = off, finite and >= 0) is the weight of ``L`` in the generator's loss,
``config.spectrum_reg_band`` the band (``'hf'``), ``config.spectrum_reg_decay`` (0.99, in [0, 1)) the decay of the target, and the
window is the metric's ``config.spectrum_window``.  The critic step moves the target towards the real batch as the critic sees it
before augmentation, ``T <- decay T + (1 - decay) S(real)`` (the first observation copies); the generator step adds
``spectrum_reg * ops.spectrum_loss(fake, T, band)`` on the un-augmented fakes and keeps the unweighted term in
``last_losses['spectrum_reg']``.  ``T`` lives on the device, is per rank (not all-reduced), is dropped at a growth event and rebuilt
at the new size, and travels in checkpoints only while the option is on.  Below ``MIN_RES`` (the 4^2 and 8^2 phases) nothing is
launched and the term is None.  With the weight at 0 nothing is built, drawn or launched.

The kernels are not captured into step graphs: with the option on the learner steps eagerly (graphs.GraphedStep reports itself not
eligible)."""
import math

import torch

from . import ops
from .spectrum import MAX_RES, MIN_RES, check_options

BANDS = ops.SPECTRUM_BANDS
FIELDS = ('spectrum_reg', 'spectrum_reg_band', 'spectrum_reg_decay')


def _number(config, name, default):
    v = getattr(config, name, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f'config.{name} must be a finite number (got {v!r})')
    return v


def validate_config(config):
    """The ``spectrum_reg*`` fields of ``config``; raises ValueError and names the field.  -> None with ``spectrum_reg`` = 0, else
    ``dict(weight=, band=, decay=, window=)``."""
    weight = _number(config, 'spectrum_reg', 0.0)
    if weight < 0:
        raise ValueError(f'config.spectrum_reg must be finite and >= 0 (got {weight!r})')
    progressive = getattr(config, 'model', None) in ('ProGAN', 'StyleGAN')
    if not progressive:
        if weight or hasattr(config, 'spectrum_reg_band') or hasattr(config, 'spectrum_reg_decay'):
            raise ValueError('config.spectrum_reg is a ProGAN / StyleGAN option (the ResNet GAN learner has no power-spectrum '
                             'regulariser)')
        return None
    band = getattr(config, 'spectrum_reg_band', 'hf')
    if not isinstance(band, str) or band not in BANDS:
        raise ValueError(f'config.spectrum_reg_band must be one of {sorted(BANDS)} (got {band!r})')
    decay = _number(config, 'spectrum_reg_decay', 0.99)
    if not 0 <= decay < 1:
        raise ValueError(f'config.spectrum_reg_decay must be in [0, 1) (got {decay!r})')
    if weight == 0:
        return None
    return dict(weight=float(weight), band=band, decay=float(decay),
                window=check_options(getattr(config, 'spectrum_window', 'hann'), prefix='spectrum_'))


def saved_config_fields(cfg):
    """``cfg`` (a dict of config fields) as a checkpoint stores it: with ``spectrum_reg`` = 0 no ``spectrum_reg*`` field is written, so
    files saved with the option off are what they were before the fields existed."""
    if cfg.get('spectrum_reg'):
        return cfg
    return {k: v for k, v in cfg.items() if k not in FIELDS}


def from_config(config):
    opts = validate_config(config)
    return None if opts is None else SpectrumRegulariser(device=config.dev, **opts)


class SpectrumRegulariser(object):
    """The target profile ``T`` of the current resolution on the device, its moving average over the real batches and the loss
    term of the generator step."""

    def __init__(self, weight, band='hf', decay=0.99, window='hann', device='cuda'):
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(weight) or weight < 0:
            raise ValueError(f'spectrum_reg: the weight must be finite and >= 0 (got {weight!r})')
        if band not in BANDS:
            raise ValueError(f'spectrum_reg: band must be one of {sorted(BANDS)} (got {band!r})')
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0 <= decay < 1:
            raise ValueError(f'spectrum_reg: decay must be in [0, 1) (got {decay!r})')
        self.weight, self.band, self.decay, self.window = float(weight), band, float(decay), check_options(window)
        self.device = torch.device(device)
        self.target = None          # (R/2 + 1,) fp64 on the device, None until the first observation at this resolution

    @staticmethod
    def active(res):
        """Does the transform cover ``res`` x ``res`` images?  (Not the 4^2 and 8^2 phases: nothing is launched there.)"""
        return MIN_RES <= int(res) <= MAX_RES

    def reset(self):
        """A growth event: the target is rebuilt at the new size from the next real batch."""
        self.target = None

    def _fresh(self, res, device):
        if self.target is not None and self.target.numel() == res // 2 + 1:
            return False
        self.target = torch.empty(res // 2 + 1, dtype=torch.float64, device=device)
        return True

    def observe(self, real):
        """``T <- decay T + (1 - decay) S(real)``; the first observation (and the first at a new size) copies.  No host read."""
        res = int(real.shape[-1])
        if not self.active(res):
            return
        first = self._fresh(res, real.device)
        try:
            ops.spectrum_target_update(real, self.target, self.decay, first, self.window)
        except Exception:
            if first:
                self.target = None
            raise

    def set_target(self, images):
        """``T = S(images)``: a fixed reference set (N, 3, R, R), or a test's."""
        self.target = ops.spectrum_profile_mean(images, self.window)

    def loss(self, fake):
        """The unweighted term of (N, 3, R, R) generated images as a 0-dim device tensor with its backward, or None below ``MIN_RES``."""
        res = int(fake.shape[-1])
        if not self.active(res):
            return None
        if self.target is None or self.target.numel() != res // 2 + 1:
            raise RuntimeError(f'spectrum_reg: no target profile at {res}x{res} yet: run a critic step on a real batch first, or give '
                               f'one with set_target(images)')
        return ops.spectrum_loss(fake, self.target, self.band, self.window)

    # -- checkpoints ---------------------------------------------------------------------------------------------------------
    def state(self):
        return {'spectrum_reg_target': None if self.target is None else self.target.detach().cpu()}

    def restore(self, ck):
        t = ck.get('spectrum_reg_target')
        self.target = None if t is None else t.to(device=self.device, dtype=torch.float64).contiguous()
