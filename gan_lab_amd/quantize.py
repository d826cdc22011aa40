"""Feature quantisation for the ResNet GAN critic (Zhao et al., ICML 2020, "Feature Quantization Improves GAN Training"; FQ-BigGAN):
the configuration surface.  The layer itself is NOT in the package yet - its kernels are not merged - so this module holds what
can be decided without them: the ``fq_*`` fields, their ranges and the options they exclude.  tests/fq_reference.py states the
arithmetic the layer will have to compute.

``config.fq_codes`` = K (ResNet GAN only; 0 = off, else in [1, 4096]; FQ-BigGAN uses 2^10) asks for a layer in the critic that
replaces every spatial feature vector by the nearest of K dictionary rows (straight-through gradient) and lets the dictionary follow
the features by Laplace-smoothed moving averages with ``config.fq_decay`` (0.8; in [0, 1)); the critic step adds
``config.fq_commit`` (1.0; finite and >= 0) times the mean squared distance of the features from their codes to its loss.  The
layer is first order, like the critic's attention block, so ``fq_codes > 0`` excludes the gradient penalties (hinge loss + spectral
normalisation is the recipe it belongs to).

``validate_config`` checks all of that when the learner is built and names the field at fault.  A valid request with
``fq_codes > 0`` is then refused by ``require_layer`` as ``NotImplementedError`` - there is no PyTorch fall-back for a missing
kernel - the way ``cgan='acgan'`` is refused (conditional.py).  With ``fq_codes`` = 0 nothing is built and checkpoints keep the
config they have always had (``saved_config_fields``).
"""
import math

MAX_CODES = 4096
FIELDS = ('fq_codes', 'fq_decay', 'fq_commit')


def _number(config, name, default):
    v = getattr(config, name, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f'config.{name} must be a finite number (got {v!r})')
    return v


def validate_config(config):
    """The ``fq_*`` fields of ``config``; raises ValueError and names the field.  -> None with ``fq_codes`` = 0, else
    ``dict(codes=, decay=, commit=)``."""
    codes = getattr(config, 'fq_codes', 0)
    if isinstance(codes, bool) or not isinstance(codes, int) or not 0 <= codes <= MAX_CODES:
        raise ValueError(f'config.fq_codes must be 0 (off) or an integer in [1, {MAX_CODES}] (got {codes!r})')
    decay, commit = _number(config, 'fq_decay', 0.8), _number(config, 'fq_commit', 1.0)
    if not 0 <= decay < 1:
        raise ValueError(f'config.fq_decay must be in [0, 1) (got {decay!r})')
    if commit < 0:
        raise ValueError(f'config.fq_commit must be finite and >= 0 (got {commit!r})')
    if codes == 0:
        return None
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.fq_codes is a ResNet GAN option (the progressive critics have no quantisation layer)')
    if getattr(config, 'gradient_penalty', None) is not None:
        raise ValueError(f"config.fq_codes={codes} puts a quantisation layer into the critic, and the double backward of a gradient "
                         f"penalty (config.gradient_penalty={config.gradient_penalty!r}) through it is not provided: train it with "
                         f"loss='hinge', spectral_norm=True and gradient_penalty=None")
    return dict(codes=codes, decay=float(decay), commit=float(commit))


def require_layer(fq):
    """``fq``: what ``validate_config`` returned.  A valid request for the layer is refused until its kernels are in the package."""
    if fq is not None:
        raise NotImplementedError(f"config.fq_codes={fq['codes']}: the feature quantisation layer's kernels are not in this package "
                                  f"yet and there is no PyTorch fall-back; set config.fq_codes=0")


def saved_config_fields(cfg):
    """``cfg`` (a dict of config fields) as a checkpoint stores it: with ``fq_codes`` = 0 no ``fq_*`` field is written, so files
    saved with the feature off are what they were before the fields existed."""
    if cfg.get('fq_codes'):
        return cfg
    return {k: v for k, v in cfg.items() if not k.startswith('fq_')}
