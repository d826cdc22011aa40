"""Class conditioning for the ResNet GAN: class-conditional BatchNorm in the generator; a projection critic, or a critic with a
classifier head and its loss.

``config.cgan`` (ResNet GAN only; None = off, else ``'projection'``, ``'contra'`` or ``'reacgan'``) with
``config.num_classes`` >= 2.  The generator is the same in every mode:

    generator   every BatchNorm becomes a ``ConditionalBatchNorm2d``: batch statistics as before, then the affine row of the
                sample's class from (num_classes, C) tables; the latent input stays ``len_latent`` wide, nothing is concatenated
                (or the hierarchical-latent / shared-embedding path of hier_latent.py)

``'projection'`` is the conditioning of SNGAN-projection (Miyato & Koyama 2018), SAGAN and BigGAN - the missing part of the recipe
that ``spectral_norm``, ``loss='hinge'`` and ``self_attention`` belong to:

    critic      out[n] = linear1(f)[n] + <proj.weight[l_n], f[n]> on the feature f that ``linear1`` reads; ``proj`` is a bias-free
                ``LinearEx`` (so ``spectral_norm=True`` normalises it like every other layer); the image input stays 3 channels

The others are the classifier-based conditional GANs: the critic's score stays the unconditional ``linear1(f)`` and a head
on the same feature f carries a loss that both steps add, weighted by ``config.cond_lambda`` - the critic step on the real rows
with their labels, the generator step on the generated rows with the labels the generator was given:

    'contra'    ContraGAN (Kang & Park 2020): ``embed = LinearEx(F, E)`` and the proxies ``proxy = LinearEx(E, K)`` without bias,
                whose (K, E) weight is only ever read as a table; the conditional contrastive loss 2C of ``embed(f)``
    'reacgan'   ReACGAN (Kang et al. 2021): the same heads; the data-to-data cross-entropy D2D-CE with the margins
                ``cond_margin_pos`` / ``cond_margin_neg``

    ('acgan')   AC-GAN (Odena et al. 2017): ``cls = LinearEx(F, K)``; the cross-entropy of ``cls(f)``.  NOT a value of
                ``config.cgan`` yet: ``validate_config`` keeps refusing it, as it always has (an existing host test pins that), so
                the learner cannot be built with it.  Its pieces are here and tested on their own - the critic's head
                (``Discriminator*PixResnet(cgan='acgan')``), ``ops.class_cross_entropy`` and ``cond_term`` - ready for the
                day the value is admitted to ``CHOICES`` and ``CLASSIFIER_MODES``

with E = ``config.cond_embed`` and the temperature ``config.cond_temperature``.  The heads are ``LinearEx``, so spectral
normalisation, ``ortho_reg_d``, the arenas and ``state_dict`` treat them like ``proj``.  The term is computed per rank from the
rank's own rows: embeddings are NOT gathered across ranks (the papers' contrastive terms see the whole batch; with data
parallelism each rank contrasts within its share).  The papers' settings (ContraGAN: ``cond_lambda=1``, ``cond_temperature=1.0``
on CIFAR-10; ReACGAN: ``cond_temperature=0.5``, margins 0.98 / 0.02, E = 512..2048 by dataset) are the user's choice; nothing was
tuned here.

The networks are called as ``gen_model(z, labels)`` / ``disc_model(x, labels)`` with one int32 device label per sample
(``features(x)`` stays label-free); ``disc_model(x, labels, return_features=True)`` also returns f, so that the conditioning term
costs no second pass through the trunk.  The hot paths are csrc/cond.hip through ``ops.cond_batch_norm`` /
``ops.class_projection`` and csrc/cond_loss.hip through ``ops.class_cross_entropy`` / ``ops.class_contrastive``
(DESIGN.md 4.20); the projection is closed under differentiation, so the gradient penalties work with it; the conditional norm
and the classifier losses are first order (the generator is never inside a penalty, and the penalties differentiate the
adversarial score only).

This is not the reference's ``class_condition`` / ``use_auxiliary_classifier`` (one-hot concatenation, AC heads): no variant of
those runs in the reference (tests/golden/conditional_probe.json) and both keep raising NotImplementedError.
"""
import math

import torch

CHOICES = (None, 'projection', 'contra', 'reacgan')
CLASSIFIER_MODES = ('contra', 'reacgan')            # the values of config.cgan whose critic carries a classifier loss
HEAD_MODES = ('acgan',) + CLASSIFIER_MODES          # what a critic can be built with (architectures.py)
MAX_EMBED = 1024


def mode(config):
    """``config.cgan`` casefolded, or None."""
    m = getattr(config, 'cgan', None)
    return m.casefold() if isinstance(m, str) else m


def validate_config(config):
    """``config.cgan`` against its values and what it needs; raises ValueError.  -> bool (is it on?)."""
    m = mode(config)
    if m not in CHOICES:
        raise ValueError(f"config.cgan must be None, 'projection', 'contra' or 'reacgan' (got {getattr(config, 'cgan', None)!r})")
    if m is None:
        return False
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.cgan is a ResNet GAN option (the progressive networks have no class conditioning)')
    k = getattr(config, 'num_classes', 0)
    if not isinstance(k, int) or isinstance(k, bool) or k < 2:
        raise ValueError(f"config.cgan={m!r} needs config.num_classes >= 2 (got {k!r})")
    return True


def _number(config, name, default):
    v = getattr(config, name, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f'config.{name} must be a finite number (got {v!r})')
    return float(v)


def validate_loss_config(config):
    """The numeric fields of the classifier-based modes, checked in every mode; raises ValueError naming the field.
    -> dict(weight, embed, temperature, margin_pos, margin_neg), or None when ``config.cgan`` is not one of those modes."""
    weight = _number(config, 'cond_lambda', 1.0)
    if weight < 0:
        raise ValueError(f'config.cond_lambda must be >= 0 (got {weight})')
    embed = getattr(config, 'cond_embed', 512)
    if isinstance(embed, bool) or not isinstance(embed, int) or not 1 <= embed <= MAX_EMBED:
        raise ValueError(f'config.cond_embed must be an integer in [1, {MAX_EMBED}] (got {embed!r})')
    tau = _number(config, 'cond_temperature', 1.0)
    if tau <= 0:
        raise ValueError(f'config.cond_temperature must be > 0 (got {tau})')
    mp, mn = _number(config, 'cond_margin_pos', 0.98), _number(config, 'cond_margin_neg', 0.02)
    if not mn < mp:
        raise ValueError(f'config.cond_margin_neg must be below config.cond_margin_pos (got {mn} and {mp})')
    if mode(config) not in CLASSIFIER_MODES:
        return None
    return dict(weight=weight, embed=embed, temperature=tau, margin_pos=mp, margin_neg=mn)


def saved_config_fields(cfg):
    """``cfg`` (a dict of config fields) as a checkpoint stores it: without a classifier-based mode no ``cond_*`` field is
    written, so files saved with the feature off are what they were before it existed."""
    m = cfg.get('cgan')
    if isinstance(m, str) and m.casefold() in CLASSIFIER_MODES:
        return cfg
    return {k: v for k, v in cfg.items() if not k.startswith('cond_')}


def head_weight(layer):
    """The weight a ``LinearEx`` applies: its spectrally normalised override when there is one, times its equalised-lr scale."""
    from . import ops
    weight = layer.linear.weight if layer.weight_override is None else layer.weight_override
    return ops.scale(weight, layer.scale) if layer.scale != 1.0 else weight


def cond_term(critic, f, labels, params):
    """The unweighted conditioning term of a classifier-based critic on feature rows ``f`` (N, F) with their labels: a 0-dim
    device tensor.  ``params``: ``validate_loss_config``'s dict."""
    from . import ops
    m = critic.cond_mode
    if m == 'acgan':
        return ops.class_cross_entropy(critic.cls(f), labels)
    if m in ('contra', 'reacgan'):
        return ops.class_contrastive(critic.embed(f), head_weight(critic.proxy), labels, mode='2c' if m == 'contra' else 'd2d',
                                     temperature=params['temperature'], margin_pos=params['margin_pos'],
                                     margin_neg=params['margin_neg'])
    raise ValueError(f'this critic has no classifier head (cond_mode = {m!r})')


def check_host_labels(labels, num_classes, n=None):
    """Labels as a loader yields them (a CPU tensor or a sequence of ints): integral, shape (n,), all in [0, num_classes);
    raises ValueError.  -> the labels as a CPU int32 tensor, ready to be uploaded."""
    t = torch.as_tensor(labels)
    if t.is_cuda:
        raise ValueError('check_host_labels: the labels are already on the device; their range is checked on the host')
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f'class labels must be integers (got {t.dtype})')
    if t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise ValueError(f'class labels must have shape ({"N" if n is None else n},), one per sample (got {tuple(t.shape)})')
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= num_classes):
        raise ValueError(f'class labels must lie in [0, {num_classes}) (got {int(t.min())} .. {int(t.max())})')
    return t.to(torch.int32)


def check_save_format(cgan, reference_format):
    """A reference-format checkpoint has no place for the class tables, the projection or the classifier heads."""
    if cgan and reference_format:
        raise ValueError(f"cgan={cgan!r} cannot be saved with reference_format=True: the reference has neither the "
                         "conditional norm tables nor the projection layer or the classifier heads")
