"""Class conditioning for the ResNet GAN: class-conditional BatchNorm in the generator, a projection critic.

``config.cgan`` (ResNet GAN only; None = off, ``'projection'`` the only other value) with ``config.num_classes`` >= 2 is the
conditioning of SNGAN-projection (Miyato & Koyama 2018), SAGAN and BigGAN - the missing part of the recipe that
``spectral_norm``, ``loss='hinge'`` and ``self_attention`` belong to:

    generator   every BatchNorm becomes a ``ConditionalBatchNorm2d``: batch statistics as before, then the affine row of the
                sample's class from (num_classes, C) tables; the latent input stays ``len_latent`` wide, nothing is concatenated
    critic      out[n] = linear1(f)[n] + <proj.weight[l_n], f[n]> on the feature f that ``linear1`` reads; ``proj`` is a bias-free
                ``LinearEx`` (so ``spectral_norm=True`` normalises it like every other layer); the image input stays 3 channels

The networks are called as ``gen_model(z, labels)`` / ``disc_model(x, labels)`` with one int32 device label per sample
(``features(x)`` stays label-free).  The hot path is csrc/cond.hip through ``ops.cond_batch_norm`` / ``ops.class_projection``
(DESIGN.md 4.12); the projection is closed under differentiation, so the gradient penalties work, the conditional norm is first
order like the BatchNorm beside it (the generator is never inside a penalty).

This is not the reference's ``class_condition`` / ``use_auxiliary_classifier`` (one-hot concatenation, AC heads): no variant of
those runs in the reference (tests/golden/conditional_probe.json) and both keep raising NotImplementedError.
"""
import torch

CHOICES = (None, 'projection')


def validate_config(config):
    """``config.cgan`` against its values and what it needs; raises ValueError.  -> bool (is it on?)."""
    mode = getattr(config, 'cgan', None)
    if mode not in CHOICES:
        raise ValueError(f"config.cgan must be None or 'projection' (got {mode!r})")
    if mode is None:
        return False
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.cgan is a ResNet GAN option (the progressive networks have no class conditioning)')
    k = getattr(config, 'num_classes', 0)
    if not isinstance(k, int) or isinstance(k, bool) or k < 2:
        raise ValueError(f"config.cgan='projection' needs config.num_classes >= 2 (got {k!r})")
    return True


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
    """A reference-format checkpoint has no place for the class tables or the projection."""
    if cgan and reference_format:
        raise ValueError("cgan='projection' cannot be saved with reference_format=True: the reference has neither the "
                         "conditional norm tables nor the projection layer")
