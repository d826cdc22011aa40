"""BigGAN's orthogonal regularisation (Brock et al. 2019, eq. 3) of a ResNet GAN network, batched over all of its layers.

``config.ortho_reg = beta`` (generator) / ``config.ortho_reg_d = beta`` (critic); ResNet GAN only, default 0 = off: nothing is
built, nothing is launched.  For every ``Conv2dEx`` / ``LinearEx`` weight ``W`` of the network (the 3x3 convolutions, the 1x1
skips, self-attention's 1x1 convolutions, the first linear, the critic's ``proj``), viewed as ``Wm = W.reshape(Cout, -1)``,

    R_beta(W) = beta * || (Wm Wm^T) o (1 - I) ||_F^2          M = (Wm Wm^T) o (1 - I)
    d R_beta / d W = 4 * beta * M Wm

and the learner ADDS that gradient to the parameter's slot of the gradient arena after the all-reduce and before the
optimiser step (every rank adds the same rank-independent term, so data parallelism needs nothing more).  The parameter is not
touched.  The gradient is the true derivative of the penalty as the paper writes it; BigGAN-PyTorch's ``ortho()`` applies
``2 * strength * M Wm`` - HALF of this for the same number - so ``ortho_reg = s / 2`` reproduces a BigGAN-PyTorch run with
strength ``s`` (its 1e-4 is ``ortho_reg = 5e-5`` here; the paper's beta = 1e-4 is ``ortho_reg = 1e-4``).

Left alone, as in BigGAN: BatchNorm / LayerNorm affines, the (num_classes, C) conditional-BatchNorm tables (BigGAN exempts its
embedding likewise), biases and attention's ``gamma``.  The regulariser works on the STORED parameter: with
``use_equalized_lr`` the unscaled one, with ``spectral_norm`` the raw ``W`` and not ``W / sigma``.

Where it runs: the layers compute nothing.  The manager below owns one device-resident job table over the parameter arena
(``ops.OrthoTable``) and ``apply()`` is three launches whatever the number of layers (csrc/ortho.hip): both chained products
per layer run on the fp32 matrix cores through the association with the smaller middle dimension, so the (Cout, Cout) matrix
of the generator's first linear is never formed.  No atomics, bitwise reproducible, nothing is read back by the host.  The
regulariser has no state: checkpoints keep their layout.
"""
import math
import numbers

from . import ops
from .spectral_norm import normalised_layers

regularised_layers = normalised_layers      # [(prefix, container module, holder of .weight)]: every Conv2dEx / LinearEx


def _strength(config, name):
    v = getattr(config, name, 0.)
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f'config.{name} must be a real number >= 0 (got {v!r})')
    if not math.isfinite(v) or v < 0:
        raise ValueError(f'config.{name} must be a finite number >= 0 (got {v!r})')
    return float(v)


def validate_config(config):
    """``config.ortho_reg`` / ``config.ortho_reg_d``; raises ValueError.  -> (generator strength, critic strength)."""
    g, d = _strength(config, 'ortho_reg'), _strength(config, 'ortho_reg_d')
    if (g or d) and getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.ortho_reg / config.ortho_reg_d are ResNet GAN options')
    return g, d


class OrthoReg(object):
    """``reg = OrthoReg(model, arena, beta)``: regularises every Conv2dEx / LinearEx weight of ``model``, whose parameters live
    in ``arena`` (an ``optim.ParamArena``)."""

    def __init__(self, model, arena, beta):
        beta = float(beta)
        if not math.isfinite(beta) or beta < 0:
            raise ValueError(f'OrthoReg: beta must be a finite number >= 0 (got {beta!r})')
        layers = regularised_layers(model)
        if not layers:
            raise ValueError('OrthoReg: the model has no Conv2dEx / LinearEx layer')
        self.model, self.arena, self.beta = model, arena, beta
        self.names, self.shapes, jobs = [], [], []
        for prefix, _, holder in layers:
            p = holder.weight
            if getattr(p, '_ganlab_arena', None) is not arena:
                raise ValueError(f'OrthoReg: {prefix}.weight does not live in the given arena')
            self.names.append(prefix + '.weight')
            self.shapes.append((p.shape[0], p.numel() // p.shape[0]))
            jobs.append(dict(w=p.data, gw=p.grad))
        self.table = ops.OrthoTable(jobs)

    def _check_attached(self):
        if not self.arena.is_attached():
            raise RuntimeError('OrthoReg: the model\'s parameters left their arena (the job table points into it); rebuild the '
                               'arena and the manager')

    def apply(self):
        """Adds 4 beta M Wm to every regularised parameter's gradient slot and refreshes the penalties."""
        self._check_attached()
        ops.ortho_apply(self.table, self.beta)

    @property
    def penalty(self):
        """beta * sum over the layers, as of the last ``apply()``: a 1-element device tensor."""
        return self.table.total

    def per_layer(self):
        """{parameter key: that layer's beta * sum(M^2) (a 1-element device tensor)}."""
        return {k: self.table.penalties[i:i + 1] for i, k in enumerate(self.names)}

    @staticmethod
    def validate_config(config):
        return validate_config(config)
