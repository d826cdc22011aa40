"""SAGAN self-attention for the ResNet GAN (Zhang et al. 2019; the layer BigGAN kept).

``config.self_attention`` (ResNet GAN only; None = off, ``'g'``, ``'d'`` or ``'gd'``) adds one ``SelfAttention2d`` block to
the generator and / or the critic, at SAGAN's positions (resnetgan/architectures.py).  For an (N, C, H, W) map ``x``

    q = theta(x)                  (N, C/8, HW)       1x1 convolutions without bias
    k = maxpool2x2(phi(x))        (N, C/8, HW/4)
    v = maxpool2x2(g(x))          (N, C/2, HW/4)
    a = softmax_s(q^T k) v        (N, C/2, HW)       no 1/sqrt(d) scale
    out = x + gamma * o(a)        gamma a learned scalar that starts at 0: a new block is the identity

The 1x1 convolutions are ordinary ``Conv2dEx`` layers (so ``spectral_norm=True`` normalises the critic's four like any other
layer; ``gamma`` is not normalised); the core ``ops.attention`` is one fused flash-style kernel on the exact-fp32 MFMA and never
materialises the (HW, HW/4) map (csrc/attention.hip).  Everything is first order: a gradient penalty's double
backward through a critic with attention is not provided, so ``'d'`` requires ``gradient_penalty=None`` (hinge loss + spectral
normalisation is the SAGAN recipe); ``'g'`` works with every loss and penalty, the penalties never differentiate through the
generator.
"""
import torch
from torch import nn

from . import ops
from .utils.custom_layers import Conv2dEx

CHOICES = (None, 'g', 'd', 'gd')
NI_MIN, NI_MAX, NI_MULTIPLE = 32, 512, 32


def validate_config(config):
    """``config.self_attention`` against its values and the options it excludes; raises ValueError.
    -> (generator has a block, critic has a block)."""
    sa = getattr(config, 'self_attention', None)
    if sa not in CHOICES:
        raise ValueError(f"config.self_attention must be one of None, 'g', 'd', 'gd' (got {sa!r})")
    if sa is None:
        return False, False
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.self_attention is a ResNet GAN option (the progressive networks have no attention block)')
    if 'd' in sa and getattr(config, 'gradient_penalty', None) is not None:
        raise ValueError(f"config.self_attention={sa!r} puts an attention block into the critic, and the double backward of "
                         f"a gradient penalty (config.gradient_penalty={config.gradient_penalty!r}) through attention is not "
                         f"provided: train it with loss='hinge', spectral_norm=True and gradient_penalty=None")
    return 'g' in sa, 'd' in sa


def check_save_format(self_attention, reference_format):
    """A reference-format checkpoint has no place for the block (the reference has no attention)."""
    if self_attention and reference_format:
        raise ValueError('self_attention cannot be saved with reference_format=True: the reference has no attention block '
                         '(the self_attn.* parameters would be dropped)')


class SelfAttention2d(nn.Module):
    """The SAGAN block on an (N, ni, H, W) map, H and W even.  ``ni`` a multiple of 32 in [32, 512]: the core then runs with
    Dk = ni / 8 in [4, 64] and Dv = ni / 2 in [16, 256], the range of the fused kernel."""

    def __init__(self, ni, equalized_lr=False):
        super().__init__()
        if not isinstance(ni, int) or ni % NI_MULTIPLE or not NI_MIN <= ni <= NI_MAX:
            raise ValueError(f'SelfAttention2d: ni must be a multiple of {NI_MULTIPLE} in [{NI_MIN}, {NI_MAX}] (got {ni!r})')
        self.ni = ni
        kw = dict(ks=1, include_bias=False, equalized_lr=equalized_lr)
        self.theta = Conv2dEx(ni, ni // 8, **kw)
        self.phi = Conv2dEx(ni, ni // 8, **kw)
        self.g = Conv2dEx(ni, ni // 2, **kw)
        self.o = Conv2dEx(ni // 2, ni, **kw)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        q = self.theta(x)
        k = ops.max_pool2x2(self.phi(x))
        v = ops.max_pool2x2(self.g(x))
        return ops.gated_residual(x, self.o(ops.attention(q, k, v)), self.gamma)
