"""DiffAugment (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training", NeurIPS 2020): the same random,
differentiable transform of the critic's inputs, real and generated, in every critic pass of the D and the G step.

A policy is a comma-separated subset of ``color``, ``translation``, ``cutout``, in that order and each at most once; the
parts apply in that order.  The kernels are csrc/augment.hip (DESIGN.md "DiffAugment"); the parameters of a batch are
(N, 8) rows drawn from the device Philox stream (``rng.augment_params``)."""
from . import ops, rng

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
PARTS = (('color', COLOR), ('translation', TRANSLATION), ('cutout', CUTOUT))


def parse_policy(policy):
    """'color,translation,cutout' -> bit mask.  Any other spelling, a repeated part or a part out of order raises
    ValueError."""
    if not isinstance(policy, str):
        raise ValueError(f'DiffAugment policy must be a string such as "color,translation,cutout", got {policy!r}')
    names = [name for name, _ in PARTS]
    mask, last = 0, -1
    for part in policy.split(','):
        if part not in names:
            raise ValueError(f'DiffAugment policy {policy!r}: unknown part {part!r} (parts: {", ".join(names)})')
        k = names.index(part)
        if k <= last:
            raise ValueError(f'DiffAugment policy {policy!r}: parts must appear at most once, in the order '
                             f'{",".join(names)}')
        mask |= PARTS[k][1]
        last = k
    return mask


def sizes(h, w):
    """(sh, sw, ch, cw): the translation bounds and the cutout size of an h x w image (int(0.125 h + 0.5), int(0.5 h + 0.5))."""
    return (h + 4) // 8, (w + 4) // 8, (h + 1) // 2, (w + 1) // 2


class DiffAugment(object):
    """``aug = DiffAugment('color,translation,cutout'); y = aug(x)`` - draws fresh parameters unless ``params`` is given."""

    def __init__(self, policy):
        self.policy = policy
        self.mask = parse_policy(policy)

    def draw(self, n, h, w, device='cuda'):
        return rng.augment_params(n, h, w, device)

    def __call__(self, x, params=None):
        if params is None:
            params = self.draw(x.shape[0], x.shape[2], x.shape[3], x.device)
        return ops.diff_augment(x, params, self.mask)

    def __repr__(self):
        return f'DiffAugment({self.policy!r})'


def from_config(policy):
    """The learners' augmentation: None (off) or a validated ``DiffAugment``."""
    return None if policy is None else DiffAugment(policy)
