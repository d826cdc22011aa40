"""Process-wide counter-based RNG stream for latents and per-layer noise (Philox4x32-10 in HIP)."""
import torch

from . import ops

_STATE = {'seed': 0x5EED, 'offset': 0}
# While a step graph is being captured (graphs.GraphedStep) the stream position cannot be a launch argument - it would be
# frozen into the graph: draws then read a device-resident base (rewritten before every replay) and pass only their
# distance from the position the capture started at.
_DEVICE_BASE = {'block': None, 'start': 0}


def begin_device_offsets(block):
    _DEVICE_BASE['block'], _DEVICE_BASE['start'] = block, _STATE['offset']


def end_device_offsets():
    """Back to by-value offsets; returns how far the stream advanced since ``begin_device_offsets``."""
    n = _STATE['offset'] - _DEVICE_BASE['start']
    _DEVICE_BASE['block'] = None
    return n


def manual_seed(seed, rank=0):
    _STATE['seed'] = (int(seed) * 0x9E3779B97F4A7C15 + int(rank) * 0xD1B54A32D192ED03) & (2 ** 64 - 1)
    _STATE['offset'] = 0


def seed_from_config(random_seed):
    """Seed the device stream the way config.py:337-376 seeds numpy / torch: ``random_seed`` in [0, 2**32) is used as
    is, -1 draws a fresh one.  Called by the learners at construction (the process group, if any, exists by then):
    rank 0's seed is shared, then every rank mixes its own rank in, so that the replicas of a data-parallel run draw
    DIFFERENT latents and per-layer noise (an effective fake batch of B * world_size) yet a fixed ``random_seed``
    reproduces the run."""
    import os
    from . import parallel
    seed = int(random_seed) if random_seed is not None else -1
    if seed < 0:
        seed = int.from_bytes(os.urandom(7), 'little')
    if parallel.is_dist():
        import torch.distributed as dist
        box = [seed]
        dist.broadcast_object_list(box, src=0)
        seed = int(box[0])
    manual_seed(seed, parallel.rank())
    return seed


def randn(shape, device='cuda'):
    n = 1
    for s in shape:
        n *= int(s)
    if _DEVICE_BASE['block'] is not None:
        out = ops.randn_dev(tuple(shape), _STATE['seed'], _DEVICE_BASE['block'], _STATE['offset'] - _DEVICE_BASE['start'],
                            device)
    else:
        out = ops.randn(tuple(shape), _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += (n + 3) // 4
    return out


def trunc_randn(shape, threshold, device='cuda'):
    """``randn`` truncated to [-threshold, threshold] (the truncation trick; sampling.py): the same counters, so the stream
    advances exactly as ``randn`` of the same shape advances it.  Not available while a step graph is being captured."""
    threshold = ops.check_truncation(threshold)
    n = 1
    for s in shape:
        n *= int(s)
    if _DEVICE_BASE['block'] is not None:
        raise RuntimeError('rng.trunc_randn: not available while a step graph is being captured')
    out = ops.trunc_randn(tuple(shape), threshold, _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += (n + 3) // 4
    return out


def randint(n, high, device='cuda'):
    """(n,) int32 uniform in [0, high): the class labels a conditional generator step draws (conditional.py); advances the stream
    by ceil(n / 4) counters.  Not available while a step graph is being captured (the ResNet GAN steps eagerly)."""
    n = int(n)
    if _DEVICE_BASE['block'] is not None:
        raise RuntimeError('rng.randint: not available while a step graph is being captured')
    out = ops.randint(n, high, _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += (n + 3) // 4
    return out


def augment_params(n, h, w, device='cuda'):
    """(n, 8) DiffAugment parameter rows for (h, w) images (augment.py); advances the stream by 2 counters per row."""
    n = int(n)
    if _DEVICE_BASE['block'] is not None:
        out = ops.diffaug_params_dev(n, h, w, _STATE['seed'], _DEVICE_BASE['block'], _STATE['offset'] - _DEVICE_BASE['start'],
                                     device)
    else:
        out = ops.diffaug_params(n, h, w, _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += 2 * n
    return out


def cr_params(n, shift, flip, device='cuda'):
    """(n, 4) int32 rows (flip, dx, dy, 0) of the consistency-regularisation image transform (consistency.py): flip in {0, 1}
    (always 0 when ``flip`` is False), dx, dy uniform in [-shift, shift]; advances the stream by 1 counter per row, so a short
    draw is a prefix of a long one from the same position."""
    n = int(n)
    if _DEVICE_BASE['block'] is not None:
        out = ops.cr_params(n, shift, flip, _STATE['seed'], _STATE['offset'] - _DEVICE_BASE['start'], device,
                            base=_DEVICE_BASE['block'])
    else:
        out = ops.cr_params(n, shift, flip, _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += n
    return out


def ada_params(n, h, w, state, policy, device='cuda'):
    """(n, 32) ADA parameter rows for (h, w) images at the probability held in the device block ``state`` (ada.py);
    advances the stream by 8 counters per row.  A policy with a filter, noise or cutout group returns an ``ops.AdaDraw``
    instead: the same rows, the (n, 16) ext rows from the next 4 counters per row and, with noise, the (n, 3, h, w) field
    ``randn`` draws right after them - all consumed whatever the gates say, since p lives on the device."""
    n = int(n)
    if _DEVICE_BASE['block'] is not None:
        out = ops.ada_params_dev(n, h, w, state, policy & ~ops.ADA_NEW_GROUPS, _STATE['seed'], _DEVICE_BASE['block'],
                                 _STATE['offset'] - _DEVICE_BASE['start'], device)
    else:
        out = ops.ada_params(n, h, w, state, policy & ~ops.ADA_NEW_GROUPS, _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += ops.ADA_COUNTERS * n
    if not policy & ops.ADA_NEW_GROUPS:
        return out
    if _DEVICE_BASE['block'] is not None:
        ext = ops.ada_ext_params_dev(n, h, w, state, policy, _STATE['seed'], _DEVICE_BASE['block'],
                                     _STATE['offset'] - _DEVICE_BASE['start'], device)
    else:
        ext = ops.ada_ext_params(n, h, w, state, policy, _STATE['seed'], _STATE['offset'], device)
    _STATE['offset'] += ops.ADA_EXT_COUNTERS * n
    noise = randn((n, 3, int(h), int(w)), device) if policy & ops.ADA_NOISE else None
    return ops.AdaDraw(out, ext, noise)


def swd_positions(n_images, n_per_image, size, device='cuda', seed=None, offset=None):
    """(n_images, n_per_image, 2) int32 patch centres uniform in [3, size - 4] for the sliced Wasserstein metric (swd.py);
    ceil(n_per_image / 2) counters per image.  By default drawn from, and advancing, the process stream; with an explicit
    ``seed`` / ``offset`` the draw is a pure function of them and the process stream is left alone - an evaluation uses the
    same centres for the real and the fake set, and must not move the training stream."""
    n_images, per = int(n_images), (int(n_per_image) + 1) // 2
    if seed is None and offset is None:
        if _DEVICE_BASE['block'] is not None:
            raise RuntimeError('rng.swd_positions: not available while a step graph is being captured')
        out = ops.swd_positions(n_images, n_per_image, size, _STATE['seed'], _STATE['offset'], device)
        _STATE['offset'] += per * n_images
        return out
    return ops.swd_positions(n_images, n_per_image, size, _STATE['seed'] if seed is None else seed, offset or 0, device)


def swd_directions(n_dirs, device='cuda', seed=None, offset=None):
    """(n_dirs, 147) unit-norm Gaussian projection directions (swd.py); 147 counters per direction.  ``seed`` / ``offset``
    as in ``swd_positions``."""
    n_dirs = int(n_dirs)
    if seed is None and offset is None:
        if _DEVICE_BASE['block'] is not None:
            raise RuntimeError('rng.swd_directions: not available while a step graph is being captured')
        out = ops.swd_directions(n_dirs, _STATE['seed'], _STATE['offset'], device)
        _STATE['offset'] += ops.SWD_DESC * n_dirs
        return out
    return ops.swd_directions(n_dirs, _STATE['seed'] if seed is None else seed, offset or 0, device)
