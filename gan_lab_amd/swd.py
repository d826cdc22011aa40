"""Sliced Wasserstein distance (SWD) between Laplacian-pyramid patch descriptors of two image sets: the sample-quality
metric of Karras et al. 2018 ("Progressive Growing of GANs", section 5), on the GPU (csrc/swd.hip).

Per resolution level R, R/2, ..., 16 of the pyramid, ``nhoods_per_image`` 7x7x3 neighbourhoods per image are gathered at
random centres, normalised per channel over the whole set (mean, population standard deviation), projected on
``dir_repeats x dirs_per_repeat`` random unit directions, sorted per direction, and the mean absolute difference of the two
sorted sets is reported times 1e3.  The one deviation from the paper's code: images are used as given (the network's own
normalised fp32 space), not quantised to uint8 first.

A channel that is constant over a whole set at some level has zero variance: that level's SWD is NaN, as the definition
gives it (0 / 0); the other levels are unaffected.

Everything random is a pure function of ``seed``: the centres of image i at a level, and the directions of a repeat, do not
depend on how the set was fed, and the process RNG stream (latents, noise, augmentation) is never touched.
"""
import math

import torch

from . import ops, rng
from ._metric_common import device_gate, host_only_error, wanted as _wanted

DESC = ops.SWD_DESC
MIN_RES = 16
_MASK = 2 ** 64 - 1


def _substream(seed, k):
    """Philox key of sub-stream k (0: directions, 1 + level index: centres) of an evaluation seeded with ``seed``."""
    return (int(seed) * 0x9E3779B97F4A7C15 + (int(k) + 1) * 0xD1B54A32D192ED03 + 0x53574421) & _MASK


def check_res(res, what='res'):
    if not isinstance(res, int) or isinstance(res, bool) or res < MIN_RES or res & (res - 1):
        raise ValueError(f'swd: {what} must be a power of two >= {MIN_RES}, got {res!r}')
    return res


def _positive_int(v, name):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise ValueError(f'swd: {name} must be a positive integer, got {v!r}')
    return v


def check_options(nhoods_per_image, dir_repeats, dirs_per_repeat, seed, prefix=''):
    """The metric's options; ``prefix`` names them as the caller knows them (``'swd_'``: the config fields)."""
    names = ('nhoods', 'dir_repeats', 'dirs_per_repeat') if prefix else ('nhoods_per_image', 'dir_repeats', 'dirs_per_repeat')
    for v, name in zip((nhoods_per_image, dir_repeats, dirs_per_repeat), names):
        _positive_int(v, prefix + name)
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 2 ** 63:
        raise ValueError(f'swd: {prefix}seed must be an integer in [0, 2**63), got {seed!r}')


def validate_config(config):
    """Called when a learner is built: the ``swd_*`` options are checked whether or not the metric is requested, and 'swd'
    is refused among the critic's metrics (it compares image sets; the critic has no part in it)."""
    check_options(getattr(config, 'swd_nhoods', 128), getattr(config, 'swd_dir_repeats', 4),
                  getattr(config, 'swd_dirs_per_repeat', 128), getattr(config, 'swd_seed', 0), prefix='swd_')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'swd': the sliced Wasserstein distance is a generator metric "
                         "(config.gen_metrics)")


def wanted(metrics):
    return _wanted(metrics, 'swd')


def levels_of(res, min_res=MIN_RES):
    return [res >> k for k in range(int(math.log2(res // min_res)) + 1)]


def laplacian_pyramid(x, min_res=MIN_RES):
    """[lap_R, lap_R/2, ..., gauss_min_res] of an (N, 3, R, R) fp32 batch on the GPU."""
    x = ops._c(x, 'laplacian_pyramid input')
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f'laplacian_pyramid: needs an (N, C, R, R) batch, got {tuple(x.shape)}')
    check_res(int(x.shape[2]), 'the image size')
    gauss = [x]
    while gauss[-1].shape[2] > min_res:
        gauss.append(ops.swd_down(gauss[-1]))
    return [ops.swd_band(gauss[i], gauss[i + 1]) for i in range(len(gauss) - 1)] + [gauss[-1]]


def descriptors(level, positions, with_stats=False):
    """(N n, 147) descriptor rows of an (N, 3, S, S) level at the (N, n, 2) int32 centres ``positions`` ((y, x), each in
    [3, S - 4]); ``with_stats``: also the (6,) fp64 per-channel mean and population standard deviation of the rows."""
    level = ops._c(level, 'descriptors level')
    positions = ops._ct(positions, torch.int32, 'descriptors positions')
    s = level.shape[-1]
    if positions.numel() and (int(positions.min()) < 3 or int(positions.max()) > s - 4):
        raise ValueError(f'descriptors: centres must lie in [3, {s - 4}] for a {s}x{s} level')
    n_img, n = positions.shape[:2]
    desc = torch.empty((n_img * n, DESC), dtype=torch.float32, device=level.device)
    part = torch.empty((n_img, 6), dtype=torch.float64, device=level.device)
    ops.swd_gather(level, positions, desc, part)
    return (desc, ops.swd_stats(part, n * 49)) if with_stats else desc


class SlicedWasserstein(object):
    """One evaluation: ``feed_real`` / ``feed_fake`` minibatches of (k, 3, res, res) images until both sets hold
    ``n_images``, then ``result()``.  ``reset()`` starts the next evaluation in the same buffers."""

    def __init__(self, res, n_images, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0, device='cuda'):
        # every argument check comes before any allocation
        self.res = check_res(res)
        self.n_images = _positive_int(n_images, 'n_images')
        check_options(nhoods_per_image, dir_repeats, dirs_per_repeat, seed)
        self.n, self.dir_repeats, self.dirs_per_repeat, self.seed = nhoods_per_image, dir_repeats, dirs_per_repeat, seed
        self.levels = levels_of(res)
        self.m = self.n_images * self.n
        if self.dirs_per_repeat * self.m >= 2 ** 32 - 1:
            raise ValueError(f'swd: dirs_per_repeat x descriptors = {self.dirs_per_repeat} x {self.m} exceeds the sort\'s '
                             f'2^32 - 1 keys; use fewer directions per repeat or fewer images')
        self.device, self._host_only = device_gate(device, 'swd')
        self._fed = {'real': 0, 'fake': 0}
        if self._host_only:
            return
        dev = self.device
        self._desc = {k: [torch.empty((self.m, DESC), dtype=torch.float32, device=dev) for _ in self.levels]
                      for k in self._fed}
        self._part = {k: [torch.empty((self.n_images, 6), dtype=torch.float64, device=dev) for _ in self.levels]
                      for k in self._fed}
        # projections and their sorted copies of one repeat, both sets
        self._proj = [torch.empty((self.dirs_per_repeat, self.m), dtype=torch.float32, device=dev) for _ in range(4)]

    def reset(self):
        self._fed = {'real': 0, 'fake': 0}

    def feed_real(self, x):
        self._feed('real', x)

    def feed_fake(self, x):
        self._feed('fake', x)

    def positions(self, level_index, first=0, count=None):
        """(count, n, 2) int32 centres of images ``first .. first + count - 1`` at level ``level_index``: a function of the
        seed and the image's index in its set only, the same for both sets."""
        count = self.n_images - first if count is None else count
        return rng.swd_positions(count, self.n, self.levels[level_index], self.device,
                                 seed=_substream(self.seed, 1 + level_index), offset=first * ((self.n + 1) // 2))

    def directions(self, repeat):
        """(dirs_per_repeat, 147) unit directions of repeat ``repeat`` (shared by all levels and both sets)."""
        return rng.swd_directions(self.dirs_per_repeat, self.device, seed=_substream(self.seed, 0),
                                  offset=repeat * self.dirs_per_repeat * DESC)

    def _feed(self, which, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, self.res, self.res) or \
                x.dtype != torch.float32:
            raise ValueError(f'swd: a feed must be a (k, 3, {self.res}, {self.res}) float32 batch, got '
                             f'{tuple(getattr(x, "shape", ()))} {getattr(x, "dtype", type(x).__name__)}')
        k, fed = x.shape[0], self._fed[which]
        if fed + k > self.n_images:
            raise ValueError(f'swd: the {which} set was declared with {self.n_images} images; this feed of {k} would make '
                             f'{fed + k}')
        if k == 0:
            return
        if not self._host_only:
            for li, level in enumerate(laplacian_pyramid(x.detach())):
                ops.swd_gather(level, self.positions(li, fed, k), self._desc[which][li][fed * self.n:(fed + k) * self.n],
                               self._part[which][li][fed:fed + k])
        self._fed[which] = fed + k

    def result(self):
        """{'levels': [res, ..., 16], 'swd': [1e3 x distance per level], 'mean': their average}."""
        r, f = self._fed['real'], self._fed['fake']
        if r != f:
            raise ValueError(f'swd: the two sets must hold the same number of images (real {r}, fake {f})')
        if r != self.n_images:
            raise ValueError(f'swd: {self.n_images} images per set were declared, {r} were fed')
        if self._host_only:
            raise host_only_error('swd')
        d = self.dirs_per_repeat
        dists = []
        for li in range(len(self.levels)):
            stats = {k: ops.swd_stats(self._part[k][li], self.n * 49) for k in self._fed}
            for rep in range(self.dir_repeats):
                dirs = self.directions(rep)
                pr, pf, sr, sf = self._proj
                ops.swd_project(self._desc['real'][li], dirs, stats['real'], out=pr)
                ops.swd_project(self._desc['fake'][li], dirs, stats['fake'], out=pf)
                ops.swd_sort(pr, out=sr)
                ops.swd_sort(pf, out=sf)
                dists.append(ops.swd_distance(sr, sf))
        host = torch.stack(dists).cpu().tolist()          # the evaluation's one host read
        swd = [1e3 * (math.fsum(host[li * self.dir_repeats:(li + 1) * self.dir_repeats]) / self.dir_repeats)
               for li in range(len(self.levels))]
        return {'levels': list(self.levels), 'swd': swd, 'mean': math.fsum(swd) / len(swd)}
