"""Multi-scale structural similarity (MS-SSIM; Wang, Simoncelli and Bovik 2003) between pairs of images of one set: the
sample-diversity metric of Karras et al. 2018 ("Progressive Growing of GANs", section 5), on the GPU (csrc/msssim.hip; DESIGN.md
4.8).  Lower means more diverse; a generator that has collapsed onto a few modes scores near 1 whatever its SWD says.

Pairs are images (2j, 2j + 1) of the set, in the order they were fed.  At each of five levels (side R, R/2, ..., R/16) the two
images' local means, variances and covariance under a Gaussian window (11 taps, sigma 1.5; min(11, S) taps and sigma 1.5 s / 11
where the side S is below 11; valid mode) give a contrast-structure term cs and the full ssim per pixel and channel; their means
CS_i and SSIM_i are clamped below at 0, the next level is the 2 x 2 mean, and a pair scores prod_{i<4} CS_i^w_i x SSIM_4^w_4.
The one deviation from the paper's code is SWD's: images are used as given (the network's own normalised fp32 space), not
quantised to uint8, so the dynamic range L of C1 = (0.01 L)^2, C2 = (0.03 L)^2 is an option (``data_range``, default 2).

Nothing here is random and nothing depends on how the set was split into feeds: results are bitwise reproducible.
"""
import math

import torch

from . import ops
from ._metric_common import device_gate, host_only_error, wanted as _wanted

MIN_RES = 16                         # five levels need R / 16 >= 1
LEVELS = ops.MSSSIM_LEVELS
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_SCRATCH_BYTES = 64 << 20            # the pooled levels of one chunk of pairs: a feed larger than this is walked in chunks


def check_res(res, what='res'):
    if not isinstance(res, int) or isinstance(res, bool) or res < MIN_RES or res & (res - 1):
        raise ValueError(f'msssim: {what} must be a power of two >= {MIN_RES}, got {res!r}')
    return res


def check_options(data_range, prefix=''):
    """The metric's option; ``prefix`` names it as the caller knows it (``'msssim_'``: the config field ``msssim_range``)."""
    name = prefix + 'range' if prefix else 'data_range'
    if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not math.isfinite(data_range) or \
            data_range <= 0:
        raise ValueError(f'msssim: {name} must be a finite number > 0, got {data_range!r}')
    return float(data_range)


def validate_config(config):
    """Called when a learner is built: ``msssim_range`` is checked whether or not the metric is requested, and 'msssim' is
    refused among the critic's metrics (it compares generated images with each other; the critic has no part in it)."""
    check_options(getattr(config, 'msssim_range', 2.0), prefix='msssim_')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'msssim': multi-scale structural similarity is a generator metric "
                         "(config.gen_metrics)")


def wanted(metrics):
    return _wanted(metrics, 'msssim')


def constants(data_range):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def _pooled_buffers(n_pairs, res, device):
    """Levels 1..4 of ``n_pairs`` pairs, images interleaved (a of pair j at 2j, b at 2j + 1) like a fed batch."""
    return [torch.empty((2 * n_pairs, 3, res >> i, res >> i), dtype=torch.float32, device=device) for i in range(1, LEVELS)]


def _run_levels(a, b, res, c1, c2, workspace, first, n_pairs, pooled):
    """All five levels of the pairs (a[j], b[j]), which are pairs ``first ..`` of an evaluation of ``n_pairs``."""
    k = a.shape[0]
    for level in range(LEVELS):
        na = nb = None
        if level + 1 < LEVELS:
            nxt = pooled[level][:2 * k]
            na, nb = nxt[0::2], nxt[1::2]
        ops.msssim_level(a, b, level, res, c1, c2, workspace, first, n_pairs, na, nb)
        a, b = na, nb


def pairs(a, b, data_range=2.0, return_levels=False):
    """Per-pair MS-SSIM of two (P, 3, R, R) fp32 GPU batches: ((P,) fp64 values, (P, 5, 2) fp64 table of (CS_i, SSIM_i)); with
    ``return_levels`` also the pooled levels 1..4 the kernels wrote, as [(a_i, b_i)].  For tests and tools: it allocates."""
    data_range = check_options(data_range)
    a, b = ops._c(a, 'msssim.pairs a'), ops._c(b, 'msssim.pairs b')
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1 or a.shape[1] != 3 or a.shape[2] != a.shape[3]:
        raise ValueError(f'msssim.pairs: needs two equal (P, 3, R, R) batches, got {tuple(a.shape)} and {tuple(b.shape)}')
    res = check_res(int(a.shape[2]), 'the image size')
    n = int(a.shape[0])
    ws = ops.msssim_workspace(n, res, a.device)
    pooled = _pooled_buffers(n, res, a.device)
    table = torch.empty((n, LEVELS, 2), dtype=torch.float64, device=a.device)
    values = torch.empty(n, dtype=torch.float64, device=a.device)
    out = torch.empty(6, dtype=torch.float64, device=a.device)
    c1, c2 = constants(data_range)
    _run_levels(a, b, res, c1, c2, ws, 0, n, pooled)
    ops.msssim_finish(ws, n, res, table, values, out)
    if return_levels:
        return values, table, [(p[0::2], p[1::2]) for p in pooled]
    return values, table


class MultiScaleSSIM(object):
    """One evaluation: ``feed`` minibatches of (k, 3, res, res) images, k even, until the set holds ``n_images``, then
    ``result()``.  ``reset()`` starts the next evaluation in the same buffers."""

    def __init__(self, res, n_images, data_range=2.0, device='cuda'):
        # every argument check comes before any allocation
        self.res = check_res(res)
        if not isinstance(n_images, int) or isinstance(n_images, bool) or n_images < 2 or n_images % 2:
            raise ValueError(f'msssim: n_images must be a positive even integer (images are scored in pairs), got {n_images!r}')
        self.n_images, self.n_pairs = n_images, n_images // 2
        self.data_range = check_options(data_range)
        self.c1, self.c2 = constants(self.data_range)
        self.device, self._host_only = device_gate(device, 'msssim')
        self._fed = 0
        if self._host_only:
            return
        dev = self.device
        per_pair = sum(2 * 3 * (res >> i) ** 2 * 4 for i in range(1, LEVELS))
        self._chunk = max(1, min(self.n_pairs, _SCRATCH_BYTES // per_pair))
        self._ws = ops.msssim_workspace(self.n_pairs, res, dev)
        self._pooled = _pooled_buffers(self._chunk, res, dev)
        self._table = torch.empty((self.n_pairs, LEVELS, 2), dtype=torch.float64, device=dev)
        self._values = torch.empty(self.n_pairs, dtype=torch.float64, device=dev)
        self._out = torch.empty(6, dtype=torch.float64, device=dev)

    def reset(self):
        self._fed = 0

    def feed(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, self.res, self.res) or \
                x.dtype != torch.float32:
            raise ValueError(f'msssim: a feed must be a (k, 3, {self.res}, {self.res}) float32 batch, got '
                             f'{tuple(getattr(x, "shape", ()))} {getattr(x, "dtype", type(x).__name__)}')
        k = x.shape[0]
        if k % 2:
            raise ValueError(f'msssim: a feed must hold an even number of images (pairs never straddle feeds), got {k}')
        if self._fed + k > self.n_images:
            raise ValueError(f'msssim: the set was declared with {self.n_images} images; this feed of {k} would make '
                             f'{self._fed + k}')
        if k == 0:
            return
        if not self._host_only:
            x = ops._c(x.detach(), 'msssim feed')
            for off in range(0, k // 2, self._chunk):
                n = min(self._chunk, k // 2 - off)
                _run_levels(x[2 * off:2 * (off + n):2], x[2 * off + 1:2 * (off + n):2], self.res, self.c1, self.c2, self._ws,
                            self._fed // 2 + off, self.n_pairs, self._pooled)
        self._fed += k

    def result(self):
        """{'msssim': mean over pairs, 'pairs': n, 'per_level': [[mean CS_0..3], mean SSIM_4]}."""
        if self._fed != self.n_images:
            raise ValueError(f'msssim: {self.n_images} images were declared, {self._fed} were fed')
        if self._host_only:
            raise host_only_error('msssim')
        ops.msssim_finish(self._ws, self.n_pairs, self.res, self._table, self._values, self._out)
        host = self._out.cpu().tolist()               # the evaluation's one host read
        return {'msssim': host[0], 'pairs': self.n_pairs, 'per_level': [host[1:LEVELS], host[LEVELS]]}

    def per_pair(self):
        """After ``result()``: the (pairs,) values and the (pairs, 5, 2) table, on the device."""
        return self._values, self._table
