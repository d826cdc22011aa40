"""Azimuthally averaged power spectrum of an image set and its distance between fakes and reals (Durall et al. 2020, "Watch
your Up-Convolution"; Dzanic et al. 2020; the spectrum plots of Karras et al. 2021), on the GPU (csrc/spectrum.hip).
It is the validation metric that sees frequency content: a wrong blur tap or a lossy upsample shows as a bump or a sag in the
high-frequency tail of the generator's profile long before a loss, SWD or MS-SSIM line moves.

Per (3, R, R) image, R a power of two in [16, 1024], used as given (the network's own normalised fp32 space, not quantised):
``y = x w[i] w[j]`` with the periodic Hann window ``w[i] = 0.5 - 0.5 cos(2 pi i / R)`` (``window='hann'``, the default) or
``w = 1`` (``'none'``); ``P[u, v] = 1/3 sum_c |DFT2(y_c)[u, v]|^2 / (R^2 W)``, ``W = (sum_i w[i]^2 / R)^2``, so that white noise of
variance s^2 has P ~ s^2 under either window; with signed frequencies ku, kv in [-R/2, R/2), bin k = 0 .. R/2 holds the
coefficients with ``(2k-1)^2 <= 4 (ku^2 + kv^2) < (2k+1)^2`` (the nearest integer radius, in integer arithmetic; bin 0 is DC alone,
the corners beyond R/2 are dropped) and ``A[k]`` is the mean of P over the bin.  A set's profile ``S[k]`` is the mean of ``A_n[k]``
over its images, ``dB[k] = 10 log10(max(S[k], 1e-30))``, and two sets are ``spectrum = sqrt(mean_{k=1..R/2} (dB_fake[k] -
dB_real[k])^2)`` apart (DC excluded: an overall brightness offset is normalisation, not spectrum shape) and ``hf`` = the same over
``k = R/4+1 .. R/2``, the band where upsampling artifacts live.

Nothing here is random and nothing depends on how the set was split into feeds: results are bitwise reproducible.
"""
import torch

from . import ops
from ._metric_common import device_gate, host_only_error, wanted as _wanted

MIN_RES = ops.SPECTRUM_MIN_RES
MAX_RES = ops.SPECTRUM_MAX_RES
WINDOWS = ops.SPECTRUM_WINDOWS           # name -> the kernel's code
DB_FLOOR = 1e-30                         # S[k] is clamped here before the logarithm: an all-zero set reads -300 dB
_SCRATCH_BYTES = 64 << 20                # the half spectra of one chunk of images: a feed larger than this is walked in chunks


def check_res(res, what='res'):
    if not isinstance(res, int) or isinstance(res, bool) or res < MIN_RES or res > MAX_RES or res & (res - 1):
        raise ValueError(f'spectrum: {what} must be a power of two in [{MIN_RES}, {MAX_RES}], got {res!r}')
    return res


def check_options(window, prefix=''):
    """The metric's option; ``prefix`` names it as the caller knows it (``'spectrum_'``: the config field ``spectrum_window``)."""
    if not isinstance(window, str) or window not in WINDOWS:
        raise ValueError(f"spectrum: {prefix}window must be one of {sorted(WINDOWS)}, got {window!r}")
    return window


def validate_config(config):
    """Called when a learner is built: ``spectrum_window`` is checked whether or not the metric is requested, and 'spectrum' is
    refused among the critic's metrics (it compares generated images with the validation reals; the critic has no part in it)."""
    check_options(getattr(config, 'spectrum_window', 'hann'), prefix='spectrum_')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'spectrum': the radial power-spectrum distance is a generator metric "
                         "(config.gen_metrics)")


def wanted(metrics):
    return _wanted(metrics, 'spectrum')


def bins(res):
    return res // 2 + 1


def _chunk(res, n):
    per_image = ops.spectrum_scratch_bytes(2, res) - ops.spectrum_scratch_bytes(1, res)
    return max(1, min(n, _SCRATCH_BYTES // per_image))


def _run(x, res, window, workspace, first, n_images, scratch, chunk):
    for off in range(0, x.shape[0], chunk):
        ops.spectrum_feed(x[off:off + chunk], res, window, scratch, workspace, first + off, n_images)


def profiles(x, window='hann'):
    """Per-image profiles of a (N, 3, R, R) fp32 GPU batch: an (N, R/2 + 1) fp64 device tensor.  For tests and tools: it
    allocates."""
    window = check_options(window)
    x = ops._c(x, 'spectrum.profiles x')
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f'spectrum.profiles: needs a (N, 3, R, R) batch, got {tuple(x.shape)}')
    res = check_res(int(x.shape[2]), 'the image size')
    n = int(x.shape[0])
    chunk = _chunk(res, n)
    ws = ops.spectrum_workspace(n, res, x.device)
    _run(x, res, window, ws, 0, n, ops.spectrum_scratch(chunk, res, x.device), chunk)
    return ws


class PowerSpectrum(object):
    """One evaluation: ``feed`` minibatches of (k, 3, res, res) images until the set holds ``n_images``, then ``profile()``
    (or ``distance(fake, real)``).  ``reset()`` starts the next evaluation in the same buffers."""

    def __init__(self, res, n_images, window='hann', device='cuda'):
        # every argument check comes before any allocation
        self.res = check_res(res)
        if not isinstance(n_images, int) or isinstance(n_images, bool) or n_images < 1:
            raise ValueError(f'spectrum: n_images must be a positive integer, got {n_images!r}')
        self.n_images = n_images
        self.window = check_options(window)
        self.device, self._host_only = device_gate(device, 'spectrum')
        self._fed = 0
        if self._host_only:
            return
        self._chunk = _chunk(res, n_images)
        self._ws = ops.spectrum_workspace(n_images, res, self.device)
        self._scratch = ops.spectrum_scratch(self._chunk, res, self.device)
        self._out = torch.empty(4 * bins(res) + 2, dtype=torch.float64, device=self.device)

    def reset(self):
        self._fed = 0

    def feed(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, self.res, self.res) or \
                x.dtype != torch.float32:
            raise ValueError(f'spectrum: a feed must be a (k, 3, {self.res}, {self.res}) float32 batch, got '
                             f'{tuple(getattr(x, "shape", ()))} {getattr(x, "dtype", type(x).__name__)}')
        k = x.shape[0]
        if self._fed + k > self.n_images:
            raise ValueError(f'spectrum: the set was declared with {self.n_images} images; this feed of {k} would make '
                             f'{self._fed + k}')
        if k == 0:
            return
        if not self._host_only:
            _run(ops._c(x.detach(), 'spectrum feed'), self.res, self.window, self._ws, self._fed, self.n_images, self._scratch,
                 self._chunk)
        self._fed += k

    def _complete(self):
        if self._fed != self.n_images:
            raise ValueError(f'spectrum: {self.n_images} images were declared, {self._fed} were fed')
        if self._host_only:
            raise host_only_error('spectrum')

    def profile(self):
        """{'power': [S[0] .. S[R/2]], 'db': [...]}: the set profile, with one host read."""
        self._complete()
        nb = bins(self.res)
        ops.spectrum_finish(self._ws, None, self.n_images, self.res, self._out[:2 * nb])
        host = self._out[:2 * nb].cpu().tolist()
        return {'power': host[:nb], 'db': host[nb:]}

    def per_image(self):
        """The (n_images, R/2 + 1) fp64 per-image profiles A_n[k], on the device (complete once every image is fed)."""
        self._complete()
        return self._ws


def distance(fake, real):
    """The distance of two complete evaluations of the same size: {'spectrum': RMS dB difference over k = 1 .. R/2, 'hf': the
    same over k = R/4+1 .. R/2, 'fake_db': [...], 'real_db': [...], 'images': n}, with one host read."""
    if not isinstance(fake, PowerSpectrum) or not isinstance(real, PowerSpectrum):
        raise TypeError('spectrum.distance: needs two PowerSpectrum evaluations')
    if (fake.res, fake.n_images, fake.window) != (real.res, real.n_images, real.window):
        raise ValueError(f'spectrum.distance: the two sets must share resolution, image count and window, got '
                         f'{(fake.res, fake.n_images, fake.window)} and {(real.res, real.n_images, real.window)}')
    fake._complete()
    real._complete()
    nb = bins(fake.res)
    ops.spectrum_finish(fake._ws, real._ws, fake.n_images, fake.res, fake._out)
    host = fake._out.cpu().tolist()
    return {'spectrum': host[4 * nb], 'hf': host[4 * nb + 1], 'fake_db': host[nb:2 * nb], 'real_db': host[3 * nb:4 * nb],
            'fake_power': host[:nb], 'real_power': host[2 * nb:3 * nb], 'images': fake.n_images}
