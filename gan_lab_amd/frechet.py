"""The Frechet distance between two sets of feature rows (Dowson & Landau 1982; Heusel et al. 2017: FID when the rows are
Inception pool features), with the moments streamed on the GPU (csrc/frechet.hip).

  fd = |mu_r - mu_f|^2 + tr(C_r) + tr(C_f) - 2 tr (C_r C_f)^(1/2)

``Frechet`` keeps, per set, a pivot c (fp32), n, ``sum = sum_i (x_i - c)`` and ``gram = sum_i (x_i - c)(x_i - c)^T`` in float64 -
nothing else is stored, feeds may have any number of rows.  The pivot is the fp32 mean of the set's first feed: rows with a large
common offset (images are not centred) then do not cancel catastrophically in ``cov = (gram - sum sum^T / n) / (n - 1)``.
``distance`` is the closed form, in plain float64 torch and solved on the host: it is O(D^3) once per validation, LAPACK's
``eigh`` is what every FID implementation uses, and it runs (and is tested) without a GPU.  What the rows are is the caller's
choice: the learners feed ``prdc.features`` (the image reduced by 2x2 means); a user with an embedding of their own feeds its rows.
"""
import torch

from . import ops, prdc
from ._metric_common import check_rows, device_gate, host_only_error, wanted as _wanted

MAX_DIM = ops.MOMENTS_MAX_DIM


def wanted(metrics):
    return _wanted(metrics, 'fd')


def validate_config(config):
    """Called when a learner is built: ``fd_res`` is checked whether or not the metric is requested, and 'fd' is refused among the
    critic's metrics (it compares image sets; the critic has no part in it).  Returns the resolution."""
    res = prdc.check_res(getattr(config, 'fd_res', 16), 'fd_res', prefix='frechet')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'fd': the Frechet distance is a generator metric (config.gen_metrics)")
    return res


def distance(mean_r, cov_r, mean_f, cov_f):
    """{'fd', 'mean_term', 'trace_term'} of two Gaussians, float64 on the host.  With ``cov_r = U L U^T`` (``L`` clamped at 0) and
    ``A = L^(1/2) U^T cov_f U L^(1/2)`` (symmetrised), ``tr (cov_r cov_f)^(1/2) = sum sqrt(max(eigvalsh(A), 0))``: two symmetric
    eigenproblems, stable for rank-deficient covariances (fewer rows than columns), where a general matrix square root is not."""
    mean_r, cov_r, mean_f, cov_f = (torch.as_tensor(t).detach().to(device='cpu', dtype=torch.float64)
                                    for t in (mean_r, cov_r, mean_f, cov_f))
    d = mean_r.numel()
    if mean_r.dim() != 1 or d < 1 or tuple(mean_f.shape) != (d,) or tuple(cov_r.shape) != (d, d) or tuple(cov_f.shape) != (d, d):
        raise ValueError(f'frechet: distance needs (D,) means and (D, D) covariances of one width, got {tuple(mean_r.shape)}, '
                         f'{tuple(cov_r.shape)}, {tuple(mean_f.shape)}, {tuple(cov_f.shape)}')
    lam, u = torch.linalg.eigh(cov_r)
    root = lam.clamp_min(0).sqrt()
    a = (u * root).T @ cov_f @ (u * root)
    a = 0.5 * (a + a.T)
    cross = torch.linalg.eigvalsh(a).clamp_min(0).sqrt().sum()
    diff = mean_r - mean_f
    mean_term = float(diff @ diff)
    trace_term = float(torch.trace(cov_r) + torch.trace(cov_f) - 2.0 * cross)
    return {'fd': mean_term + trace_term, 'mean_term': mean_term, 'trace_term': trace_term}


class Frechet(object):
    """One evaluation: ``feed_real`` / ``feed_fake`` minibatches of (n, dim) fp32 rows, any number of them, then ``result()``.
    ``reset()`` starts the next evaluation in the same accumulators.  ``pivot``: a (dim,) fp32 tensor used for both sets instead of
    each set's first-feed mean (tests)."""

    def __init__(self, dim, device='cuda', pivot=None):
        # every argument check comes before any allocation
        if not isinstance(dim, int) or isinstance(dim, bool) or not 1 <= dim <= MAX_DIM:
            raise ValueError(f'frechet: dim must be an integer in [1, {MAX_DIM}], got {dim!r}')
        self.dim = dim
        self.device, self._host_only = device_gate(device, 'frechet')
        if pivot is not None and (not isinstance(pivot, torch.Tensor) or tuple(pivot.shape) != (dim,) or
                                  pivot.dtype != torch.float32):
            raise ValueError(f'frechet: pivot must be a ({dim},) float32 tensor, got {tuple(getattr(pivot, "shape", ()))} '
                             f'{getattr(pivot, "dtype", type(pivot).__name__)}')
        self._fixed_pivot = pivot
        self._n = {'real': 0, 'fake': 0}
        if self._host_only:
            return
        dev = self.device
        self._pivot = {w: torch.zeros(dim, dtype=torch.float32, device=dev) for w in self._n}
        self._sum = {w: torch.zeros(dim, dtype=torch.float64, device=dev) for w in self._n}
        self._gram = {w: torch.zeros(dim, dim, dtype=torch.float64, device=dev) for w in self._n}

    def reset(self):
        self._n = {'real': 0, 'fake': 0}
        if not self._host_only:
            for w in self._n:
                self._sum[w].zero_()
                self._gram[w].zero_()

    def feed_real(self, rows):
        self._feed('real', rows)

    def feed_fake(self, rows):
        self._feed('fake', rows)

    def _feed(self, which, rows):
        check_rows(rows, self.dim, 'frechet')
        n = rows.shape[0]
        if n == 0:
            return
        if not self._host_only:
            rows = ops._c(rows.detach(), f'frechet {which} rows')
            if self._n[which] == 0:
                self._pivot[which].copy_(rows.mean(dim=0) if self._fixed_pivot is None else self._fixed_pivot)
            ops.moments_accum(rows, self._pivot[which], self._sum[which], self._gram[which])
        self._n[which] += n

    def _check(self, which):
        if which not in self._n:
            raise ValueError(f"frechet: which must be 'real' or 'fake', got {which!r}")
        if self._host_only:
            raise host_only_error('frechet')

    def raw(self, which):
        """(n, pivot fp32 (dim,), sum float64 (dim,), gram float64 (dim, dim)) of the 'real' or 'fake' set: copies."""
        self._check(which)
        return self._n[which], self._pivot[which].clone(), self._sum[which].clone(), self._gram[which].clone()

    def moments(self, which):
        """(mean (dim,), cov (dim, dim)) of the 'real' or 'fake' set, float64 on the device; the covariance has the n - 1
        denominator (numpy.cov, pytorch-fid) and needs at least 2 rows."""
        n = self._n.get(which, 0)
        if which in self._n and n < 2:
            raise ValueError(f'frechet: the covariance needs at least 2 {which} rows, {n} were fed')
        self._check(which)
        s, g = self._sum[which], self._gram[which]
        return self._pivot[which].double() + s / n, (g - torch.outer(s, s) / n) / (n - 1)

    def result(self):
        """{'fd', 'mean_term', 'trace_term', 'n_real', 'n_fake'}: the moments are formed on the device, the distance is solved on
        the host (``distance``)."""
        for which in ('real', 'fake'):
            if self._n[which] < 2:
                raise ValueError(f'frechet: the covariance needs at least 2 {which} rows, {self._n[which]} were fed')
        (mean_r, cov_r), (mean_f, cov_f) = self.moments('real'), self.moments('fake')
        out = distance(mean_r, cov_r, mean_f, cov_f)
        out.update(n_real=self._n['real'], n_fake=self._n['fake'])
        return out
