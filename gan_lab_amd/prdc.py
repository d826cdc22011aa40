"""Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) between two sets of
feature rows, on the GPU (csrc/prdc.hip): the four numbers that separate fidelity from diversity without a
pretrained network.

Real rows are r_i (N of them), generated rows g_j (M of them), fp32 of one width.  Everything compares SQUARED Euclidean distances
and ``<=`` counts as inside.  ``rad_r[i]`` is the k-th smallest |r_i - r_i'|^2 over i' != i (the row itself is excluded by index,
a duplicate at another index counts), ``rad_g[j]`` the same within the generated set.

  precision = share of j with some i such that |g_j - r_i|^2 <= rad_r[i]      (the generated row lies in the reals' manifold)
  recall    = share of i with some j such that |r_i - g_j|^2 <= rad_g[j]      (the real row lies in the fakes' manifold)
  density   = #{(j, i): |g_j - r_i|^2 <= rad_r[i]} / (k M)                    (how many real balls hold a generated row)
  coverage  = share of i with min_j |r_i - g_j|^2 <= rad_r[i]                 (real balls that hold some generated row)

Two k-NN passes (one per set) and three passes of one set against the other give everything, the nearest real of every
generated row included; no N x M matrix is ever stored.  What the rows are is the caller's choice: ``features`` gives the
learners' default, the image itself reduced by 2x2 means - at 32 / 64 pixels a reasonable feature row (Naeem et al. find the
numbers useful away from ImageNet embeddings) - and a user with an embedding of their own feeds its rows.
"""
import torch

from . import ops
from ._metric_common import check_rows, device_gate, host_only_error, wanted as _wanted

MAX_K = ops.PRDC_MAX_K
MIN_RES = 4


def check_k(k, what='k'):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f'prdc: {what} must be an integer in [1, {MAX_K}], got {k!r}')
    return k


def check_res(res, what='res', prefix='prdc'):
    if not isinstance(res, int) or isinstance(res, bool) or res < MIN_RES or res & (res - 1):
        raise ValueError(f'{prefix}: {what} must be a power of two >= {MIN_RES}, got {res!r}')
    return res


def _positive_int(v, name):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise ValueError(f'prdc: {name} must be a positive integer, got {v!r}')
    return v


def wanted(metrics):
    return _wanted(metrics, 'prdc')


def validate_config(config):
    """Called when a learner is built: ``prdc_k`` / ``prdc_res`` are checked whether or not the metric is requested, and 'prdc'
    is refused among the critic's metrics (it compares image sets; the critic has no part in it).  Returns (k, res)."""
    k = check_k(getattr(config, 'prdc_k', 5), 'prdc_k')
    res = check_res(getattr(config, 'prdc_res', 32), 'prdc_res')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'prdc': precision / recall / density / coverage is a generator metric "
                         "(config.gen_metrics)")
    return k, res


def feature_dim(channels, img_res, res):
    """Width of ``features`` rows for (channels, img_res, img_res) images."""
    r = int(img_res)
    while r > res:
        r //= 2
    return int(channels) * r * r


def features(x, res):
    """(n, C R' R') rows of an (n, C, R, R) fp32 batch on the GPU: 2x2 means until R' <= ``res``, then flattened."""
    check_res(res)
    x = ops._c(x, 'prdc features input')
    if x.dim() != 4 or x.shape[2] != x.shape[3] or x.shape[2] & (x.shape[2] - 1):
        raise ValueError(f'prdc: features needs an (n, C, R, R) batch with R a power of two, got {tuple(x.shape)}')
    x = x.detach()
    while x.shape[2] > res:
        x = ops.k_pool2(x)
    return x.reshape(x.shape[0], -1)


class PRDC(object):
    """One evaluation: ``feed_real`` / ``feed_fake`` minibatches of (n, dim) fp32 rows until the sets hold ``n_real`` and
    ``n_fake`` rows, then ``result()`` and ``nearest_real()``.  ``reset()`` starts the next evaluation in the same buffers."""

    def __init__(self, dim, n_real, n_fake, k=5, device='cuda'):
        # every argument check comes before any allocation
        self.dim = _positive_int(dim, 'dim')
        self.n = {'real': _positive_int(n_real, 'n_real'), 'fake': _positive_int(n_fake, 'n_fake')}
        self.k = check_k(k)
        for which, n in self.n.items():
            if self.k >= n:
                raise ValueError(f'prdc: k must be below the size of both sets (k = {self.k}, n_{which} = {n}): the k-th '
                                 f'neighbour of a row is sought among the other rows of its set')
        self.device, self._host_only = device_gate(device, 'prdc')
        self._fed = {'real': 0, 'fake': 0}
        self._done = False
        if self._host_only:
            return
        dev = self.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        self._rows = {w: f32(n, self.dim) for w, n in self.n.items()}
        self._norms = {w: f32(n) for w, n in self.n.items()}
        self._knn = {w: f32(n, self.k) for w, n in self.n.items()}
        self._rad = {w: f32(n) for w, n in self.n.items()}
        # (count, smallest squared distance, its index) of the three passes of one set against the other
        self._pass = {'fake_in_real': (i32(n_fake), f32(n_fake), i32(n_fake)),
                      'real_in_fake': (i32(n_real), f32(n_real), i32(n_real)),
                      'real_covered': (i32(n_real), f32(n_real), i32(n_real))}

    def reset(self):
        self._fed = {'real': 0, 'fake': 0}
        self._done = False

    def feed_real(self, rows):
        self._feed('real', rows)

    def feed_fake(self, rows):
        self._feed('fake', rows)

    def _feed(self, which, rows):
        check_rows(rows, self.dim, 'prdc')
        n, fed = rows.shape[0], self._fed[which]
        if fed + n > self.n[which]:
            raise ValueError(f'prdc: the {which} set was declared with {self.n[which]} rows; this feed of {n} would make '
                             f'{fed + n}')
        if n == 0:
            return
        if not self._host_only:
            dst = self._rows[which][fed:fed + n]
            dst.copy_(ops._c(rows.detach(), f'prdc {which} rows'))
            ops.prdc_norms(dst, out=self._norms[which][fed:fed + n])
        self._fed[which] = fed + n
        self._done = False

    def _compute(self):
        """The five passes, into the evaluation's own buffers; nothing is read back."""
        for which, n in self.n.items():
            if self._fed[which] != n:
                raise ValueError(f'prdc: {n} {which} rows were declared, {self._fed[which]} were fed')
        if self._host_only:
            raise host_only_error('prdc')
        if self._done:
            return
        for w in ('real', 'fake'):
            ops.prdc_knn(self._rows[w], self.k, norms=self._norms[w], out=self._knn[w])
            self._rad[w].copy_(self._knn[w][:, self.k - 1])
        r, f, nr, nf = self._rows['real'], self._rows['fake'], self._norms['real'], self._norms['fake']
        ops.prdc_cross(f, r, self._rad['real'], 'key', query_norms=nf, key_norms=nr, out=self._pass['fake_in_real'])
        ops.prdc_cross(r, f, self._rad['fake'], 'key', query_norms=nr, key_norms=nf, out=self._pass['real_in_fake'])
        ops.prdc_cross(r, f, self._rad['real'], 'query', query_norms=nr, key_norms=nf, out=self._pass['real_covered'])
        self._done = True

    def radii(self, which):
        """(n,) squared k-NN radii of the 'real' or 'fake' set (after all rows are in)."""
        self._compute()
        return self._rad[which].clone()

    def result(self):
        """{'precision', 'recall', 'density', 'coverage', 'k', 'n_real', 'n_fake'}."""
        self._compute()
        c_fr, c_rf, c_cov = (self._pass[p][0] for p in ('fake_in_real', 'real_in_fake', 'real_covered'))
        # integer counts, summed in int64 on the device; the evaluation's one host read
        hit_f, pairs, hit_r, cov = torch.stack([(c_fr > 0).sum(), c_fr.sum(dtype=torch.int64), (c_rf > 0).sum(),
                                                (c_cov > 0).sum()]).cpu().tolist()
        n_real, n_fake = self.n['real'], self.n['fake']
        return {'precision': hit_f / n_fake, 'recall': hit_r / n_real, 'density': pairs / (self.k * n_fake),
                'coverage': cov / n_real, 'k': self.k, 'n_real': n_real, 'n_fake': n_fake}

    def nearest_real(self):
        """(index int64 (n_fake,), squared distance fp32 (n_fake,)): the nearest real row of every generated row, the lowest
        index of a tie."""
        self._compute()
        _, dmin, imin = self._pass['fake_in_real']
        return imin.to(torch.int64), dmin.clone()
