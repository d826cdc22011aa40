"""The Kernel Inception Distance (Binkowski et al. 2018) between two sets of feature rows, on the GPU (csrc/kid.hip; DESIGN.md
4.19): the unbiased squared maximum mean discrepancy under the cubic polynomial kernel ``k(x, y) = (gamma x.y + coef0)^3``,

  mmd2 = sum_{i != i'} k(r_i, r_i') / (n (n - 1)) + sum_{j != j'} k(g_j, g_j') / (m (m - 1)) - 2 sum_{i, j} k(r_i, g_j) / (n m)

for the real rows r_i (n of them) and the generated rows g_j (m of them), fp32 of one width.  Three matrix-free passes give the
three sums as row sums (``ops.kid_rowsums``; within a set the term i' == i is left out by index); no n x m kernel matrix is ever
stored.  ``kid`` is that number over the whole sets; the block statistics are the usual protocol - contiguous blocks of ``block``
rows of each set, the mmd2 of each pair of blocks, their mean and standard deviation.  With ``gamma = 1 / dim`` and
``coef0 = 1`` on Inception pool features this is KID proper; what the rows are is the caller's choice (the learners feed
``prdc.features``, the image reduced by 2x2 means).
"""
import torch

from . import ops, prdc
from ._metric_common import check_rows, device_gate, host_only_error, wanted as _wanted

MIN_BLOCK = 2


def wanted(metrics):
    return _wanted(metrics, 'kid')


def check_block(block, what='block'):
    if not isinstance(block, int) or isinstance(block, bool) or block < MIN_BLOCK:
        raise ValueError(f'kid: {what} must be an integer >= {MIN_BLOCK}, got {block!r}')
    return block


def validate_config(config):
    """Called when a learner is built: ``kid_res`` / ``kid_block`` are checked whether or not the metric is requested, and 'kid'
    is refused among the critic's metrics (it compares image sets; the critic has no part in it).  Returns (res, block)."""
    res = prdc.check_res(getattr(config, 'kid_res', 32), 'kid_res', prefix='kid')
    block = check_block(getattr(config, 'kid_block', 1000), 'kid_block')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'kid': the Kernel Inception Distance is a generator metric "
                         "(config.gen_metrics)")
    return res, block


def _set_size(v, name):
    if not isinstance(v, int) or isinstance(v, bool) or v < 2:
        raise ValueError(f'kid: {name} must be an integer >= 2 (the unbiased estimate divides by n (n - 1)), got {v!r}')
    return v


class KID(object):
    """One evaluation: ``feed_real`` / ``feed_fake`` minibatches of (n, dim) fp32 rows until the sets hold ``n_real`` and
    ``n_fake`` rows, then ``result()`` and ``row_sums()``.  ``reset()`` starts the next evaluation in the same buffers.
    ``gamma=None`` means ``1 / dim``; the degree is 3."""

    def __init__(self, dim, n_real, n_fake, block=1000, gamma=None, coef0=1.0, device='cuda'):
        # every argument check comes before any allocation
        if not isinstance(dim, int) or isinstance(dim, bool) or dim < 1:
            raise ValueError(f'kid: dim must be a positive integer, got {dim!r}')
        self.dim = dim
        self.n = {'real': _set_size(n_real, 'n_real'), 'fake': _set_size(n_fake, 'n_fake')}
        self.block = check_block(block)
        self.blocks = min(n_real, n_fake) // self.block
        self.gamma = 1.0 / dim if gamma is None else float(gamma)
        self.coef0 = float(coef0)
        if self.gamma != self.gamma or self.coef0 != self.coef0:
            raise ValueError(f'kid: gamma and coef0 must be numbers, got {gamma!r} and {coef0!r}')
        self.device, self._host_only = device_gate(device, 'kid')
        self._fed = {'real': 0, 'fake': 0}
        self._done = False
        if self._host_only:
            return
        dev = self.device
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        self._rows = {w: torch.empty((n, dim), dtype=torch.float32, device=dev) for w, n in self.n.items()}
        # row sums of the three passes over the whole sets, and over each pair of blocks (row b = block b)
        self._sums = {'real_real': f64(n_real), 'fake_fake': f64(n_fake), 'real_fake': f64(n_real)}
        self._block_sums = {p: f64(self.blocks, self.block) for p in self._sums}
        # the divisors of result(), on the device: a tensor divided by a tensor is an IEEE division (by a Python number the
        # library multiplies by the reciprocal, one more rounding)
        nb, blk = self.blocks, self.block
        self._div = torch.tensor([n_real * (n_real - 1), n_fake * (n_fake - 1), n_real * n_fake, blk * (blk - 1), blk * blk,
                                  max(nb, 1), max(nb - 1, 1)], dtype=torch.float64, device=dev)

    def reset(self):
        self._fed = {'real': 0, 'fake': 0}
        self._done = False

    def feed_real(self, rows):
        self._feed('real', rows)

    def feed_fake(self, rows):
        self._feed('fake', rows)

    def _feed(self, which, rows):
        check_rows(rows, self.dim, 'kid')
        n, fed = rows.shape[0], self._fed[which]
        if fed + n > self.n[which]:
            raise ValueError(f'kid: the {which} set was declared with {self.n[which]} rows; this feed of {n} would make '
                             f'{fed + n}')
        if n == 0:
            return
        if not self._host_only:
            self._rows[which][fed:fed + n].copy_(ops._c(rows.detach(), f'kid {which} rows'))
        self._fed[which] = fed + n
        self._done = False

    def _passes(self, real, fake, out):
        """The three launches for one pair of row sets, into the three (rows,) vectors ``out``."""
        ops.kid_rowsums(real, real, self.gamma, self.coef0, exclude_diag=True, out=out[0])
        ops.kid_rowsums(fake, fake, self.gamma, self.coef0, exclude_diag=True, out=out[1])
        ops.kid_rowsums(real, fake, self.gamma, self.coef0, out=out[2])

    def _compute(self):
        """Three launches over the whole sets and three per pair of blocks, into the evaluation's own buffers; nothing is read
        back."""
        for which, n in self.n.items():
            if self._fed[which] != n:
                raise ValueError(f'kid: {n} {which} rows were declared, {self._fed[which]} were fed')
        if self._host_only:
            raise host_only_error('kid')
        if self._done:
            return
        names = ('real_real', 'fake_fake', 'real_fake')
        real, fake = self._rows['real'], self._rows['fake']
        self._passes(real, fake, [self._sums[p] for p in names])
        for b in range(self.blocks):
            lo, hi = b * self.block, (b + 1) * self.block
            self._passes(real[lo:hi], fake[lo:hi], [self._block_sums[p][b] for p in names])
        self._done = True

    def row_sums(self):
        """{'real_real' (n_real,), 'fake_fake' (n_fake,), 'real_fake' (n_real,)}: float64 row sums of the kernel over the whole
        sets, the term i' == i left out within a set (after all rows are in)."""
        self._compute()
        return {p: t.clone() for p, t in self._sums.items()}

    @staticmethod
    def _mmd2(rr, ff, rf, div):
        """``div``: (n (n - 1), m (m - 1), n m) on the device."""
        return rr / div[0] + ff / div[1] - 2.0 * rf / div[2]

    def result(self):
        """{'kid', 'kid_block_mean', 'kid_block_std', 'blocks', 'block', 'n_real', 'n_fake'}.  The block mean is the blocks'
        values added in block order over their number, the standard deviation has the n - 1 denominator; without a whole block
        the mean is None, with fewer than two the deviation."""
        self._compute()
        n, m, nb, blk = self.n['real'], self.n['fake'], self.blocks, self.block
        s, bs = self._sums, self._block_sums
        div = self._div
        vals = [self._mmd2(s['real_real'].sum(), s['fake_fake'].sum(), s['real_fake'].sum(), div[0:3])]
        if nb:
            per_block = self._mmd2(bs['real_real'].sum(dim=1), bs['fake_fake'].sum(dim=1), bs['real_fake'].sum(dim=1),
                                   div[[3, 3, 4]])
            total = per_block[0]
            for b in range(1, nb):          # a fixed order: the value does not depend on how a library reduces a vector
                total = total + per_block[b]
            mean = total / div[5]
            vals.append(mean)
            if nb > 1:
                dev2 = (per_block - mean) * (per_block - mean)
                total = dev2[0]
                for b in range(1, nb):
                    total = total + dev2[b]
                vals.append((total / div[6]).sqrt())
        vals = torch.stack(vals).cpu().tolist()          # float64 scalars formed on the device; the evaluation's one host read
        return {'kid': vals[0], 'kid_block_mean': vals[1] if nb else None, 'kid_block_std': vals[2] if nb > 1 else None,
                'blocks': nb, 'block': blk, 'n_real': n, 'n_fake': m}
