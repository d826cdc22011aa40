"""The Kernel Inception Distance on the GPU (csrc/kid.hip, gan_lab_amd/kid.py) against the float64 restatement with
the full kernel matrices (tests/kid_reference.py).

Rows with small integer entries and ``gamma`` a power of two make ``t = gamma q.k + coef0``, its cube and every sum exact: row sums
and every field of ``result()`` must EQUAL the reference, duplicates and the exclusion of the row itself by index included.  On
real-valued rows each row sum is held to twice the worst relative error of ATen's CPU fp32 evaluation (``mm``, the cube and the
sum in fp32) on the same inputs, and ``kid`` to the bar those row errors imply.

Tile sizes the shapes are chosen around: 64 queries per workgroup, 64 keys per tile, depth chunks of 32, accumulation chains of
64 terms."""
import functools

import numpy as np
import pytest
import torch

import kid_reference as ref

pytestmark = pytest.mark.gpu

PASSES = ('real_real', 'fake_fake', 'real_fake')


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device='cuda', dtype=dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _evaluate(real, fake, block, gamma=None, batch=None):
    from gan_lab_amd import kid
    ev = kid.KID(real.shape[1], real.shape[0], fake.shape[0], block=block, gamma=gamma)
    for feed, rows in ((ev.feed_real, _dev(real)), (ev.feed_fake, _dev(fake))):
        step = batch or len(rows)
        for i in range(0, len(rows), step):
            feed(rows[i:i + step])
    return ev


# ---- 1. exact on integer rows ------------------------------------------------------------------------------------------------
INT_KINDS = {'ternary D=6': (6, -1, 1, 2.0 ** -3), 'wide D=192': (192, -4, 4, 2.0 ** -8)}


@functools.lru_cache(maxsize=None)
def _int_case(kind, n, m):
    d, lo, hi, gamma = INT_KINDS[kind]
    real, fake = ref.integer_rows(n, d, lo, hi, seed=n), ref.integer_rows(m, d, lo, hi, seed=1000 + m)
    return real, fake, gamma, ref.row_sums(real, fake, gamma), ref.kid(real, fake, 64, gamma)


@pytest.mark.parametrize('n,m', [(200, 136), (384, 320)])
@pytest.mark.parametrize('kind', sorted(INT_KINDS))
def test_integer_rows_equal_the_reference(kind, n, m):
    from gan_lab_amd import ops
    real, fake, gamma, want_sums, want = _int_case(kind, n, m)
    if kind.startswith('ternary'):
        # the input is what it is meant to be: duplicate rows within each set and across the sets
        assert len(np.unique(real, axis=0)) < n and len(np.unique(fake, axis=0)) < m
        assert len(np.unique(np.concatenate([real, fake]), axis=0)) < len(np.unique(real, axis=0)) + len(np.unique(fake, axis=0))
    r, f = _dev(real), _dev(fake)
    got = {'real_real': ops.kid_rowsums(r, r, gamma, exclude_diag=True), 'fake_fake': ops.kid_rowsums(f, f, gamma, exclude_diag=True),
           'real_fake': ops.kid_rowsums(r, f, gamma)}
    for p in PASSES:
        assert got[p].dtype == torch.float64 and np.array_equal(_np(got[p]), want_sums[p]), (kind, n, m, p)
    # exclude_diag leaves out one term, by index
    full = ops.kid_rowsums(r, r, gamma)
    diag = (gamma * (real.astype(np.float64) ** 2).sum(1) + 1.0) ** 3
    assert np.array_equal(_np(full), want_sums['real_real'] + diag)
    ev = _evaluate(real, fake, 64, gamma, batch=50)
    assert want['blocks'] == min(n, m) // 64 and want['kid_block_std'] > 0
    assert ev.result() == want
    sums = ev.row_sums()
    assert sorted(sums) == sorted(PASSES) and all(np.array_equal(_np(sums[p]), want_sums[p]) for p in PASSES)


# ---- 2. real-valued rows -------------------------------------------------------------------------------------------------
def _aten_row_sums(real, fake, gamma):
    """ATen's CPU fp32 evaluation: mm, then gamma t + coef0, the cube and the row sum in fp32."""
    out = {}
    for p, (a, b) in (('real_real', (real, real)), ('fake_fake', (fake, fake)), ('real_fake', (real, fake))):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        k = (gamma * (a @ b.T) + 1.0) ** 3
        if p != 'real_fake':
            k.fill_diagonal_(0.0)
        out[p] = k.sum(dim=1).double().numpy()
    return out


REAL_KINDS = {'randn': lambda z: z, 'one-signed': lambda z: np.abs(z) + 0.5}


@pytest.mark.parametrize('d', [48, 200])
@pytest.mark.parametrize('kind', sorted(REAL_KINDS))
def test_real_valued_rows(kind, d):
    n, m = 200, 136
    rng = np.random.default_rng(d)
    real = REAL_KINDS[kind](rng.standard_normal((n, d))).astype(np.float32)
    fake = REAL_KINDS[kind](0.9 * rng.standard_normal((m, d)) + 0.1).astype(np.float32)
    gamma = 1.0 / d
    want_sums, want = ref.row_sums(real, fake, gamma), ref.kid(real, fake, 64)
    ev = _evaluate(real, fake, 64)
    assert ev.gamma == gamma
    got_sums, aten = ev.row_sums(), _aten_row_sums(real, fake, gamma)
    rel = {p: float((np.abs(_np(got_sums[p]) - want_sums[p]) / np.abs(want_sums[p])).max()) for p in PASSES}
    rel_aten = {p: float((np.abs(aten[p] - want_sums[p]) / np.abs(want_sums[p])).max()) for p in PASSES}
    worst_aten = max(rel_aten.values())
    print(f'{kind} D={d}: worst relative row-sum error: kernel {max(rel.values()):.2e}, ATen CPU fp32 {worst_aten:.2e}')
    assert max(rel.values()) <= 2 * worst_aten, (rel, rel_aten)
    # kid: every row sum is within 2 * worst_aten of its value, so each of the three terms is within that share of the sum of
    # its row sums' magnitudes
    got = ev.result()
    terms = (np.abs(want_sums['real_real']).sum() / (n * (n - 1)) + np.abs(want_sums['fake_fake']).sum() / (m * (m - 1)) +
             2.0 * np.abs(want_sums['real_fake']).sum() / (n * m))
    bar = 2 * worst_aten * terms
    print(f'{kind} D={d}: kid {got["kid"]:.9g} (float64 {want["kid"]:.9g}): off by {abs(got["kid"] - want["kid"]):.2e}, bar {bar:.2e}')
    assert abs(got['kid'] - want['kid']) <= bar
    assert got['blocks'] == want['blocks'] == 2 and np.isfinite(got['kid_block_mean']) and got['kid_block_std'] >= 0


def test_row_sums_are_reproducible_and_do_not_depend_on_the_feeding():
    from gan_lab_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(3)
    q, k = torch.randn(200, 200, device='cuda', generator=gen), torch.randn(136, 200, device='cuda', generator=gen)
    a, b = ops.kid_rowsums(q, k, 1 / 200), ops.kid_rowsums(q, k, 1 / 200)
    assert torch.equal(a, b)
    assert torch.equal(ops.kid_rowsums(q, q, 1 / 200, exclude_diag=True), ops.kid_rowsums(q, q, 1 / 200, exclude_diag=True))
    out = torch.full((200,), float('nan'), dtype=torch.float64, device='cuda')
    assert ops.kid_rowsums(q, k, 1 / 200, out=out) is out and torch.equal(out, a)
    real, fake = q.cpu().numpy(), k.cpu().numpy()
    one, many = _evaluate(real, fake, 64), _evaluate(real, fake, 64, batch=7)
    assert one.result() == many.result()
    ptr = one._rows['real'].data_ptr()
    one.reset()
    with pytest.raises(ValueError, match='were fed'):
        one.result()
    one.feed_real(q)
    one.feed_fake(k)
    assert one.result() == many.result() and one._rows['real'].data_ptr() == ptr


def test_no_block_and_one_block():
    real, fake = ref.integer_rows(70, 6, -1, 1, seed=1), ref.integer_rows(66, 6, -1, 1, seed=2)
    for block, nb in ((100, 0), (64, 1)):
        got, want = _evaluate(real, fake, block, 2.0 ** -3).result(), ref.kid(real, fake, block, 2.0 ** -3)
        assert got == want and got['blocks'] == nb and got['kid_block_std'] is None and (got['kid_block_mean'] is None) == (nb == 0)


def test_wrapper_argument_checks():
    from gan_lab_amd import ops
    x = torch.zeros(10, 4, device='cuda')
    with pytest.raises(ValueError, match='exclude_diag'):
        ops.kid_rowsums(x, torch.zeros(6, 4, device='cuda'), 0.25, exclude_diag=True)
    with pytest.raises(ValueError, match='one width'):
        ops.kid_rowsums(x, torch.zeros(6, 5, device='cuda'), 0.25)
    with pytest.raises(TypeError, match='float32'):
        ops.kid_rowsums(x.double(), x, 0.25)
    with pytest.raises(TypeError, match='float64'):
        ops.kid_rowsums(x, x, 0.25, out=torch.zeros(10, device='cuda'))
    with pytest.raises(ValueError, match=r'\(10,\)'):
        ops.kid_rowsums(x, x, 0.25, out=torch.zeros(9, dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='numbers'):
        ops.kid_rowsums(x, x, float('nan'))
    assert tuple(ops.kid_rowsums(x[:, :3], x[:6, :3], 0.25).shape) == (10,)         # a strided view is made contiguous
