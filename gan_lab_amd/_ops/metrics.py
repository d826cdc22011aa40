"""Launchers of the validation metrics.  No autograd: metrics run under ``torch.no_grad`` - except the power-spectrum regulariser
at the end (``spectrum_loss``), the one metric that is also a loss term and the one ``autograd.Function`` here.

Drives csrc/swd.hip, csrc/prdc.hip, csrc/frechet.hip, csrc/kid.hip, csrc/ppl.hip, csrc/msssim.hip and csrc/spectrum.hip; composed
in gan_lab_amd/swd.py, prdc.py, frechet.py, kid.py, ppl.py, msssim.py, spectrum.py and spectrum_reg.py.  Re-exported by ``gan_lab_amd.ops``."""
import torch

from .. import _lib
from .._lib import check
from .core import _c, _ct, _new, _p, _st


# ---- sliced Wasserstein distance (csrc/swd.hip; composed in gan_lab_amd/swd.py) ----------------------------------------------
SWD_DESC = _lib.DEFINES['GANLAB_SWD_DESC']


def _swd_planes(x, what):
    x = _c(x, what)
    if x.dim() < 2 or x.shape[-1] % 2 or x.shape[-2] % 2 or min(x.shape[-2:]) < 4:
        raise ValueError(f'{what}: needs (..., H, W) planes with even H, W >= 4, got {tuple(x.shape)}')
    return x


def swd_down(x):
    """Pyramid step down: the 5x5 binomial filter with mirror boundary, every second pixel kept."""
    x = _swd_planes(x, 'swd_down input')
    h, w = x.shape[-2:]
    out = torch.empty(x.shape[:-2] + (h // 2, w // 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().ganlab_swd_down_f32(_p(x), _p(out), x.numel() // (h * w), h, w, _st()), 'swd_down')
    return out


def swd_band(g0, g1):
    """Laplacian band ``g0 - up(g1)`` (zero-insert upsample and its filter are never materialised)."""
    g0, g1 = _swd_planes(g0, 'swd_band fine level'), _c(g1, 'swd_band coarse level')
    h, w = g0.shape[-2:]
    if tuple(g1.shape) != tuple(g0.shape[:-2]) + (h // 2, w // 2):
        raise ValueError(f'swd_band: coarse level must be {tuple(g0.shape[:-2]) + (h // 2, w // 2)}, got {tuple(g1.shape)}')
    out = torch.empty_like(g0)
    check(_lib.lib().ganlab_swd_band_f32(_p(g0), _p(g1), _p(out), g0.numel() // (h * w), h, w, _st()), 'swd_band')
    return out


def swd_gather(band, pos, desc, partials):
    """Descriptor rows of an (N, 3, S, S) level at the (N, n, 2) int32 centres ``pos`` into ``desc`` ((N n, 147) rows of a
    preallocated set buffer) and the per-image fp64 channel sums into ``partials`` ((N, 6))."""
    band, pos = _c(band, 'swd_gather level'), _ct(pos, torch.int32, 'swd_gather positions')
    if band.dim() != 4 or band.shape[1] != 3 or band.shape[2] != band.shape[3] or band.shape[2] < 7 or pos.dim() != 3 or \
            pos.shape[0] != band.shape[0] or pos.shape[2] != 2:
        raise ValueError(f'swd_gather: needs an (N, 3, S, S) level with S >= 7 and (N, n, 2) positions, got '
                         f'{tuple(band.shape)} and {tuple(pos.shape)}')
    n_img, n = pos.shape[:2]
    _c(desc, 'swd_gather descriptors'), _ct(partials, torch.float64, 'swd_gather partials')
    if not desc.is_contiguous() or not partials.is_contiguous() or tuple(desc.shape) != (n_img * n, SWD_DESC) or \
            tuple(partials.shape) != (n_img, 6):
        raise ValueError(f'swd_gather: outputs must be contiguous ({n_img * n}, {SWD_DESC}) and ({n_img}, 6), got '
                         f'{tuple(desc.shape)} and {tuple(partials.shape)}')
    check(_lib.lib().ganlab_swd_gather_f32(_p(band), _p(pos), _p(desc), _p(partials), n_img, n, band.shape[2], _st()),
          'swd_gather')
    return desc


def swd_stats(partials, per_image):
    """(6,) fp64: per-channel mean, then population standard deviation, from the (images, 6) partials of ``swd_gather``
    (``per_image`` values per channel and image); reduced in a fixed order."""
    partials = _ct(partials, torch.float64, 'swd_stats partials')
    if partials.dim() != 2 or partials.shape[1] != 6 or partials.shape[0] < 1:
        raise ValueError(f'swd_stats: partials must be (images, 6), got {tuple(partials.shape)}')
    out = torch.empty(6, dtype=torch.float64, device=partials.device)
    check(_lib.lib().ganlab_swd_stats_f64(_p(partials), partials.shape[0], int(per_image), _p(out), _st()), 'swd_stats')
    return out


def swd_project(desc, dirs, stats, out=None):
    """(D, M) projections of the normalised descriptors: ``dirs @ ((desc - mean) / std).T`` with the per-channel ``stats`` of
    ``swd_stats`` applied as the rows are loaded (fp32 MFMA)."""
    desc, dirs, stats = _c(desc, 'swd_project descriptors'), _c(dirs, 'swd_project directions'), \
        _ct(stats, torch.float64, 'swd_project statistics')
    if desc.dim() != 2 or desc.shape[1] != SWD_DESC or dirs.dim() != 2 or dirs.shape[1] != SWD_DESC or stats.numel() != 6:
        raise ValueError(f'swd_project: needs (M, {SWD_DESC}) descriptors, (D, {SWD_DESC}) directions and 6 statistics, got '
                         f'{tuple(desc.shape)}, {tuple(dirs.shape)}, {tuple(stats.shape)}')
    m, d = desc.shape[0], dirs.shape[0]
    if out is None:
        out = torch.empty((d, m), dtype=torch.float32, device=desc.device)
    elif tuple(_c(out, 'swd_project output').shape) != (d, m) or not out.is_contiguous():
        raise ValueError(f'swd_project: output must be a contiguous ({d}, {m}) tensor, got {tuple(out.shape)}')
    check(_lib.lib().ganlab_swd_project_f32(_p(desc), _p(dirs), _p(stats), _p(out), m, d, _st()), 'swd_project')
    return out


_SWD_WS = {}


def _swd_workspace(nbytes, device):
    ws = _SWD_WS.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _SWD_WS[device] = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
    return ws


def swd_sort(x, out=None):
    """Each row of a (D, M) buffer sorted ascending (rocPRIM radix sorts inside the library)."""
    x = _c(x, 'swd_sort input')
    if x.dim() != 2 or x.numel() == 0:
        raise ValueError(f'swd_sort: needs a non-empty (D, M) tensor, got {tuple(x.shape)}')
    if out is None:
        out = torch.empty_like(x)
    elif tuple(_c(out, 'swd_sort output').shape) != tuple(x.shape) or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
        raise ValueError('swd_sort: output must be a contiguous tensor of the input\'s shape that does not alias it')
    d, m = x.shape
    L = _lib.lib()
    nbytes = L.ganlab_swd_sort_workspace(d, m)
    if nbytes == 0:
        raise ValueError(f'swd_sort: a ({d}, {m}) buffer is refused (D * M must stay below 2^32 - 1)')
    ws = _swd_workspace(nbytes, x.device)
    check(L.ganlab_swd_sort_f32(_p(x), _p(out), d, m, _p(ws), ws.numel(), _st()), 'swd_sort')
    return out


def swd_distance(a, b):
    """0-d fp64 device tensor: mean |a - b| over two sorted (D, M) buffers (fp64 partials, fixed order)."""
    a, b = _c(a, 'swd_distance a'), _c(b, 'swd_distance b')
    if a.dim() != 2 or a.shape != b.shape or a.numel() == 0:
        raise ValueError(f'swd_distance: needs two equal non-empty (D, M) tensors, got {tuple(a.shape)} and {tuple(b.shape)}')
    d, m = a.shape
    L = _lib.lib()
    ws = torch.empty(L.ganlab_swd_distance_workspace(d, m), dtype=torch.uint8, device=a.device)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    check(L.ganlab_swd_distance_f64(_p(a), _p(b), _p(out), d, m, _p(ws), ws.numel(), _st()), 'swd_distance')
    return out[0]


def swd_positions(n_images, n_per_image, size, seed, offset, device):
    """(n_images, n_per_image, 2) int32 patch centres uniform in [3, size - 4] from the Philox stream at ``offset``
    (ceil(n_per_image / 2) counters per image)."""
    if int(size) < 7 or int(n_images) < 1 or int(n_per_image) < 1:
        raise ValueError(f'swd_positions: needs size >= 7 and positive counts, got {n_images}, {n_per_image}, {size}')
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: swd_positions draws on the GPU (got device {device!r}); the HIP path has no CPU '
                        f'fallback')
    out = torch.empty((int(n_images), int(n_per_image), 2), dtype=torch.int32, device=device)
    check(_lib.lib().ganlab_swd_positions_i32(_p(out), int(n_images), int(n_per_image), int(size), int(seed) & (2 ** 64 - 1),
                                              int(offset), _st()), 'swd_positions')
    return out


def swd_directions(n_dirs, seed, offset, device):
    """(n_dirs, 147) unit-norm Gaussian directions from the Philox stream at ``offset`` (147 counters per direction)."""
    if int(n_dirs) < 1:
        raise ValueError(f'swd_directions: needs a positive count, got {n_dirs}')
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: swd_directions draws on the GPU (got device {device!r}); the HIP path has no CPU '
                        f'fallback')
    out = torch.empty((int(n_dirs), SWD_DESC), dtype=torch.float32, device=device)
    check(_lib.lib().ganlab_swd_directions_f32(_p(out), int(n_dirs), int(seed) & (2 ** 64 - 1), int(offset), _st()),
          'swd_directions')
    return out


# ---- k-nearest-neighbour precision / recall / density / coverage (csrc/prdc.hip; composed in gan_lab_amd/prdc.py) --------------
PRDC_MAX_K = _lib.DEFINES['GANLAB_PRDC_MAX_K']


def _prdc_rows(t, what):
    t = _c(t, what)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f'{what}: needs a non-empty (rows, width) matrix, got {tuple(t.shape)}')
    return t


def _prdc_vector(t, dtype, n, what):
    t = _ct(t, dtype, what)
    if tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f'{what}: must be a contiguous ({n},) tensor, got {tuple(t.shape)}')
    return t


def prdc_norms(rows, out=None):
    """(N,) squared Euclidean norms of the rows of an (N, D) matrix: fp64 sums in a fixed order, rounded once."""
    rows = _prdc_rows(rows, 'prdc_norms rows')
    n, d = rows.shape
    out = _new((n,), rows) if out is None else _prdc_vector(out, torch.float32, n, 'prdc_norms out')
    check(_lib.lib().ganlab_prdc_norms_f32(_p(rows), _p(out), n, d, _st()), 'prdc_norms')
    return out


def prdc_knn(rows, k, norms=None, out=None):
    """(N, k): per row of the (N, D) matrix the ``k`` smallest squared distances to the OTHER rows, ascending - the row itself is
    excluded by index, a duplicate at another index counts; the last column is the k-NN radius.  ``norms``: ``prdc_norms(rows)``
    when the caller already has them."""
    rows = _prdc_rows(rows, 'prdc_knn rows')
    n, d = rows.shape
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= PRDC_MAX_K:
        raise ValueError(f'prdc_knn: k must be an integer in [1, {PRDC_MAX_K}], got {k!r}')
    if k >= n:
        raise ValueError(f'prdc_knn: k must be below the number of rows (k = {k}, rows = {n})')
    norms = prdc_norms(rows) if norms is None else _prdc_vector(norms, torch.float32, n, 'prdc_knn norms')
    if out is None:
        out = _new((n, k), rows)
    elif tuple(_c(out, 'prdc_knn out').shape) != (n, k) or not out.is_contiguous():
        raise ValueError(f'prdc_knn: out must be a contiguous ({n}, {k}) tensor, got {tuple(out.shape)}')
    check(_lib.lib().ganlab_prdc_knn_f32(_p(rows), _p(norms), _p(out), n, d, k, _st()), 'prdc_knn')
    return out


def prdc_cross(queries, keys, radii, radius_of='key', query_norms=None, key_norms=None, out=None):
    """Queries (M, D) against keys (N, D) under a radius per key (``radius_of='key'``: ``radii`` is (N,)) or per query
    (``'query'``: (M,)).  Returns per query row (count int32, smallest squared distance fp32, its key index int32): the number of
    keys with squared distance <= the radius, and the nearest key, the lowest index of a tie.  ``out``: the three tensors."""
    queries, keys = _prdc_rows(queries, 'prdc_cross queries'), _prdc_rows(keys, 'prdc_cross keys')
    (m, d), (n, dk) = queries.shape, keys.shape
    if d != dk:
        raise ValueError(f'prdc_cross: queries and keys must have one width, got {d} and {dk}')
    if radius_of not in ('key', 'query'):
        raise ValueError(f"prdc_cross: radius_of must be 'key' or 'query', got {radius_of!r}")
    radii = _prdc_vector(radii, torch.float32, n if radius_of == 'key' else m, f'prdc_cross radii (one per {radius_of})')
    query_norms = prdc_norms(queries) if query_norms is None else \
        _prdc_vector(query_norms, torch.float32, m, 'prdc_cross query_norms')
    key_norms = prdc_norms(keys) if key_norms is None else _prdc_vector(key_norms, torch.float32, n, 'prdc_cross key_norms')
    if out is None:
        out = (torch.empty((m,), dtype=torch.int32, device=queries.device), _new((m,), queries),
               torch.empty((m,), dtype=torch.int32, device=queries.device))
    count = _prdc_vector(out[0], torch.int32, m, 'prdc_cross count')
    dmin = _prdc_vector(out[1], torch.float32, m, 'prdc_cross smallest distance')
    imin = _prdc_vector(out[2], torch.int32, m, 'prdc_cross nearest index')
    check(_lib.lib().ganlab_prdc_cross_f32(_p(queries), _p(query_norms), _p(keys), _p(key_norms), _p(radii),
                                           1 if radius_of == 'query' else 0, _p(count), _p(dmin), _p(imin), m, n, d, _st()),
          'prdc_cross')
    return count, dmin, imin


# ---- Frechet moments and KID row sums (csrc/frechet.hip, csrc/kid.hip; composed in gan_lab_amd/frechet.py and kid.py) ------------
MOMENTS_MAX_DIM = 4096               # ganlab_moments_accum_f32: a (D, D) float64 second-moment matrix of 128 MiB


def _accumulator(t, shape, what):
    """A float64 tensor a kernel adds into through its raw pointer: a non-contiguous view is an error."""
    if isinstance(t, torch.Tensor) and (tuple(t.shape) != tuple(shape) or not t.is_contiguous()):
        raise ValueError(f'{what}: must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)} with strides {t.stride()}')
    return _ct(t, torch.float64, what)


def moments_accum(rows, pivot, sum, gram):
    """``sum[a] += sum_i (x_ia - c_a)`` and ``gram[a][b] += sum_i (x_ia - c_a)(x_ib - c_b)`` over the rows of an (n, D) fp32
    matrix, ``c`` the (D,) fp32 ``pivot``; ``sum`` (D,) and ``gram`` (D, D) are float64 and accumulated into (zero them before the
    first call).  ``gram`` is written in full and stays exactly symmetric.  D <= 4096."""
    rows = _prdc_rows(rows, 'moments_accum rows')
    n, d = rows.shape
    if d > MOMENTS_MAX_DIM:
        raise ValueError(f'moments_accum: the width must be at most {MOMENTS_MAX_DIM}, got {d}')
    pivot = _prdc_vector(pivot, torch.float32, d, 'moments_accum pivot')
    sum = _accumulator(sum, (d,), 'moments_accum sum')
    gram = _accumulator(gram, (d, d), 'moments_accum gram')
    check(_lib.lib().ganlab_moments_accum_f32(_p(rows), n, d, _p(pivot), _p(sum), _p(gram), _st()), 'moments_accum')
    return sum, gram


def kid_rowsums(queries, keys, gamma, coef0=1.0, exclude_diag=False, out=None):
    """(M,) float64: ``out[i] = sum_j (gamma q_i.k_j + coef0)^3`` of the queries (M, D) against the keys (N, D); the dot product
    and ``gamma dot + coef0`` (one fma) in fp32, the cube and the sum in float64.  ``exclude_diag`` leaves ``j == i`` out by index
    and needs M == N."""
    queries, keys = _prdc_rows(queries, 'kid_rowsums queries'), _prdc_rows(keys, 'kid_rowsums keys')
    (m, d), (n, dk) = queries.shape, keys.shape
    if d != dk:
        raise ValueError(f'kid_rowsums: queries and keys must have one width, got {d} and {dk}')
    if exclude_diag and m != n:
        raise ValueError(f'kid_rowsums: exclude_diag leaves out the term j == i and needs as many queries as keys, got {m} and {n}')
    gamma, coef0 = float(gamma), float(coef0)
    if gamma != gamma or coef0 != coef0:
        raise ValueError(f'kid_rowsums: gamma and coef0 must be numbers, got {gamma!r} and {coef0!r}')
    out = torch.empty((m,), dtype=torch.float64, device=queries.device) if out is None else \
        _prdc_vector(out, torch.float64, m, 'kid_rowsums out')
    check(_lib.lib().ganlab_kid_rowsums_f32(_p(queries), m, _p(keys), n, d, gamma, coef0, 1 if exclude_diag else 0, _p(out),
                                            _st()), 'kid_rowsums')
    return out


# ---- perceptual path length (csrc/ppl.hip; composed in gan_lab_amd/ppl.py) -----------------------------------------------------
PPL_MAX_DIM = _lib.DEFINES['GANLAB_PPL_MAX_DIM']
PPL_MODES = {'lerp': _lib.DEFINES['GANLAB_PPL_LERP'], 'slerp': _lib.DEFINES['GANLAB_PPL_SLERP']}
PPL_SAMPLINGS = {'full': _lib.DEFINES['GANLAB_PPL_FULL'], 'end': _lib.DEFINES['GANLAB_PPL_END']}
PPL_RECORD = ('mean', 'lo', 'hi', 'kept', 'nonfinite')


def check_ppl_epsilon(epsilon, what='ppl_endpoints: epsilon'):
    """``epsilon`` as a float: finite, positive and below 1, else a ValueError that names ``what``."""
    try:
        eps = float(epsilon)
    except (TypeError, ValueError):
        eps = float('nan')
    if isinstance(epsilon, bool) or not 0.0 < eps < 1.0:
        raise ValueError(f'{what} must be a finite number in (0, 1) (got {epsilon!r})')
    return eps


def ppl_endpoints(a, b, epsilon, mode, sampling='full', seed=0, offset=0):
    """``(t (N,), out (2, N, D))`` from the (N, D) rows ``a`` and ``b``: ``out[0]`` the point of the path from a to b at ``t``,
    ``out[1]`` at ``t + epsilon``, one launch.  ``sampling`` 'full': ``t[n]`` uniform in [0, 1), one Philox counter per row from
    ``offset`` under the key ``seed`` (a short draw is the prefix of a long one); 'end': t = 0.  ``mode`` 'lerp': ``a + (b - a) t``
    (formed in double, rounded once); 'slerp': StyleGAN's spherical interpolation of the normalised rows, rescaled to norm
    sqrt(D); parallel, antipodal or zero rows give ``a / |a| sqrt(D)`` at both ends.  D <= 4096."""
    a, b = _prdc_rows(a, 'ppl_endpoints a'), _prdc_rows(b, 'ppl_endpoints b')
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f'ppl_endpoints: a and b must be equal (N, D) matrices on one device, got {tuple(a.shape)} on {a.device} '
                         f'and {tuple(b.shape)} on {b.device}')
    n, d = a.shape
    if d > PPL_MAX_DIM:
        raise ValueError(f'ppl_endpoints: the width of a and b must be at most {PPL_MAX_DIM}, got {d}')
    if mode not in PPL_MODES:
        raise ValueError(f"ppl_endpoints: mode must be 'lerp' or 'slerp', got {mode!r}")
    if sampling not in PPL_SAMPLINGS:
        raise ValueError(f"ppl_endpoints: sampling must be 'full' or 'end', got {sampling!r}")
    eps = check_ppl_epsilon(epsilon)
    if isinstance(offset, bool) or not isinstance(offset, int) or offset < 0:
        raise ValueError(f'ppl_endpoints: offset must be a non-negative integer, got {offset!r}')
    t, out = _new((n,), a), _new((2, n, d), a)
    check(_lib.lib().ganlab_ppl_endpoints_f32(_p(a), _p(b), _p(t), _p(out), n, d, eps, PPL_MODES[mode], PPL_SAMPLINGS[sampling],
                                              int(seed) & (2 ** 64 - 1), offset, _st()), 'ppl_endpoints')
    return t, out


def row_sqdist(x, y, out=None):
    """(N,) squared Euclidean distances between the rows of two (N, D) matrices (two tensors, or the halves of one (2N, D)
    tensor): differences, squares and sums in float64, rounded once."""
    x, y = _prdc_rows(x, 'row_sqdist x'), _prdc_rows(y, 'row_sqdist y')
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f'row_sqdist: x and y must be equal (N, D) matrices on one device, got {tuple(x.shape)} on {x.device} '
                         f'and {tuple(y.shape)} on {y.device}')
    n, d = x.shape
    out = _new((n,), x) if out is None else _prdc_vector(out, torch.float32, n, 'row_sqdist out')
    check(_lib.lib().ganlab_row_sqdist_f32(_p(x), _p(y), _p(out), n, d, _st()), 'row_sqdist')
    return out


def trimmed_mean(v, q_lo=0.01, q_hi=0.99):
    """(5,) float64 device record ``PPL_RECORD`` = (mean, lo, hi, kept, nonfinite) of the (n,) values ``v``: ``lo`` / ``hi`` are
    numpy.percentile's 'lower' at quantile ``q_lo`` / 'higher' at ``q_hi`` (sorted on the device), ``kept`` the number of values
    with lo <= v <= hi, ``mean`` their float64 mean.  A NaN or an infinity among the values: ``nonfinite`` counts them and
    mean, lo and hi are NaN."""
    v = _c(v, 'trimmed_mean values')
    if v.dim() != 1 or v.numel() < 1:
        raise ValueError(f'trimmed_mean: values must be a non-empty (n,) vector, got {tuple(v.shape)}')
    try:
        q_lo, q_hi = float(q_lo), float(q_hi)
    except (TypeError, ValueError):
        q_lo = q_hi = float('nan')
    if not 0.0 <= q_lo <= q_hi <= 1.0:
        raise ValueError(f'trimmed_mean: q_lo and q_hi must satisfy 0 <= q_lo <= q_hi <= 1, got {q_lo!r} and {q_hi!r}')
    L = _lib.lib()
    nbytes = L.ganlab_trimmed_mean_workspace(v.numel())
    if nbytes == 0:
        raise ValueError(f'trimmed_mean: {v.numel()} values are refused (the count must stay below 2^31)')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    record = torch.empty(len(PPL_RECORD), dtype=torch.float64, device=v.device)
    check(L.ganlab_trimmed_mean_f32(_p(v), v.numel(), q_lo, q_hi, _p(record), _p(ws), ws.numel(), _st()), 'trimmed_mean')
    return record


# ---- multi-scale structural similarity (csrc/msssim.hip; composed in gan_lab_amd/msssim.py) -------------------------------------
MSSSIM_LEVELS = _lib.DEFINES['GANLAB_MSSSIM_LEVELS']


def _msssim_images(t, side, what):
    """A (k, 3, side, side) fp32 GPU tensor whose images are contiguous (3, side, side) blocks a fixed number of floats apart:
    a whole batch, or every second image of one (``x[0::2]``).  Never copied: the kernel takes the stride."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f'gan_lab_amd.ops: {what} must be a float32 tensor on the GPU (got {type(t).__name__}, '
                        f'{getattr(t, "device", None)}, {getattr(t, "dtype", None)}); the HIP path has no CPU fallback')
    if t.dim() != 4 or tuple(t.shape[1:]) != (3, side, side) or t.shape[0] < 1 or \
            tuple(t.stride()[1:]) != (side * side, side, 1) or \
            (t.shape[0] > 1 and t.stride(0) < 3 * side * side):
        raise ValueError(f'{what}: needs (k, 3, {side}, {side}) images, each contiguous, got shape {tuple(t.shape)} strides '
                         f'{tuple(t.stride())}')
    return t


def msssim_workspace(pairs, res, device):
    """The fp64 per-tile partials of an evaluation of ``pairs`` pairs at ``res`` x ``res`` (all five levels), uninitialised."""
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: msssim_workspace allocates on the GPU (got device {device!r}); the HIP path has no '
                        f'CPU fallback')
    nbytes = _lib.lib().ganlab_msssim_workspace(int(pairs), int(res))
    if nbytes == 0:
        raise ValueError(f'msssim_workspace: needs pairs >= 1 and a power-of-two resolution in [16, 16384], got {pairs}, {res}')
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def msssim_level(a, b, level, res, c1, c2, workspace, first, pairs, next_a=None, next_b=None):
    """Level ``level`` (side ``res >> level``) of pairs ``first ..`` of an evaluation of ``pairs`` pairs: their (cs, ssim) tile
    partials go into ``workspace``, the 2 x 2 means of both images into ``next_a`` / ``next_b`` (None at the last level)."""
    side = int(res) >> int(level)
    a, b = _msssim_images(a, side, 'msssim_level a'), _msssim_images(b, side, 'msssim_level b')
    count = a.shape[0]
    workspace = _ct(workspace, torch.float64, 'msssim_level workspace')
    if b.shape[0] != count or (count > 1 and a.stride(0) != b.stride(0)):
        raise ValueError(f'msssim_level: a and b must hold the same number of images at the same stride, got '
                         f'{tuple(a.shape)} / {a.stride(0)} and {tuple(b.shape)} / {b.stride(0)}')
    if (next_a is None) != (next_b is None):
        raise ValueError('msssim_level: next_a and next_b come together')
    nstride = 0
    if next_a is not None:
        next_a = _msssim_images(next_a, side // 2, 'msssim_level next_a')
        next_b = _msssim_images(next_b, side // 2, 'msssim_level next_b')
        if next_a.shape[0] != count or next_b.shape[0] != count or (count > 1 and next_a.stride(0) != next_b.stride(0)):
            raise ValueError(f'msssim_level: next_a and next_b must hold {count} images at one stride, got '
                             f'{tuple(next_a.shape)} and {tuple(next_b.shape)}')
        nstride = next_a.stride(0) if count > 1 else 3 * (side // 2) ** 2
    stride = a.stride(0) if count > 1 else 3 * side * side
    check(_lib.lib().ganlab_msssim_level_f32(_p(a), _p(b), stride, _p(next_a), _p(next_b), nstride, int(first), count,
                                             int(pairs), int(res), int(level), float(c1), float(c2), _p(workspace),
                                             workspace.numel() * 8, _st()), 'msssim_level')


def msssim_finish(workspace, pairs, res, table, values, out):
    """The evaluation's partials -> ``table`` (pairs, 5, 2) = (CS_i, SSIM_i) clamped at 0, ``values`` (pairs,) = the weighted
    products, ``out`` (6,) = mean value, mean CS_0..3, mean SSIM_4; all fp64, fixed order."""
    workspace = _ct(workspace, torch.float64, 'msssim_finish workspace')
    for t, shape, what in ((table, (pairs, MSSSIM_LEVELS, 2), 'table'), (values, (pairs,), 'values'), (out, (6,), 'out')):
        if tuple(_ct(t, torch.float64, f'msssim_finish {what}').shape) != shape or not t.is_contiguous():
            raise ValueError(f'msssim_finish: {what} must be a contiguous {shape} tensor, got {tuple(t.shape)}')
    check(_lib.lib().ganlab_msssim_finish_f64(_p(workspace), workspace.numel() * 8, int(pairs), int(res), _p(table), _p(values),
                                              _p(out), _st()), 'msssim_finish')
    return out


# ---- radial power spectrum (csrc/spectrum.hip; composed in gan_lab_amd/spectrum.py) ---------------------------------------------
SPECTRUM_MIN_RES, SPECTRUM_MAX_RES = _lib.DEFINES['GANLAB_SPECTRUM_MIN_RES'], _lib.DEFINES['GANLAB_SPECTRUM_MAX_RES']
SPECTRUM_WINDOWS = {'none': _lib.DEFINES['GANLAB_SPECTRUM_WINDOW_NONE'], 'hann': _lib.DEFINES['GANLAB_SPECTRUM_WINDOW_HANN']}


def _spectrum_size(query, count, res, what):
    nbytes = query(int(count), int(res))
    if nbytes == 0:
        raise ValueError(f'{what}: needs a count >= 1 and a power-of-two resolution in [{SPECTRUM_MIN_RES}, {SPECTRUM_MAX_RES}], '
                         f'got {count}, {res}')
    return nbytes


def spectrum_scratch_bytes(count, res):
    """Bytes of scratch a feed of ``count`` images at ``res`` x ``res`` needs (a host call)."""
    return _spectrum_size(_lib.lib().ganlab_spectrum_scratch, count, res, 'spectrum_scratch_bytes')


def _spectrum_alloc(nbytes, device, what):
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: {what} allocates on the GPU (got device {device!r}); the HIP path has no CPU fallback')
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def spectrum_workspace(n_images, res, device):
    """The (n_images, res / 2 + 1) fp64 per-image profiles of an evaluation, uninitialised."""
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: spectrum_workspace allocates on the GPU (got device {device!r}); the HIP path has no '
                        f'CPU fallback')
    nbytes = _spectrum_size(_lib.lib().ganlab_spectrum_workspace, n_images, res, 'spectrum_workspace')
    return _spectrum_alloc(nbytes, device, 'spectrum_workspace').view(int(n_images), int(res) // 2 + 1)


def spectrum_scratch(count, res, device):
    """Scratch for feeds of up to ``count`` images: tables, half spectra and per-tile bin sums, uninitialised."""
    if torch.device(device).type != 'cuda':
        raise TypeError(f'gan_lab_amd.ops: spectrum_scratch allocates on the GPU (got device {device!r}); the HIP path has no '
                        f'CPU fallback')
    return _spectrum_alloc((spectrum_scratch_bytes(count, res) + 7) // 8 * 8, device, 'spectrum_scratch')


def spectrum_feed(x, res, window, scratch, workspace, first, n_images):
    """The profiles of the (k, 3, res, res) fp32 images ``x``, images ``first ..`` of an evaluation of ``n_images``, into their
    rows of ``workspace``.  ``window``: 'hann' or 'none'."""
    x = _msssim_images(x, int(res), 'spectrum_feed x')
    if window not in SPECTRUM_WINDOWS:
        raise ValueError(f'spectrum_feed: window must be one of {sorted(SPECTRUM_WINDOWS)}, got {window!r}')
    scratch = _ct(scratch, torch.float64, 'spectrum_feed scratch')
    workspace = _ct(workspace, torch.float64, 'spectrum_feed workspace')
    count = x.shape[0]
    stride = x.stride(0) if count > 1 else 3 * int(res) ** 2
    check(_lib.lib().ganlab_spectrum_feed_f32(_p(x), stride, int(first), count, int(n_images), int(res), SPECTRUM_WINDOWS[window],
                                              _p(scratch), scratch.numel() * 8, _p(workspace), workspace.numel() * 8, _st()),
          'spectrum_feed')


def spectrum_finish(workspace_a, workspace_b, n_images, res, out):
    """``out`` = set a's profile S[0 .. res/2] and its decibels; with ``workspace_b`` also set b's two rows, then the distances
    'spectrum' and 'hf': 4 (res / 2 + 1) + 2 fp64 values, else 2 (res / 2 + 1)."""
    workspace_a = _ct(workspace_a, torch.float64, 'spectrum_finish workspace_a')
    if workspace_b is not None:
        workspace_b = _ct(workspace_b, torch.float64, 'spectrum_finish workspace_b')
        if workspace_b.numel() != workspace_a.numel():
            raise ValueError(f'spectrum_finish: the two workspaces must have one size, got {workspace_a.numel()} and '
                             f'{workspace_b.numel()}')
    nb = int(res) // 2 + 1
    need = 4 * nb + 2 if workspace_b is not None else 2 * nb
    if _ct(out, torch.float64, 'spectrum_finish out').numel() != need or not out.is_contiguous():
        raise ValueError(f'spectrum_finish: out must be a contiguous tensor of {need} values, got {tuple(out.shape)}')
    check(_lib.lib().ganlab_spectrum_finish_f64(_p(workspace_a), _p(workspace_b), workspace_a.numel() * 8, int(n_images), int(res),
                                                _p(out), out.numel() * 8, _st()), 'spectrum_finish')
    return out


# ---- the power-spectrum regulariser (csrc/spectrum.hip; composed in gan_lab_amd/spectrum_reg.py) ----------------
SPECTRUM_BANDS = {'all': _lib.DEFINES['GANLAB_SPECTRUM_BAND_ALL'], 'hf': _lib.DEFINES['GANLAB_SPECTRUM_BAND_HF']}
_SPECTRUM_REG_SCRATCH_BYTES = 64 << 20      # the half spectra of one chunk of images, forward and backward alike


def _spectrum_batch(x, what):
    """``x`` as the spectrum kernels walk it: a (N, 3, R, R) fp32 GPU batch whose images are contiguous blocks a fixed number of
    floats apart - a whole batch or a slice of one along dim 0, taken as it is; anything else is made contiguous."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        _c(x, what)
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f'{what}: needs a (N, 3, R, R) batch, got {tuple(x.shape)}')
    res = int(x.shape[2])
    if res < SPECTRUM_MIN_RES or res > SPECTRUM_MAX_RES or res & (res - 1):
        raise ValueError(f'{what}: R must be a power of two in [{SPECTRUM_MIN_RES}, {SPECTRUM_MAX_RES}], got {res}')
    if tuple(x.stride()[1:]) != (res * res, res, 1) or (x.shape[0] > 1 and x.stride(0) < 3 * res * res):
        x = x.contiguous()
    return x, res


def _spectrum_chunk(res, n, chunk):
    if chunk is None:
        per_image = spectrum_scratch_bytes(2, res) - spectrum_scratch_bytes(1, res)
        return max(1, min(n, _SPECTRUM_REG_SCRATCH_BYTES // per_image))
    if not isinstance(chunk, int) or isinstance(chunk, bool) or chunk < 1:
        raise ValueError(f'spectrum: chunk must be a positive integer or None, got {chunk!r}')
    return min(n, chunk)


def _spectrum_window(window, what):
    if window not in SPECTRUM_WINDOWS:
        raise ValueError(f'{what}: window must be one of {sorted(SPECTRUM_WINDOWS)}, got {window!r}')
    return window


def _spectrum_profiles(x, res, window, chunk):
    """The (N, res / 2 + 1) per-image profiles of ``x``, walked ``chunk`` images at a time through one scratch."""
    n = int(x.shape[0])
    ws = spectrum_workspace(n, res, x.device)
    scratch = spectrum_scratch(chunk, res, x.device)
    for off in range(0, n, chunk):
        spectrum_feed(x[off:off + chunk], res, window, scratch, ws, off, n)
    return ws


def spectrum_profile_mean(x, window='hann', chunk=None):
    """The set profile ``S`` of a (N, 3, R, R) fp32 batch: a (R/2 + 1,) fp64 device tensor (the images in index order; no host
    read).  No autograd."""
    window = _spectrum_window(window, 'spectrum_profile_mean')
    x, res = _spectrum_batch(x.detach() if isinstance(x, torch.Tensor) else x, 'spectrum_profile_mean x')
    n = int(x.shape[0])
    ws = _spectrum_profiles(x, res, window, _spectrum_chunk(res, n, chunk))
    out = torch.empty(res // 2 + 1, dtype=torch.float64, device=x.device)
    check(_lib.lib().ganlab_spectrum_reg_target_f64(_p(ws), ws.numel() * 8, n, res, 0.0, 1, _p(out), _st()), 'spectrum_reg_target')
    return out


def spectrum_target_update(x, target, decay, first, window='hann', chunk=None):
    """``target <- decay target + (1 - decay) S(x)`` in place (``first``: ``target <- S(x)``), one small kernel behind the
    profiles; no host read.  What ``SpectrumRegulariser.observe`` runs in the critic step (DESIGN.md 4.9b lists it with the ops)."""
    window = _spectrum_window(window, 'spectrum_target_update')
    x, res = _spectrum_batch(x.detach() if isinstance(x, torch.Tensor) else x, 'spectrum_target_update x')
    target = _ct(target, torch.float64, 'spectrum_target_update target')
    if not target.is_contiguous() or tuple(target.shape) != (res // 2 + 1,):
        raise ValueError(f'spectrum_target_update: target must be a contiguous ({res // 2 + 1},) tensor, got {tuple(target.shape)}')
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError(f'spectrum_target_update: decay must be in [0, 1), got {decay!r}')
    n = int(x.shape[0])
    ws = _spectrum_profiles(x, res, window, _spectrum_chunk(res, n, chunk))
    check(_lib.lib().ganlab_spectrum_reg_target_f64(_p(ws), ws.numel() * 8, n, res, float(decay), 1 if first else 0, _p(target),
                                                    _st()), 'spectrum_reg_target')
    return target


class _SpectrumLossBwd(torch.autograd.Function):
    """The gradients ``_SpectrumLoss.backward`` computed, tied to its inputs: differentiating them - a second differentiation of the
    loss - raises by the op's name."""

    @staticmethod
    def forward(ctx, x, gout, gx):
        return gx.view_as(gx)

    @staticmethod
    def backward(ctx, gg):
        raise RuntimeError('gan_lab_amd.ops.spectrum_loss is first order only: its backward was asked to differentiate twice (no '
                           'double backward is provided; keep it out of create_graph=True penalties)')


class _SpectrumLoss(torch.autograd.Function):
    """L(S(x), T) -> 0-dim fp32; the backward recomputes the half spectrum chunk by chunk (nothing but ``x`` and R/2 + 1 doubles is
    kept between the two)."""

    @staticmethod
    def forward(ctx, x, target, band, window, chunk):
        res, n = int(x.shape[2]), int(x.shape[0])
        ws = _spectrum_profiles(x, res, window, chunk)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        coef = torch.empty(res // 2 + 1, dtype=torch.float64, device=x.device)
        check(_lib.lib().ganlab_spectrum_reg_finish_f64(_p(ws), ws.numel() * 8, n, res, SPECTRUM_WINDOWS[window],
                                                        SPECTRUM_BANDS[band], _p(target), _p(loss), _p(coef), _st()),
              'spectrum_reg_finish')
        ctx.save_for_backward(x, coef)
        ctx.window, ctx.chunk = window, chunk
        return loss

    @staticmethod
    def backward(ctx, gout):
        x, coef = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        res, n, chunk = int(x.shape[2]), int(x.shape[0]), ctx.chunk
        g = _c(gout.detach(), 'spectrum_loss cotangent')
        gx = torch.empty((n, 3, res, res), dtype=torch.float32, device=x.device)
        L = _lib.lib()
        nbytes = L.ganlab_spectrum_reg_scratch(chunk, res)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        stride = x.stride(0) if n > 1 else 3 * res * res
        xd = x.detach()
        for off in range(0, n, chunk):
            count = min(chunk, n - off)
            check(L.ganlab_spectrum_reg_backward_f32(_p(xd[off:off + count]), stride, count, res, SPECTRUM_WINDOWS[ctx.window],
                                                     _p(coef), _p(g), _p(gx[off:off + count]), _p(scratch), scratch.numel() * 8,
                                                     _st()), 'spectrum_reg_backward')
        if torch.is_grad_enabled():
            gx = _SpectrumLossBwd.apply(x, gout, gx)
        return gx, None, None, None, None


def spectrum_loss(x, target, band='all', window='hann', chunk=None):
    """``mean_{k in band} (ln max(S[k], 1e-30) - ln max(target[k], 1e-30))^2`` of the set profile S of the (N, 3, R, R) fp32 batch
    ``x`` against the (R/2 + 1,) fp64 device profile ``target``: a 0-dim fp32 device tensor.  ``band``: 'all' (k = 1 .. R/2) or
    'hf' (k = R/4+1 .. R/2).  Differentiable ONCE in ``x`` (a second differentiation raises); ``target`` gets no gradient and is
    not written.  ``chunk``: images per pass through the scratch (None: as many as 64 MiB of half spectra hold)."""
    window = _spectrum_window(window, 'spectrum_loss')
    if band not in SPECTRUM_BANDS:
        raise ValueError(f'spectrum_loss: band must be one of {sorted(SPECTRUM_BANDS)}, got {band!r}')
    x, res = _spectrum_batch(x, 'spectrum_loss x')
    target = _ct(target, torch.float64, 'spectrum_loss target')
    if tuple(target.shape) != (res // 2 + 1,):
        raise ValueError(f'spectrum_loss: target must hold the {res // 2 + 1} bins of a {res} x {res} image, got '
                         f'{tuple(target.shape)}')
    return _SpectrumLoss.apply(x, target.detach(), band, window, _spectrum_chunk(res, int(x.shape[0]), chunk))
