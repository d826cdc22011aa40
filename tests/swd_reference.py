"""Float64 numpy restatement of the sliced Wasserstein distance between Laplacian-pyramid patch descriptors (Karras et al.
2018), step by step as DESIGN.md 4.7 defines it.  A test helper: plain numpy, no GPU, nothing of the package imported.

    pyramid      f = [1,4,6,4,1]/16; down = (f (x) f) with mirror boundary (numpy 'reflect'), then [::2, ::2];
                 up = zeros at the odd positions of a 2x grid, then (2f) (x) (2f) with mirror boundary;
                 lap[i] = gauss[i] - up(gauss[i+1]), last level gauss[-1]
    descriptors  7x7x3 neighbourhoods at given centres, rows of 147 in (channel, dy, dx) order
    normalise    per channel over ALL descriptors of a set: subtract the mean, divide by the population std
    project      on unit-norm directions
    distance     per direction mean |sort(a) - sort(b)|; mean over directions, then over repeats; x 1e3
"""
import numpy as np

F = np.array([1., 4., 6., 4., 1.]) / 16.


def filt(x, k):
    """Separable 5-tap filter ``k (x) k`` over the last two axes, mirror boundary (the edge sample is not repeated)."""
    k = np.asarray(k, dtype=x.dtype)
    h, w = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)], mode='reflect')
    t = sum(k[a] * p[..., a:a + h, :] for a in range(5))
    return sum(k[b] * t[..., :, b:b + w] for b in range(5))


def down(x):
    return filt(x, F)[..., ::2, ::2]


def up(x):
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]), dtype=x.dtype)
    z[..., ::2, ::2] = x
    return filt(z, 2. * F)


def laplacian_pyramid(x, min_res=16):
    gauss = [np.asarray(x)]
    while gauss[-1].shape[-1] > min_res:
        gauss.append(down(gauss[-1]))
    return [gauss[i] - up(gauss[i + 1]) for i in range(len(gauss) - 1)] + [gauss[-1]]


def reconstruct(pyramid):
    x = pyramid[-1]
    for band in pyramid[-2::-1]:
        x = band + up(x)
    return x


def descriptors(level, positions):
    """(N, 3, S, S) level, (N, n, 2) integer centres (y, x) in [3, S - 4] -> (N n, 147)."""
    level, positions = np.asarray(level), np.asarray(positions)
    n_img, n = positions.shape[:2]
    s = level.shape[-1]
    assert positions.min() >= 3 and positions.max() <= s - 4
    img = np.arange(n_img)[:, None, None, None, None]
    ch = np.arange(3)[None, None, :, None, None]
    yy = positions[:, :, 0][:, :, None, None, None] + np.arange(-3, 4)[None, None, None, :, None]
    xx = positions[:, :, 1][:, :, None, None, None] + np.arange(-3, 4)[None, None, None, None, :]
    return level[img, ch, yy, xx].reshape(n_img * n, 147)


def channel_stats(desc):
    d = np.asarray(desc, dtype=np.float64).reshape(-1, 3, 49)
    return d.mean(axis=(0, 2)), d.std(axis=(0, 2))


def normalise(desc):
    d = np.asarray(desc).reshape(-1, 3, 49)
    mean = d.mean(axis=(0, 2), keepdims=True)
    std = d.std(axis=(0, 2), keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        return ((d - mean) / std).reshape(-1, 147)


def directions(rng, repeats, per_repeat):
    d = rng.standard_normal((repeats, per_repeat, 147))
    return d / np.sqrt((d * d).sum(axis=2, keepdims=True))


def sliced_distance(a, b, dirs):
    """a, b: normalised (M, 147) descriptors; dirs: (repeats, per_repeat, 147) unit vectors."""
    reps = []
    for d in dirs:
        pa, pb = np.sort(a @ d.T, axis=0), np.sort(b @ d.T, axis=0)
        reps.append(np.abs(pa - pb).mean(axis=0).mean())
    return float(np.mean(reps))


def swd(real, fake, positions, dirs, min_res=16):
    """real, fake: (N, 3, R, R); positions: one (N, n, 2) array per level, used for BOTH sets; dirs as above.
    Returns {'levels', 'swd', 'mean'} like ``SlicedWasserstein.result()``."""
    pr, pf = laplacian_pyramid(real, min_res), laplacian_pyramid(fake, min_res)
    out = [1e3 * sliced_distance(normalise(descriptors(a, p)), normalise(descriptors(b, p)), dirs)
           for a, b, p in zip(pr, pf, positions)]
    return {'levels': [lv.shape[-1] for lv in pr], 'swd': out, 'mean': float(np.mean(out))}


def sample_images(n, res, seed, smooth=0):
    """The tests' image distribution, float32 in roughly [-1, 1]: band-limited noise plus white noise ('smooth + noise');
    ``smooth`` extra f (x) f passes give the shifted distribution of the discrimination check."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 3, res, res), dtype=np.float32)
    low = filt(filt(rng.standard_normal((n, 3, res, res), dtype=np.float32), F), F)
    x = 0.15 * x + 1.6 * low
    for _ in range(smooth):
        x = filt(x, F)
    return np.ascontiguousarray(x, dtype=np.float32)
