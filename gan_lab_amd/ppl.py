"""Perceptual path length (Karras et al. 2019, the StyleGAN paper's metric of how smooth and disentangled a latent space is), on
the GPU (csrc/ppl.hip): the mean, over random pairs of latents, of

  d(G(path(t)), G(path(t + epsilon))) / epsilon^2

``path`` the spherical interpolation between two latents z (``space='z'``) or the linear one between their images in W (``'w'``),
``t`` uniform in [0, 1) (``sampling='full'``) or 0 (``'end'``), after the distances outside the 1st .. 99th percentile are dropped,
as the StyleGAN evaluation code drops them.

The paper's ``d`` is LPIPS, a pretrained network this package does not ship.  Here ``d`` is ``ops.pyramid_mse`` - the multi-scale
mean squared error in the network's image space that projection uses - or, with ``embed``, the squared Euclidean distance between
rows of any embedding the caller supplies (feed VGG features and the number is PPL proper).  Numbers are comparable between
runs of one ``d`` only.

Per batch of B pairs there is ONE generator call on the 2B rows ``[points at t; points at t + epsilon]``: both ends of a pair
run through the same kernels of the same launch.  The distance of a pair is ~epsilon^2 of the image's energy, so two launches
that chose their kernels by batch size would add rounding of the size of the signal.  The end points, the distances and the
trimmed mean stay on the device; the host reads back one record of five doubles per evaluation.

Everything random - the latents, the ``t`` draws, the per-layer noise maps - is a pure function of ``seed``; the process's training
stream (gan_lab_amd/rng.py) is not touched.
"""
import torch

from . import ops
from ._metric_common import wanted as _wanted

SPACES = ('z', 'w')
SAMPLINGS = ('full', 'end')
MODES = ('lerp', 'slerp')
_MASK = 2 ** 64 - 1
_MAP_CHUNK = 4096             # latents per mapping-network call (space 'w')


def _substream(seed, k):
    """Philox key of sub-stream k (0: the latents, 1: the ``t`` draws, 2: the noise maps) of an evaluation seeded with ``seed``
    (``project._substream``'s construction under this module's own tag)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + (int(k) + 1) * 0xD1B54A32D192ED03 + 0x50504C) & _MASK


def wanted(metrics):
    return _wanted(metrics, 'ppl')


def check_samples(n, what='n_samples'):
    if isinstance(n, bool) or not isinstance(n, int) or n < 2:
        raise ValueError(f'ppl: {what} must be an integer >= 2 (got {n!r})')
    return n


def check_seed(seed, what='seed'):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError(f'ppl: {what} must be an integer in [0, 2**63) (got {seed!r})')
    return seed


def check_sampling(sampling, what='sampling'):
    if sampling not in SAMPLINGS:
        raise ValueError(f"ppl: {what} must be 'full' or 'end' (got {sampling!r})")
    return sampling


def check_trim(trim):
    """``trim`` = (low, high) percentiles as the two quantiles ``ops.trimmed_mean`` takes (percent / 100, numpy's division)."""
    try:
        lo, hi = (float(v) for v in trim)
    except (TypeError, ValueError):
        raise ValueError(f'ppl: trim must be a pair of percentiles (got {trim!r})') from None
    if not 0.0 <= lo <= hi <= 100.0:
        raise ValueError(f'ppl: trim must satisfy 0 <= low <= high <= 100 (got {trim!r})')
    return lo / 100.0, hi / 100.0


def validate_config(config):
    """Called when a progressive learner is built: the ``ppl_*`` fields are checked whether or not the metric is requested, and
    'ppl' is refused among the critic's metrics.  Returns (samples, space, sampling, epsilon, seed), ``space`` resolved: None means
    'w' for StyleGAN and 'z' for ProGAN, which has no W."""
    samples = check_samples(getattr(config, 'ppl_samples', 1024), 'ppl_samples')
    style = getattr(config, 'model', 'StyleGAN') == 'StyleGAN'
    space = getattr(config, 'ppl_space', None)
    if space is not None and space not in SPACES:
        raise ValueError(f"ppl: ppl_space must be 'z', 'w' or None (got {space!r})")
    if space == 'w' and not style:
        raise ValueError(f"ppl: ppl_space='w' needs a mapping network; {getattr(config, 'model', None)} has none (use 'z')")
    if space is None:
        space = 'w' if style else 'z'
    sampling = check_sampling(getattr(config, 'ppl_sampling', 'full'), 'ppl_sampling')
    epsilon = ops.check_ppl_epsilon(getattr(config, 'ppl_epsilon', 1e-4), 'ppl: ppl_epsilon')
    seed = check_seed(getattr(config, 'ppl_seed', 0), 'ppl_seed')
    if wanted(getattr(config, 'disc_metrics', None)):
        raise ValueError("config.disc_metrics lists 'ppl': the perceptual path length is a generator metric (config.gen_metrics)")
    return samples, space, sampling, epsilon, seed


def path_length(synth, latents_a, latents_b, mode, sampling='full', epsilon=1e-4, batch=16, weights=None, embed=None,
                trim=(1, 99), seed=0):
    """The path length of ``synth`` - any callable from (B, D) latents to (B, C, R, R) images - between the rows of ``latents_a``
    and ``latents_b`` (n, D), ``mode`` 'lerp' or 'slerp' (``ops.ppl_endpoints``).

    Pairs go in batches of ``batch``; per batch ``synth`` is called ONCE on the 2B rows ``[points at t; points at t + epsilon]``.
    The distance of a pair is ``ops.pyramid_mse`` of its two images under ``weights`` (None: every level the resolution allows,
    weight 1) or, with ``embed``, ``ops.row_sqdist`` of the rows ``embed(images)`` flattened.  ``t`` of pair i is draw i of the
    sub-stream 1 of ``seed``, whatever the batch size.  Returns ``{'ppl', 'lo', 'hi', 'kept', 'distances'}``: ``distances`` the
    raw (n,) device tensor, ``lo`` / ``hi`` its ``trim`` percentiles ('lower' / 'higher'), ``kept`` the number within them,
    ``ppl`` their float64 mean over ``epsilon^2`` (NaN if a distance is not finite)."""
    if mode not in MODES:
        raise ValueError(f"ppl: mode must be 'lerp' or 'slerp' (got {mode!r})")
    check_sampling(sampling)
    eps = ops.check_ppl_epsilon(epsilon, 'ppl: epsilon')
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError(f'ppl: batch must be an integer >= 1 (got {batch!r})')
    q_lo, q_hi = check_trim(trim)
    check_seed(seed)
    a, b = ops._c(latents_a, 'ppl latents_a'), ops._c(latents_b, 'ppl latents_b')
    if a.dim() != 2 or a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f'ppl: latents_a and latents_b must be equal (n, D) matrices (got {tuple(a.shape)} and {tuple(b.shape)})')
    n, d = a.shape
    key = _substream(seed, 1)
    distances = torch.empty(n, dtype=torch.float32, device=a.device)
    with torch.no_grad():
        for i0 in range(0, n, batch):
            k = min(batch, n - i0)
            _, ends = ops.ppl_endpoints(a[i0:i0 + k], b[i0:i0 + k], eps, mode, sampling, key, i0)
            x = synth(ends.view(2 * k, d))
            if not isinstance(x, torch.Tensor) or x.dim() < 2 or x.shape[0] != 2 * k:
                raise ValueError(f'ppl: synth must return {2 * k} images for {2 * k} latents (got '
                                 f'{tuple(getattr(x, "shape", ()))})')
            if embed is None:
                if x.dim() != 4:
                    raise ValueError(f'ppl: synth must return (B, C, R, R) images (got {tuple(x.shape)})')
                w = (1.0,) * ops.pyramid_max_levels(int(x.shape[2])) if weights is None else weights
                dist, _ = ops.pyramid_mse(x[:k], x[k:], w)
                distances[i0:i0 + k].copy_(dist)
            else:
                e = embed(x)
                if not isinstance(e, torch.Tensor) or e.dim() < 2 or e.shape[0] != 2 * k:
                    raise ValueError(f'ppl: embed must return {2 * k} rows for {2 * k} images (got '
                                     f'{tuple(getattr(e, "shape", ()))})')
                e = ops._c(e.flatten(1), 'ppl embedded rows')
                ops.row_sqdist(e[:k], e[k:], out=distances[i0:i0 + k])
        record = ops.trimmed_mean(distances, q_lo, q_hi).cpu().tolist()         # the evaluation's one host read
    mean, lo, hi, kept, _ = record
    return {'ppl': mean / (eps * eps), 'lo': lo, 'hi': hi, 'kept': int(kept), 'distances': distances}


def _latents(distribution, count, length, key, dev):
    """``count`` latents of ``distribution`` from the Philox key ``key`` alone."""
    if distribution == 'normal':
        return ops.randn((count, length), key, 0, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(key & (2 ** 63 - 1))
    return torch.rand(count, length, dtype=torch.float32, device=dev, generator=g)


def noise_maps(gen, key, batch_index, dev):
    """The per-layer (1, 1, h, w) noise maps of batch ``batch_index`` of an evaluation: one map per layer for every row of the
    batch - so for both ends of every pair -, the layers' maps one after the other in the Philox stream under ``key``, the batches
    one after the other behind them."""
    sides = [4 * 2 ** (k // 2) for k in range(len(gen.gen_layers))]
    per_batch = sum((s * s + 3) // 4 for s in sides)
    maps, offset = [], batch_index * per_batch
    for s in sides:
        maps.append(ops.randn((1, 1, s, s), key, offset, dev))
        offset += (s * s + 3) // 4
    return maps


class _StyleSynth(object):
    """``path_length``'s callable over a StyleGAN generator: z -> w -> image ('z') or w -> image ('w'), with the noise maps of the
    batch it is called for (calls come in batch order)."""

    def __init__(self, gen, space, key, dev):
        self.gen, self.space, self.key, self.dev, self.calls = gen, space, key, dev, 0

    def __call__(self, rows):
        maps = noise_maps(self.gen, self.key, self.calls, self.dev) if self.gen.use_noise else None
        self.calls += 1
        ws = self.gen.z_to_w(rows) if self.space == 'z' else rows
        return self.gen.synthesis(ws, noise=maps)


def generator_path_length(learner_or_gen, n_samples, space, sampling='full', epsilon=1e-4, batch=16, weights=None, embed=None,
                          trim=(1, 99), seed=0, time_average=None):
    """``path_length`` of a generator between ``n_samples`` pairs of its own latents.

    ``learner_or_gen``: a ProGAN / StyleGAN learner - the generator evaluated is the time-averaged one where the learner keeps one
    (``time_average=None``: ``config.use_ewma_gen``), else the live one - or a ``ProGenerator`` / ``StyleGenerator`` itself.
    ``space='z'``: spherical interpolation of the latents, then the generator (for StyleGAN ``z_to_w`` then ``synthesis``);
    ``space='w'`` (StyleGAN only): ``z_to_w`` of both ends, linear interpolation, then ``synthesis`` with the one dlatent for all
    layers.  The generator runs in eval mode, without truncation and mixing; its per-layer noise maps are drawn once per batch
    and shared by both ends of every pair (``noise_maps``).  Latents 0 .. n-1 of sub-stream 0 of ``seed`` are the paths' starts,
    n .. 2n-1 their ends; the ``t`` draws are sub-stream 1, the noise maps sub-stream 2.

    Nothing of the learner changes: module modes, the noise / mixing switches, ``requires_grad`` flags, ``w_ewma``, the EWMA copy
    and the training random stream are as found afterwards.  Not available while a resolution fades in."""
    from . import rng
    from .progan.architectures import ProGenerator
    from .stylegan.architectures import StyleGenerator
    learner = None
    if isinstance(learner_or_gen, (ProGenerator, StyleGenerator)):
        gen = live = learner_or_gen
    else:
        learner = learner_or_gen
        live = getattr(learner, 'gen_model', None)
        if not isinstance(live, (ProGenerator, StyleGenerator)):
            raise TypeError('ppl: needs a ProGAN / StyleGAN learner or generator')
    style = isinstance(live, StyleGenerator)
    check_samples(n_samples)
    if space not in SPACES:
        raise ValueError(f"ppl: space must be 'z' or 'w' (got {space!r})")
    if space == 'w' and not style:
        raise ValueError("ppl: space='w' needs a mapping network; ProGAN has none (use 'z')")
    check_sampling(sampling)
    ops.check_ppl_epsilon(epsilon, 'ppl: epsilon')
    check_trim(trim)
    check_seed(seed)
    if live.fade_in_phase:
        raise ValueError('ppl: not available while fade_in_phase is set (the image then blends two resolutions)')

    kept_lagged = None
    if learner is not None:
        if time_average is None:
            time_average = bool(learner.config.use_ewma_gen)
        kept_lagged = learner.gen_model_lagged
        if time_average and kept_lagged is None:
            learner.materialize_lagged_generator().to(learner.config.dev)   # a private copy of the EWMA shadow: not kept
        gen = learner.gen_model_lagged if time_average else live
        learner.gen_model_lagged = kept_lagged
    dev = next(gen.parameters()).device
    distribution = getattr(gen, 'latent_distribution', None) or getattr(learner, 'latent_distribution', 'normal')

    modes = [(mod, mod.training) for mod in gen.modules()]
    switches = (gen._use_noise, gen._use_mixing_reg, gen.use_truncation_trick, gen.w_ewma) if style else None
    flags = [(p, p.requires_grad) for p in gen.parameters()]
    stream = rng._STATE['offset']
    try:
        gen.eval()
        if style:
            gen.use_truncation_trick = False
        for p, _ in flags:
            p.requires_grad_(False)
        with torch.no_grad():
            z = _latents(distribution, 2 * n_samples, gen.len_latent, _substream(seed, 0), dev)
            if space == 'w':
                z = torch.cat([gen.z_to_w(z[i:i + _MAP_CHUNK]) for i in range(0, len(z), _MAP_CHUNK)])
            synth = _StyleSynth(gen, space, _substream(seed, 2), dev) if style else gen
            return path_length(synth, z[:n_samples], z[n_samples:], 'lerp' if space == 'w' else 'slerp', sampling, epsilon,
                               batch, weights, embed, trim, seed)
    finally:
        rng._STATE['offset'] = stream
        for p, flag in flags:
            p.requires_grad_(flag)
        for mod, mode in modes:
            mod.training = mode
        if style:
            gen._use_noise, gen._use_mixing_reg, gen.use_truncation_trick, gen.w_ewma = switches
