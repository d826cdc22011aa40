"""Adaptive discriminator augmentation (Karras et al., "Training Generative Adversarial Networks with Limited Data",
NeurIPS 2020): every critic input, real and generated, goes through a random affine warp, a random color matrix, a random
band filter, additive noise and a cutout, whose elementary transforms each fire with probability p, and a controller moves p
from the overfitting signal r_t = E[sign(D(real))].

A policy is a comma-separated subset of ``blit``, ``geom``, ``color``, ``filter``, ``noise``, ``cutout``, in that order (the
order of application) and each at most once.  The kernels are csrc/ada.hip and csrc/ada_filter.hip (DESIGN.md "ADA"); the
parameters of a batch are (N, 32) rows drawn from the device Philox stream (``rng.ada_params``) at the p held in a small
device block, which the controller kernel updates: the host never reads it in a step, so captured step graphs replay it.
The last three groups add (N, 16) ``ext`` rows and, for noise, a field of normals to a draw (``ops.AdaDraw``); a policy without
them draws, launches and computes exactly what it did before they existed.

Strengths are the paper's: four filter bands, each gated at p with a log2-normal gain of std 1, noise std 0.1 |z|, cutout
size 0.5.  This project's addition: every normal is clamped to +-3 (as the geometric draws already are), which bounds the
sum of |h| over a drawn filter by 8.21, its value over the corners of the clamp."""
import torch

from . import ops, rng

BLIT, GEOM, COLOR = 1, 2, 4
FILTER, NOISE, CUTOUT = ops.ADA_FILTER, ops.ADA_NOISE, ops.ADA_CUTOUT
PARTS = (('blit', BLIT), ('geom', GEOM), ('color', COLOR), ('filter', FILTER), ('noise', NOISE), ('cutout', CUTOUT))
ROW, EXT_ROW = ops.ADA_ROW, ops.ADA_EXT_ROW


def parse_policy(policy):
    """'blit,geom,color' -> 7, 'blit,geom,color,filter,noise,cutout' -> 63: the bit mask.  Any other spelling, a repeated part
    or a part out of order raises ValueError."""
    if not isinstance(policy, str):
        raise ValueError(f'ADA policy must be a string such as "blit,geom,color", got {policy!r}')
    names = [name for name, _ in PARTS]
    mask, last = 0, -1
    for part in policy.split(','):
        if part not in names:
            raise ValueError(f'ADA policy {policy!r}: unknown part {part!r} (parts: {", ".join(names)})')
        k = names.index(part)
        if k <= last:
            raise ValueError(f'ADA policy {policy!r}: parts must appear at most once, in the order {",".join(names)}')
        mask |= PARTS[k][1]
        last = k
    return mask


def step_size(batch, world, interval, kimg):
    """How far one adjustment moves p: the images seen between two adjustments over ``kimg`` thousand, so that p can go from
    0 to 1 in ``kimg`` thousand images (the paper's rule)."""
    return batch * world * interval / (kimg * 1000.0)


def next_p(p, acc_sum, acc_n, target, step_size):
    """The controller's adjustment on the host, in fp32 like the kernel: p moves one ``step_size`` towards making
    acc_sum / acc_n equal ``target`` and is clamped to [0, 1]; no samples, no move."""
    import numpy as np
    f = np.float32
    p, step = f(p), f(step_size)
    if f(acc_n) <= 0:
        return float(p)
    d = f(acc_sum) / f(acc_n) - f(target)
    sgn = f(1) if d > 0 else f(-1) if d < 0 else f(0)
    return float(min(max(f(p + sgn * step), f(0)), f(1)))


def reduce_accumulators(state, group=None):
    """Sum ``acc_sum`` and ``acc_n`` (state[1:3]) over the process group, in place, so that every rank adjusts p from the same
    statistics.  A single process: nothing to do."""
    from . import parallel
    if parallel.is_dist():
        import torch.distributed as dist
        acc = state[1:3].clone()
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
        state[1:3].copy_(acc)
    return state


def rows_from_matrices(M, C=None):
    """(N, 32) parameter rows on the host from (N, 2, 3) maps ``M`` (output pixel -> source position, centred pixel units)
    and (N, 3, 4) color matrices ``C`` (identity when None): fills in G = M[:, :, :2]^-1, which the adjoint kernel needs.
    The gate and raw-draw columns stay zero."""
    M = torch.as_tensor(M, dtype=torch.float64).reshape(-1, 2, 3)
    n = M.shape[0]
    if C is None:
        C = torch.eye(3, 4, dtype=torch.float64).expand(n, 3, 4)
    C = torch.as_tensor(C, dtype=torch.float64).reshape(n, 3, 4)
    rows = torch.zeros(n, ROW, dtype=torch.float64)
    rows[:, 0:6] = M.reshape(n, 6)
    rows[:, 6:10] = torch.linalg.inv(M[:, :, :2]).reshape(n, 4)
    rows[:, 10:22] = C.reshape(n, 12)
    return rows.float()


def filter_bank():
    """The (4, 43) float64 filter bank of the ``filter`` group, by the official recipe: from the sym2 wavelet
    lo = [(1 - s), (3 - s), (3 + s), (1 + s)] / (4 sqrt 2), s = sqrt 3, and hi[k] = (-1)^k lo[k], the 7-tap
    lo2 = conv(lo, reversed lo) / 2 and hi2 likewise; start from F = eye(4, 1) and for i = 1, 2, 3 upsample every row by 2
    (zeros between, the last zero dropped), convolve every row with lo2 and add hi2 to the centre 7 taps of row i.  Row b is
    the impulse response of octave band b; the four rows sum to the unit impulse at tap 21.  The library holds its own copy
    (``ops.ada_filter_bank``)."""
    import numpy as np
    s = np.sqrt(3.0)
    lo = np.array([1 - s, 3 - s, 3 + s, 1 + s]) / (4 * np.sqrt(2.0))
    hi = lo * (-1.0) ** np.arange(4)
    lo2, hi2 = np.convolve(lo, lo[::-1]) / 2, np.convolve(hi, hi[::-1]) / 2
    bank = np.eye(4, 1)
    for i in range(1, 4):
        up = np.zeros((4, 2 * bank.shape[1]))
        up[:, ::2] = bank
        bank = np.stack([np.convolve(row, lo2) for row in up[:, :-1]])
        c = bank.shape[1] // 2
        bank[i, c - 3:c + 4] += hi2
    return torch.from_numpy(bank)


def ext_rows(g=None, sigma=None, rect=None, gates=None, n=None):
    """(N, 16) hand-made ``ext`` rows on the host: ``g`` (N, 4) band gains (None: ones), ``sigma`` (N,) noise scales (None:
    zeros), ``rect`` (N, 4) integer cutout rectangles (j0, j1, i0, i1) - columns [j0, j1), rows [i0, i1) - (None: empty).
    ``gates`` (N,) overrides the gate mask, which is otherwise: all four band bits where g differs from ones, bit 4 where
    sigma is not zero, bit 5 where the rectangle is not empty.  The kernels act on the mask: gains, sigma and rectangle
    behind a closed bit are ignored.  The raw-draw columns stay zero."""
    given = [torch.as_tensor(v).shape[0] for v in (g, sigma, rect, gates) if v is not None]
    n = int(n) if n is not None else (given[0] if given else 1)
    rows = torch.zeros(n, EXT_ROW, dtype=torch.float64)
    rows[:, 0:4] = 1.0 if g is None else torch.as_tensor(g, dtype=torch.float64).reshape(n, 4)
    if sigma is not None:
        rows[:, 4] = torch.as_tensor(sigma, dtype=torch.float64).reshape(n)
    if rect is not None:
        rows[:, 5:9] = torch.as_tensor(rect, dtype=torch.float64).reshape(n, 4)
    if gates is None:
        rows[:, 9] = 15.0 * (rows[:, 0:4] != 1.0).any(dim=1) + 16.0 * (rows[:, 4] != 0) + \
            32.0 * ((rows[:, 6] > rows[:, 5]) & (rows[:, 8] > rows[:, 7]))
    else:
        rows[:, 9] = torch.as_tensor(gates, dtype=torch.float64).reshape(n)
    return rows.float()


class AdaptiveAugment(object):
    """``aug = AdaptiveAugment('blit,geom,color', p=0.2, target=None); y = aug(x)`` - draws fresh rows unless ``params`` is
    given.  ``target`` None keeps p fixed; otherwise ``update(real_logits)`` after every critic pass accumulates
    sign(D(real)) and, every ``interval`` calls, moves p by ``step_size`` towards r_t = target - on the device."""

    def __init__(self, policy, p=0.0, target=0.6, interval=4, kimg=500, device='cuda'):
        self.policy = policy
        self.mask = parse_policy(policy)
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f'ADA probability must be in [0, 1], got {p!r}')
        if target is not None and (int(interval) < 1 or float(kimg) <= 0):
            raise ValueError(f'ADA needs ada_interval >= 1 and ada_kimg > 0, got {interval!r} and {kimg!r}')
        self.target = None if target is None else float(target)
        self.interval, self.kimg = int(interval), float(kimg)
        # (p, acc_sum, acc_n, calls): read by the parameter draw and rewritten by the controller kernel
        self.state = torch.tensor([float(p), 0.0, 0.0, 0.0], dtype=torch.float32, device=device)
        self._calls = None          # host copy of the call count, data parallel only

    @property
    def adaptive(self):
        return self.target is not None

    @property
    def p(self):
        """The current probability: a host read (a sync) - for logging and saving, never inside a step."""
        return float(self.state[0].item())

    def draw(self, n, h, w, device='cuda'):
        """What ``__call__`` takes as ``params``: the (n, 32) rows, or with a filter, noise or cutout group an ``ops.AdaDraw``
        (rows, ext rows, noise field), which slices along the batch like the rows do."""
        return rng.ada_params(n, h, w, self.state, self.mask, device)

    def __call__(self, x, params=None):
        if params is None:
            params = self.draw(x.shape[0], x.shape[2], x.shape[3], x.device)
        if isinstance(params, ops.AdaDraw):
            return ops.ada_augment(x, params.params, params.ext, params.noise)
        return ops.ada_augment(x, params)

    def update(self, real_logits):
        """Feed the critic's outputs on the (augmented) real batch of one D step to the controller."""
        from . import parallel
        if not self.adaptive:
            return
        logits = real_logits.detach().reshape(-1)
        world = parallel.world_size()
        step = step_size(logits.numel(), world, self.interval, self.kimg)
        if world == 1:
            ops.ada_update(self.state, logits, self.interval, step, self.target)
            return
        # data parallel (eager only): accumulate, and every ``interval`` calls sum the statistics over the ranks before the
        # adjustment; the call count is the same on every rank, so the host may keep it
        ops.ada_update(self.state, logits, 0, step, self.target)
        if self._calls is None:
            self._calls = int(self.state[3].item()) - 1       # once, after construction or a checkpoint load
        self._calls += 1
        if self._calls >= self.interval:
            reduce_accumulators(self.state)
            ops.ada_update(self.state, None, 1, step, self.target)
            self._calls = 0

    def state_dict(self):
        """The four state scalars as plain floats (a host read)."""
        p, acc_sum, acc_n, calls = (float(v) for v in self.state.detach().cpu().tolist())
        return dict(p=p, acc_sum=acc_sum, acc_n=acc_n, calls=calls)

    def load_state_dict(self, sd):
        with torch.no_grad():
            self.state.copy_(torch.tensor([float(sd[k]) for k in ('p', 'acc_sum', 'acc_n', 'calls')], dtype=torch.float32))
        self._calls = None

    def __repr__(self):
        return f'AdaptiveAugment({self.policy!r}, target={self.target!r}, interval={self.interval}, kimg={self.kimg:g})'


def from_config(config):
    """The learners' ADA: None (``config.ada`` is None) or an ``AdaptiveAugment`` on ``config.dev``.  ``ada`` together with
    ``diffaugment`` raises ValueError: both would augment the same critic inputs."""
    policy = getattr(config, 'ada', None)
    if policy is None:
        return None
    if getattr(config, 'diffaugment', None) is not None:
        raise ValueError('config.ada and config.diffaugment are both set: choose one augmentation of the critic inputs')
    return AdaptiveAugment(policy, p=getattr(config, 'ada_p', 0.0), target=getattr(config, 'ada_target', 0.6),
                           interval=getattr(config, 'ada_interval', 4), kimg=getattr(config, 'ada_kimg', 500),
                           device=config.dev)
