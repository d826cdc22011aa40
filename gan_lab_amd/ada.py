"""Adaptive discriminator augmentation (Karras et al., "Training Generative Adversarial Networks with Limited Data",
NeurIPS 2020): every critic input, real and generated, goes through a random affine warp and a random color matrix whose
elementary transforms each fire with probability p, and a controller moves p from the overfitting signal
r_t = E[sign(D(real))].

A policy is a comma-separated subset of ``blit``, ``geom``, ``color``, in that order and each at most once.  The kernels are
csrc/ada.hip (DESIGN.md "ADA"); the parameters of a batch are (N, 32) rows drawn from the device Philox stream
(``rng.ada_params``) at the p held in a small device block, which the controller kernel updates: the host never reads it in
a step, so captured step graphs replay it."""
import torch

from . import ops, rng

BLIT, GEOM, COLOR = 1, 2, 4
PARTS = (('blit', BLIT), ('geom', GEOM), ('color', COLOR))
ROW = ops.ADA_ROW


def parse_policy(policy):
    """'blit,geom,color' -> bit mask.  Any other spelling, a repeated part or a part out of order raises ValueError."""
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
        return rng.ada_params(n, h, w, self.state, self.mask, device)

    def __call__(self, x, params=None):
        if params is None:
            params = self.draw(x.shape[0], x.shape[2], x.shape[3], x.device)
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
