"""Flat parameter arenas + fused Adam / RMSprop / SGD / optimistic Adam / EWMA (K15) for the G and D parameter sets.

MI355X-first layout: all parameters of a network live in ONE contiguous fp32 buffer (and all
gradients in another), so that
  * the optimiser step is one kernel launch per contiguous run instead of ~100 small ones
    (reference: torch.optim.Adam(betas=(0,.99)) built by backprop_utils.py:109-120 and re-created at
    every phase boundary, progan/learner.py:1064-1095),
  * the EWMA generator update (progan/learner.py:909-916) is one launch,
  * the data-parallel gradient exchange is a handful of large RCCL all-reduces over the flat
    gradient buffer (parallel.py) rather than one per tensor.
Parameters stay ordinary ``nn.Parameter`` objects (views into the arena), so ``state_dict()``,
``named_parameters()`` and checkpoints are unchanged.
"""
from collections import OrderedDict

import torch

from . import ops

_ALIGN = 4  # floats (16 B): keeps every parameter view 16-byte aligned for float4 kernels


def _round_up(n, m):
    return (n + m - 1) // m * m


class ParamArena(object):
    """Re-homes the given named parameters into one flat buffer (+ one flat grad buffer)."""

    def __init__(self, named_params, device=None):
        self.names, self.params, self.offsets, self.sizes = [], [], [], []
        named_params = [(k, p) for k, p in named_params]
        if not named_params:
            raise ValueError('empty parameter list')
        device = device if device is not None else named_params[0][1].device
        off = 0
        for k, p in named_params:
            self.names.append(k)
            self.params.append(p)
            self.offsets.append(off)
            self.sizes.append(p.numel())
            off += _round_up(p.numel(), _ALIGN)
        self.total = off
        self.serial = 0          # bumped by zero_grad(): ops.direct_param_grads writes each slot once per step
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.gflat = torch.zeros(off, dtype=torch.float32, device=device)
        with torch.no_grad():
            for p, o, n in zip(self.params, self.offsets, self.sizes):
                self.flat[o:o + n].copy_(p.detach().reshape(-1))
        self.attach()

    def attach(self):
        """(Re-)point every parameter's data and grad at its arena slot."""
        for p, o, n in zip(self.params, self.offsets, self.sizes):
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.gflat[o:o + n].view(p.shape)
            p._ganlab_arena = self

    def is_attached(self):
        base, gbase = self.flat.data_ptr(), self.gflat.data_ptr()
        for p, o in zip(self.params, self.offsets):
            if p.data_ptr() != base + 4 * o or p.grad is None or p.grad.data_ptr() != gbase + 4 * o:
                return False
        return True

    def reabsorb(self):
        """Parameters were re-allocated behind our back (e.g. ``model.to('cpu')`` and back for a
        checkpoint, progan/learner.py:962-985): copy their values in and re-attach."""
        with torch.no_grad():
            for p, o, n in zip(self.params, self.offsets, self.sizes):
                if p.data_ptr() != self.flat.data_ptr() + 4 * o:
                    self.flat[o:o + n].copy_(p.detach().reshape(-1).to(self.flat.device))
        self.attach()

    def zero_grad(self):
        self.gflat.zero_()
        self.serial += 1
        if not self.is_attached():
            self.reabsorb()

    def slot(self, name):
        i = self.names.index(name)
        return self.offsets[i], self.sizes[i]

    def views_of(self, flat):
        return OrderedDict((k, flat[o:o + n].view(p.shape))
                           for k, p, o, n in zip(self.names, self.params, self.offsets, self.sizes))


class _FusedArenaOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the maximal runs of parameters that are adjacent in memory (one launch each - one for an
    arena-backed network), the per-run state buffers a subclass declares, their carry across a re-layout, their export / import as
    plain data, and the step-graph protocol of graphs.GraphedStep (``dev_scalars`` / ``host_scalars``).  Parameters whose ``grad``
    is None are skipped, like torch.

    A subclass sets ``NAME`` (the ``config.optimizer`` value), ``STATE`` - ((run key, checkpoint key), ...) of its buffers, the
    checkpoint keys being torch's own state names where they exist -, and implements ``_step_scalars`` and ``_launch``."""

    NAME = None
    STATE = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._runs = None
        self._sig = None
        # step-graph capture (graphs.GraphedStep): device address of this optimiser's three per-step floats; while set, step()
        # launches the kernel that reads them there and leaves the step count to host_scalars()
        self.dev_scalars = None

    # -- what a subclass defines ---------------------------------------------------------------------------------------------
    def _active(self, group):
        """The (run key, checkpoint key) pairs of the buffers this group's update reads (all of ``STATE`` by default)."""
        return self.STATE

    def _step_scalars(self, group, t):
        """The three floats of step ``t`` (1-based) that change from step to step: what the ``_dev`` kernel reads."""
        raise NotImplementedError

    def _launch(self, group, run, pv, gv, scalars):
        """One launch over a run; ``scalars``: ``_step_scalars`` of this step, or None to read them at ``dev_scalars``."""
        raise NotImplementedError

    # -- shared --------------------------------------------------------------------------------------------------------------
    def host_scalars(self, advance=True):
        """The per-step floats of the NEXT step of the (single) parameter group, advancing its step count: what ``step()``
        computes on the host, for a replayed step."""
        group = self.param_groups[0]
        cached = self.state.get('_fused', {}).get(id(group))
        if cached is None:
            raise RuntimeError('host_scalars() before the first eager step()')
        if advance:
            cached['step'] += 1
        return self._step_scalars(group, cached['step'])

    def _build_runs(self, params):
        items = sorted(((p.data_ptr(), p) for p in params), key=lambda t: t[0])
        runs, cur = [], None
        for ptr, p in items:
            n = p.numel()
            gptr = p.grad.data_ptr()
            if cur is not None:
                gap = (ptr - cur['end']) // 4
                ggap = (gptr - cur['gend']) // 4
                if 0 <= gap < _ALIGN and gap == ggap and (ptr - cur['end']) % 4 == 0:
                    cur['params'].append(p)
                    cur['end'] = ptr + 4 * n
                    cur['gend'] = gptr + 4 * n
                    continue
            cur = dict(params=[p], start=ptr, end=ptr + 4 * n, gstart=gptr, gend=gptr + 4 * n)
            runs.append(cur)
        for r in runs:
            r['n'] = (r['end'] - r['start']) // 4
            r['offs'] = {id(p): (p.data_ptr() - r['start']) // 4 for p in r['params']}
        return runs

    def _new_state(self, group, run):
        dev = run['params'][0].device
        for key, _ in self._active(group):
            run[key] = torch.zeros(run['n'], dtype=torch.float32, device=dev)

    @torch.no_grad()
    def step(self, closure=None):
        touched = []
        if self.dev_scalars is not None and len(self.param_groups) != 1:
            # host_scalars() describes ONE (lr, step count): a replayed multi-group optimiser would train every group with
            # group 0's.  graphs.GraphedStep only captures the learners' single-group optimisers.
            raise RuntimeError(f'{type(self).__name__}.dev_scalars (step-graph capture) supports exactly one parameter group')
        for group in self.param_groups:
            params = [p for p in group['params'] if p.grad is not None]
            if not params:
                continue
            sig = tuple((p.data_ptr(), p.grad.data_ptr()) for p in params)
            st = self.state.setdefault('_fused', {})
            key = id(group)
            cached = st.get(key)
            if cached is None or cached['sig'] != sig:
                runs = self._build_runs(params)
                old = cached
                cached = dict(sig=sig, runs=runs, step=old['step'] if old else 0)
                for r in runs:
                    self._new_state(group, r)
                    if old is not None:  # carry the state across a re-layout
                        self._carry(old, r)
                st[key] = cached
            scalars = None
            if self.dev_scalars is None:
                cached['step'] += 1
                scalars = self._step_scalars(group, cached['step'])
            for r in cached['runs']:
                p0 = r['params'][0]
                # raw views over the whole run (padding floats have zero grad -> stay zero)
                pv = torch.as_strided(p0.data.reshape(-1), (r['n'],), (1,))
                gv = torch.as_strided(p0.grad.reshape(-1), (r['n'],), (1,))
                self._launch(group, r, pv, gv, scalars)
                touched.append((r['start'], r['end']))
        # packed conv weights inside the rewritten memory are stale: they are re-packed (all of them, one launch) at
        # their next use; the other network's stay valid
        if touched:
            ops.bump_weight_epoch(touched)

    def _carry(self, old, run):
        """Copy the state of parameters that survive a re-layout (keyed by parameter object)."""
        for p in run['params']:
            for r in old['runs']:
                o = r['offs'].get(id(p))
                if o is not None:
                    n, no = p.numel(), run['offs'][id(p)]
                    for key, _ in self.STATE:
                        if key in run and key in r:
                            run[key][no:no + n].copy_(r[key][o:o + n])

    def export_moments(self, named_params):
        """Plain-data optimiser state for checkpoints: {'step', <checkpoint key>: {name: tensor}, ...}, one map per buffer."""
        out = dict(step=0, **{ck: {} for _, ck in self.STATE})
        for group in self.param_groups:
            cached = self.state.get('_fused', {}).get(id(group))
            if cached is None:
                continue
            out['step'] = cached['step']
            for name, p in named_params:
                for r in cached['runs']:
                    o = r['offs'].get(id(p))
                    if o is not None:
                        for key, ck in self.STATE:
                            if key in r:
                                out[ck][name] = r[key][o:o + p.numel()].view(p.shape).detach().cpu().clone()
        return out

    @torch.no_grad()
    def import_moments(self, named_params, saved):
        """Inverse of export_moments (parameters must already have their arena-backed grads)."""
        named_params = list(named_params)
        missing = [ck for _, ck in self.STATE if ck not in saved]
        if missing or 'step' not in saved:
            raise ValueError(f"optimizer state of a checkpoint does not belong to optimizer='{self.NAME}': it holds "
                             f"{sorted(k for k in saved)}, '{self.NAME}' keeps {['step'] + [ck for _, ck in self.STATE]} "
                             f"(saved under optimizer='{optimizer_of_state(saved)}'?)")
        for group in self.param_groups:
            params = [p for p in group['params'] if p.grad is not None]
            runs = self._build_runs(params)
            for r in runs:
                self._new_state(group, r)
            for name, p in named_params:
                for r in runs:
                    o = r['offs'].get(id(p))
                    if o is not None:
                        for key, ck in self.STATE:
                            if key in r and name in saved[ck]:
                                r[key][o:o + p.numel()].copy_(saved[ck][name].reshape(-1))
            self.state.setdefault('_fused', {})[id(group)] = dict(
                sig=tuple((p.data_ptr(), p.grad.data_ptr()) for p in params), runs=runs, step=int(saved['step']))

    def zero_grad(self, set_to_none=False):
        # keep the arena-backed .grad views alive: zero in place
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is not None:
                    p.grad.zero_()


def _check_common(lr, eps=None, weight_decay=0):
    if not 0.0 <= lr:
        raise ValueError(f'Invalid learning rate: {lr}')
    if eps is not None and not 0.0 < eps:
        raise ValueError(f'Invalid epsilon value: {eps} (the fused kernels need eps > 0: padding floats divide 0 by eps)')
    if not 0.0 <= weight_decay:
        raise ValueError(f'Invalid weight_decay value: {weight_decay}')


class FusedAdam(_FusedArenaOptimizer):
    """torch.optim.Adam semantics (no amsgrad; L2 weight decay) with the update done by the HIP
    kernel ``ganlab_adam_f32`` over maximal runs of parameters that are adjacent in memory - one
    launch for an arena-backed network.  Parameters whose ``grad`` is None are skipped, like torch."""

    NAME = 'adam'
    STATE = (('m', 'exp_avg'), ('v', 'exp_avg_sq'))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)

    def _step_scalars(self, group, t):
        """(lr, 1 - beta1^t, 1 - beta2^t)."""
        b1, b2 = group['betas']
        return float(group['lr']), 1 - b1 ** t, 1 - b2 ** t

    def _launch(self, group, r, pv, gv, scalars):
        b1, b2 = group['betas']
        if scalars is None:
            ops.adam_step_dev(pv, gv, r['m'], r['v'], self.dev_scalars, b1, b2, group['eps'], group['weight_decay'])
        else:
            ops.adam_step(pv, gv, r['m'], r['v'], group['lr'], b1, b2, group['eps'], group['weight_decay'], scalars[1],
                          scalars[2])


class FusedOptimisticAdam(_FusedArenaOptimizer):
    """Optimistic Adam (Daskalakis et al. 2018, "Training GANs with Optimism", Algorithm 1): Adam's moments and bias corrections,
    ``p -= 2 lr d_t - lr d_{t-1}`` with ``d`` Adam's direction; ``d_0 = 0``, so the first step is twice Adam's.  One launch of
    ``ganlab_oadam_f32`` per run."""

    NAME = 'oadam'
    STATE = (('m', 'exp_avg'), ('v', 'exp_avg_sq'), ('prev', 'prev_dir'))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        _check_common(lr, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    _step_scalars = FusedAdam._step_scalars

    def _launch(self, group, r, pv, gv, scalars):
        b1, b2 = group['betas']
        if scalars is None:
            ops.oadam_step_dev(pv, gv, r['m'], r['v'], r['prev'], self.dev_scalars, b1, b2, group['eps'], group['weight_decay'])
        else:
            ops.oadam_step(pv, gv, r['m'], r['v'], r['prev'], group['lr'], b1, b2, group['eps'], group['weight_decay'],
                           scalars[1], scalars[2])


class FusedRMSprop(_FusedArenaOptimizer):
    """torch.optim.RMSprop semantics (``centered=False``; L2 weight decay; ``eps`` outside the root) by ``ganlab_rmsprop_f32``,
    one launch per run.  The momentum buffer exists only with ``momentum`` > 0."""

    NAME = 'rmsprop'
    STATE = (('sq', 'square_avg'), ('buf', 'momentum_buffer'))

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0):
        _check_common(lr, eps, weight_decay)
        if not 0.0 <= alpha:
            raise ValueError(f'Invalid alpha value: {alpha}')
        if not 0.0 <= momentum:
            raise ValueError(f'Invalid momentum value: {momentum}')
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum))

    def _active(self, group):
        return self.STATE if group['momentum'] > 0 else self.STATE[:1]

    def _step_scalars(self, group, t):
        """(lr, 0, 0): RMSprop has no other per-step scalar."""
        return float(group['lr']), 0.0, 0.0

    def _launch(self, group, r, pv, gv, scalars):
        rest = (group['alpha'], group['eps'], group['weight_decay'], group['momentum'])
        if scalars is None:
            ops.rmsprop_step_dev(pv, gv, r['sq'], r.get('buf'), self.dev_scalars, *rest)
        else:
            ops.rmsprop_step(pv, gv, r['sq'], r.get('buf'), group['lr'], *rest)


class FusedSGD(_FusedArenaOptimizer):
    """torch.optim.SGD semantics (dampening 0, no Nesterov; L2 weight decay) by ``ganlab_sgd_f32``, one launch per run.  With
    ``momentum`` > 0 the buffer of step 1 is the gradient itself (torch's first step); without it there is no state at all."""

    NAME = 'sgd'
    STATE = (('buf', 'momentum_buffer'),)

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0):
        _check_common(lr, None, weight_decay)
        if not 0.0 <= momentum:
            raise ValueError(f'Invalid momentum value: {momentum}')
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _active(self, group):
        return self.STATE if group['momentum'] > 0 else ()

    def _step_scalars(self, group, t):
        """(lr, first, 0): ``first`` is 1.0 on step 1 and 0.0 afterwards."""
        return float(group['lr']), 1.0 if t == 1 else 0.0, 0.0

    def _launch(self, group, r, pv, gv, scalars):
        if scalars is None:
            ops.sgd_step_dev(pv, gv, r.get('buf'), self.dev_scalars, group['weight_decay'], group['momentum'])
        else:
            ops.sgd_step(pv, gv, r.get('buf'), group['lr'], group['weight_decay'], group['momentum'], scalars[1] != 0.0)


# ``config.optimizer`` -> class.  'momentum' is SGD with ``config.momentum``; 'sgd' is SGD without.
OPTIMIZERS = {'adam': FusedAdam, 'rmsprop': FusedRMSprop, 'momentum': FusedSGD, 'sgd': FusedSGD, 'oadam': FusedOptimisticAdam}
CONFIG_FIELDS = ('momentum', 'rmsprop_momentum')


def optimizer_of_state(saved):
    """The ``config.optimizer`` value(s) whose ``export_moments`` wrote ``saved``, by its keys ('momentum' and 'sgd' share one)."""
    keys = set(saved) - {'step'}
    names = [n for n, cls in OPTIMIZERS.items() if {ck for _, ck in cls.STATE} == keys]
    return '/'.join(names) if names else 'unknown'


def saved_config_fields(cfg, optimizer=None):
    """``cfg`` (a dict of config fields) as a checkpoint stores it: with ``optimizer`` = 'adam' the ``momentum`` /
    ``rmsprop_momentum`` fields are not written, so files saved under Adam are what they were before the fields existed.
    ``optimizer``: the learner's current value (default: the config's own field)."""
    if str(cfg.get('optimizer', 'adam') if optimizer is None else optimizer).casefold() != 'adam':
        return cfg
    return {k: v for k, v in cfg.items() if k not in CONFIG_FIELDS}


def check_saved_optimizer(saved, current):
    """``saved``: the ``optimizer`` field of a checkpoint (None in files older than the field: Adam); ``current``: the learner's.
    A file saved under one optimiser does not load under another: their state buffers differ."""
    saved = 'adam' if saved is None else str(saved).casefold()
    current = str(current).casefold()
    if saved != current:
        raise ValueError(f"the checkpoint was saved with optimizer='{saved}' and this learner runs optimizer='{current}': "
                         f"their optimizer states are not interchangeable (build the learner with optimizer='{saved}')")


def check_save_format(optimizer, reference_format):
    """The reference can only read Adam state: a reference-format checkpoint under any other optimiser is refused."""
    if reference_format and str(optimizer).casefold() != 'adam':
        raise ValueError(f"reference_format=True needs optimizer='adam' (got optimizer='{optimizer}'): the reference's load_model "
                         f"restores torch.optim.Adam state only; save in this package's plain format")


class EwmaTracker(object):
    """EWMA shadow of the generator parameters (progan/learner.py:462-472, :909-916, :662-684):
    ``lagged = p*(1-beta) + lagged*beta`` over the whole arena in one launch.  ``lagged_params`` is
    the name -> tensor view dict the reference keeps (same key order as ``named_parameters()``)."""

    def __init__(self, arena):
        self.rebuild(arena, None)

    def rebuild(self, arena, old_lagged, rename=None):
        """New arena after a growth step: carry over the values of surviving parameters (after the
        reference's ``torgb -> prev_torgb`` re-keying), start new parameters from their current value."""
        self.arena = arena
        self.flat = arena.flat.detach().clone()
        self.lagged_params = arena.views_of(self.flat)
        if old_lagged is not None:
            rename = rename or {}
            with torch.no_grad():
                for k_old, v in old_lagged.items():
                    if rename and k_old in rename.values():
                        continue          # e.g. the previous prev_torgb.* is overwritten by the renamed torgb.*
                    k = rename.get(k_old, k_old)
                    if k in self.lagged_params and self.lagged_params[k].shape == v.shape:
                        self.lagged_params[k].copy_(v)

    def update(self, beta):
        if not self.arena.is_attached():
            self.arena.reabsorb()
        ops.ewma_step(self.flat, self.arena.flat, float(beta) if beta else 0.0)
