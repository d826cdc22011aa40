"""The sampling side of the ResNet GAN, as BigGAN samples (Brock et al. 2019, sections 3.1 and 4, appendix C): an averaged
generator, the truncation trick and standing statistics.  ResNet GAN only; everything is off by default, and with the options off
the learner draws no extra random number, launches nothing extra and writes the checkpoints it always wrote.

``config.use_ewma_gen`` / ``ewma_decay`` / ``ewma_start`` - ``GeneratorEMA``: a deep copy of the generator in eval mode whose
parameters live in their own ``ParamArena`` (the layout of the live one).  After every generator update

    avg = d * avg + (1 - d) * live          d = 0 until update number ``ewma_start``, ``ewma_decay`` from then on

runs over the whole parameter arena (``ops.ewma_step``) and over every BatchNorm buffer (``ops.ewma_many``, a device-resident
table of segments: the buffers live outside the arena): two launches whatever the number of layers.  ``d = 0`` is a plain copy,
so until ``ewma_start`` the copy simply follows the live network (BigGAN's ``ema.update``).  ``num_batches_tracked`` is copied,
not averaged, and only when the state is read (``state_dict()``): no forward in eval mode reads it.

``config.truncation`` - ``learner.generate(truncation=t)`` draws its latents from the standard normal truncated to [-t, t].
BigGAN resamples the entries that fall outside; here the draw is the inverse CDF of the truncated normal on the project's
Philox stream (``rng.trunc_randn``; csrc/sample.hip): the same distribution without a data-dependent loop, and the stream
advances exactly as an untruncated draw of the same shape advances it.

``config.standing_stat_batches`` - ``standing_stats``: the running statistics of a BatchNorm are a 0.1-momentum average over
the LIVE weights' recent batches - wrong for averaged weights, and noisy.  Standing statistics re-estimate them for the network
as it is: reset the buffers, run ``num_batches`` forwards in train mode with momentum 1 / (k + 1) on pass k, so that they end as
the plain average of the batch statistics (``torch.nn.BatchNorm2d(momentum=None)``), and go back to eval mode.  This covers
``BatchNorm2d``, ``ConditionalBatchNorm2d`` and ``ModulatedBatchNorm2d`` on the kernels they already run on.
"""
import copy

import torch

FROM_CONFIG = object()      # generate(truncation=...): "whatever config.truncation says"
_DEFAULTS = (('use_ewma_gen', False), ('ewma_decay', 0.9999), ('ewma_start', 0), ('truncation', None),
             ('standing_stat_batches', 16))


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def validate_config(config):
    """The sampling options of ``config`` against their ranges; raises ValueError.  -> (use_ewma_gen, ewma_decay, ewma_start,
    truncation, standing_stat_batches).  ResNet GAN only: the progressive models have an averaged generator of their own
    (their ``use_ewma_gen``), which this does not touch."""
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        return None
    use, decay, start, trunc, batches = (getattr(config, k, d) for k, d in _DEFAULTS)
    if not isinstance(use, bool):
        raise ValueError(f'config.use_ewma_gen must be a bool (got {use!r})')
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= float(decay) < 1.0) or \
            torch.tensor(float(decay), dtype=torch.float32).item() >= 1.0:
        raise ValueError(f'config.ewma_decay must lie in [0, 1), and below 1 in float32 (got {decay!r})')
    if not _is_int(start) or start < 0:
        raise ValueError(f'config.ewma_start must be an int >= 0, the generator updates before averaging begins (got {start!r})')
    if trunc is not None:
        from . import ops
        trunc = ops.check_truncation(trunc, 'config.truncation')
    if not _is_int(batches) or batches < 1:
        raise ValueError(f'config.standing_stat_batches must be an int >= 1 (got {batches!r})')
    return use, float(decay), start, trunc, batches


def check_save_format(use_ewma_gen, reference_format):
    """A reference-format ResNet GAN checkpoint has no place for the averaged generator."""
    if use_ewma_gen and reference_format:
        raise ValueError('use_ewma_gen cannot be saved with reference_format=True: the reference\'s ResNet GAN has no averaged '
                         'generator')


def saved_config_fields(cfg):
    """``cfg`` (a dict of config fields) as a checkpoint stores it: a sampling option at its default is not written, so files
    saved with the options off are what they were before the options existed."""
    off = {k for k, d in _DEFAULTS if k in cfg and cfg[k] == d and type(cfg[k]) is type(d)}
    if 'use_ewma_gen' not in off:
        off -= {'ewma_decay', 'ewma_start'}
    return {k: v for k, v in cfg.items() if k not in off}


def _norms(net):
    from .utils.custom_layers import ConditionalBatchNorm2d, ModulatedBatchNorm2d
    return [m for m in net.modules()
            if isinstance(m, (torch.nn.modules.batchnorm._BatchNorm, ConditionalBatchNorm2d, ModulatedBatchNorm2d))]


class GeneratorEMA(object):
    """``GeneratorEMA(generator, arena, decay, start)``: the averaged copy ``model`` of ``generator`` (whose parameters live in
    ``arena``).  ``update()`` after every generator update; ``rebind`` when the generator moved to a new arena."""

    def __init__(self, generator, arena, decay=0.9999, start=0):
        self.decay, self.start, self.updates = float(decay), int(start), 0
        self.model = copy.deepcopy(generator)       # parameters: fresh tensors, no longer views into ``arena``
        self.model.eval().requires_grad_(False)
        from .optim import ParamArena
        self.arena = ParamArena(self.model.named_parameters(), arena.flat.device)
        self.table = None
        self.rebind(generator, arena)
        # a generator with hier_latent / shared_embed: the copy's manager came along with the deep copy and still holds the
        # live generator's job table - the copy gets one of its own over its own arena
        hier = getattr(self.model, 'hier', None)
        if hier is not None:
            own = set(self.model.modules())
            assert hier.generator is self.model and all(m in own for m, _, _ in hier.norms)
            hier.table = None
            if self.arena.flat.is_cuda:
                hier.attach()
                assert self._hier_in_own_arena()

    def _hier_in_own_arena(self):
        lo = self.arena.flat.data_ptr()
        hi = lo + 4 * self.arena.total
        return all(lo <= w.data_ptr() < hi for w in self.model.hier.table.weights)

    def rebind(self, generator, arena):
        """The live generator and the arena its parameters live in now (a rebuilt arena: checkpoint load)."""
        if arena.names != self.arena.names or arena.offsets != self.arena.offsets or arena.sizes != self.arena.sizes:
            raise ValueError('GeneratorEMA: the generator\'s arena does not have the layout of the averaged copy\'s')
        self.src, self.arena_src = generator, arena
        live = dict(generator.named_buffers())
        self._float_pairs, self._other_pairs = [], []
        for name, buf in self.model.named_buffers():
            pair = (buf, live[name])
            (self._float_pairs if buf.dtype == torch.float32 else self._other_pairs).append(pair)
        self.table = None

    def _buffer_table(self):
        from . import ops
        if self._float_pairs and (self.table is None or not self.table.is_current()):
            self.table = ops.EwmaTable(self._float_pairs)
        return self.table

    def decay_of_update(self, number):
        """The decay of update ``number`` (1-based): 0 - a copy - before update ``start``, ``decay`` from it on."""
        return 0.0 if number < self.start else self.decay

    def update(self):
        """One step of the average, after a generator update: 2 launches."""
        from . import ops
        if not self.arena_src.is_attached():
            self.arena_src.reabsorb()
        d = self.decay_of_update(self.updates + 1)
        ops.ewma_step(self.arena.flat, self.arena_src.flat, d)
        table = self._buffer_table()
        if table is not None:
            ops.ewma_many(table, d)
        self._weights_moved()
        self.updates += 1

    def _weights_moved(self):
        """The copy's parameters were rewritten through raw pointers: its packed conv weights are stale (ops.bump_weight_epoch)."""
        from . import ops
        lo = self.arena.flat.data_ptr()
        ops.bump_weight_epoch([(lo, lo + 4 * self.arena.total)])

    def sync_counters(self):
        """``num_batches_tracked`` (every buffer that is not float32) of the copy <- the live generator's."""
        with torch.no_grad():
            for dst, src in self._other_pairs:
                dst.copy_(src)

    def reset(self):
        """The copy <- the live generator as it is now, the update count <- 0."""
        if not self.arena_src.is_attached():
            self.arena_src.reabsorb()
        with torch.no_grad():
            self.arena.flat.copy_(self.arena_src.flat)
            for dst, src in self._float_pairs + self._other_pairs:
                dst.copy_(src)
        self._weights_moved()
        self.updates = 0

    def state_dict(self):
        self.sync_counters()
        return {'model': {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}, 'updates': self.updates}

    def load_state_dict(self, state):
        self.model.load_state_dict(state['model'])      # in place: the parameters stay views into the copy's arena
        if not self.arena.is_attached():
            self.arena.reabsorb()
        self._weights_moved()
        self.updates = int(state['updates'])


def _num_classes(gen):
    if getattr(gen, 'shared_embed', 0):
        return gen.shared.num_embeddings
    return gen._cond_norms[0].num_classes


def standing_stats(gen, num_batches, batch_size, len_latent, labels_fn=None, truncation=None):
    """BigGAN's standing statistics for ``gen`` as it is: every norm's ``running_mean`` / ``running_var`` <- the plain average of
    the batch mean / unbiased batch variance over ``num_batches`` forwards in train mode on fresh latents (``truncation``: from
    the truncated normal), ``num_batches_tracked`` <- ``num_batches``.  ``labels_fn(batch_size)`` -> the labels of a batch;
    None: uniform from the Philox stream for a class-conditional generator.  The momenta and the train / eval state of every
    module are restored."""
    from . import ops, rng
    if not _is_int(num_batches) or num_batches < 1:
        raise ValueError(f'standing_stats: num_batches must be an int >= 1 (got {num_batches!r})')
    if truncation is not None:
        truncation = ops.check_truncation(truncation, 'truncation')
    norms = _norms(gen)
    dev = next(gen.parameters()).device
    cond = bool(getattr(gen, 'cgan', False))
    if cond and labels_fn is None:
        classes = _num_classes(gen)
        labels_fn = lambda b: rng.randint(b, classes, dev)  # noqa: E731
    modes = [(m, m.training) for m in gen.modules()]
    momenta = [m.momentum for m in norms]
    with torch.no_grad():
        for m in norms:
            m.running_mean.zero_()
            m.running_var.fill_(1.0)
            m.num_batches_tracked.zero_()
        gen.train()
        try:
            for k in range(num_batches):
                for m in norms:
                    m.momentum = 1.0 / (k + 1)      # a host float (never None: ops.batch_norm takes float(momentum))
                z = rng.randn((batch_size, len_latent), dev) if truncation is None else \
                    rng.trunc_randn((batch_size, len_latent), truncation, dev)
                gen(z, labels_fn(batch_size)) if cond else gen(z)
        finally:
            for m, mom in zip(norms, momenta):
                m.momentum = mom
            for m, flag in modes:
                m.training = flag
