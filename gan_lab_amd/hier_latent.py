"""BigGAN's generator conditioning for the ResNet GAN: hierarchical latents ("skip-z") and a shared class embedding.

``config.hier_latent`` (bool) and ``config.shared_embed`` (int E, the embedding width; needs a ``cgan`` mode) - ResNet GAN
only, both off by default - replace the 2018 conditioning of the generator (one (num_classes, C) table per norm, the latent
entering through the first linear only) by BigGAN's (Brock et al. 2019, section 3 and appendix B):

    shared embedding     the class is embedded once, ``e(y) = shared.weight[y]`` (num_classes, E), for all norms
    hierarchical latent  ``z`` is split over the first linear and the B residual blocks: ``chunk = len_latent // (B + 1)``, the
                         first linear reads the first ``len_latent - B * chunk`` entries, block b the next ``chunk``
    modulation           both norms of block b are ``ModulatedBatchNorm2d``:
                         ``y = act((x - mean) * rstd * (1 + <gain.W[c], cond_b[n]>) + <shift.W[c], cond_b[n]>)`` with
                         ``cond_b[n] = [z_b[n], e(y_n)]`` (whichever parts are on); ``gain`` / ``shift`` are bias-free ``LinearEx``

With ``hier_latent`` alone (no labels) this is self-modulation (Chen et al. 2019).  The norm behind the last block is a plain
``BatchNorm2d`` (BigGAN's output layer), and with ``shared_embed`` the generator holds no (num_classes, C) table at all.  The
critic, the projection and the learner's label routing are untouched.

Where it runs: the layers compute nothing.  ``HierModulation`` below - owned by the generator, as ``SpectralNorm`` is by the
critic - holds one device-resident job table over the generator's parameters (``ops.HierTable``).  One launch writes every
gain and shift of the network into a flat (N, T) buffer, ``T = 2 * sum C``, reading ``z`` at the chunk's offset and the
embedding row directly (``cond`` is never formed); every norm reads its columns in place (``ops.mod_batch_norm_cols``) and writes
d gain / d shift into the same columns of one flat gradient buffer; at most three launches then produce every weight gradient
(written into the gradient arena), ``dz`` and the embedding's gradient, whatever the number of layers (csrc/hier.hip).  No
atomics, bitwise reproducible, nothing is read back by the host.  ``gain`` / ``shift`` are ``LinearEx``: ``ortho_reg``
regularises them like every other linear, and leaves ``shared.weight`` alone as it leaves the class tables (both as in BigGAN).
"""


def validate_config(config):
    """``config.hier_latent`` / ``config.shared_embed`` against their values and what they need; raises ValueError.
    -> (hier_latent, shared_embed)."""
    hier, embed = getattr(config, 'hier_latent', False), getattr(config, 'shared_embed', 0)
    if not isinstance(hier, bool):
        raise ValueError(f'config.hier_latent must be a bool (got {hier!r})')
    if not isinstance(embed, int) or isinstance(embed, bool) or embed < 0:
        raise ValueError(f'config.shared_embed must be an int >= 0, the width of the shared class embedding (got {embed!r})')
    if not hier and not embed:
        return False, 0
    if getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.hier_latent / config.shared_embed are ResNet GAN options (the progressive generators have '
                         'their own conditioning)')
    if embed and getattr(config, 'cgan', None) is None:      # any mode: the generator side is the same in all of them
        raise ValueError("config.shared_embed > 0 embeds the class: it needs config.cgan='projection' (or another cgan mode; and "
                         "num_classes >= 2)")
    if hier:
        blocks = num_blocks(getattr(config, 'res_samples', 64))
        if blocks is not None:
            chunk_layout(getattr(config, 'len_latent', 128), blocks)
    return hier, embed


def num_blocks(res):
    """Residual blocks of the ``res``-pixel ResNet generator (None: no such generator)."""
    return {32: 3, 64: 4}.get(res)


def chunk_layout(len_latent, blocks):
    """-> (width of the first linear's input, [(offset, width)] per block): ``chunk = len_latent // (blocks + 1)``, the first
    linear reads the first ``len_latent - blocks * chunk`` entries of z and block b the next ``chunk``."""
    if not isinstance(len_latent, int) or isinstance(len_latent, bool) or len_latent < blocks + 1:
        raise ValueError(f'hier_latent: len_latent must be an int >= {blocks + 1}, one entry for the first linear and for each '
                         f'of the {blocks} blocks (got {len_latent!r})')
    chunk = len_latent // (blocks + 1)
    first = len_latent - blocks * chunk
    return first, [(first + b * chunk, chunk) for b in range(blocks)]


def check_save_format(hier_latent, shared_embed, reference_format):
    """A reference-format checkpoint has no place for the modulation linears or the shared embedding."""
    if (hier_latent or shared_embed) and reference_format:
        raise ValueError('hier_latent / shared_embed cannot be saved with reference_format=True: the reference has neither the '
                         'modulation linears nor the shared embedding')


class HierModulation(object):
    """``HierModulation(generator)``: the manager of a generator built with ``hier_latent`` and / or ``shared_embed``.
    ``blocks``: [(the block's two ModulatedBatchNorm2d, (z offset, z width))].  The job table is built at the first call on the
    GPU and again whenever the parameters moved (a new arena, ``.to()``); ``attach()`` does it ahead of time (the learner calls
    it with every new arena, so that nothing is uploaded inside a step)."""

    def __init__(self, generator, norms, len_latent, shared=None):
        self.generator, self.len_latent, self.shared = generator, int(len_latent), shared
        self.norms = list(norms)                      # [(ModulatedBatchNorm2d, z_off, z_len)]
        self.table = None

    def attach(self):
        from . import ops
        jobs = []
        for m, z_off, z_len in self.norms:
            for lin, one in ((m.gain, 1.0), (m.shift, 0.0)):
                jobs.append(dict(w=lin.linear.weight, z_off=z_off, z_len=z_len, scale=lin.scale, one=one))
        self.table = ops.HierTable(jobs, self.len_latent, self.shared.weight if self.shared is not None else None)
        for i, (m, _, _) in enumerate(self.norms):
            m.cols = (self.table.cols[2 * i], self.table.cols[2 * i + 1])
        return self.table

    def __call__(self, z, labels):
        """Runs the modulation for this forward and hands every norm its columns: (mod, mod.detach(), gradient buffer)."""
        from . import ops
        if self.table is None or not self.table.is_current():
            self.attach()
        mod = ops.hier_modulate(self.table, z, labels)
        handle = (mod, mod.detach(), self.table.grad_buffer(z.shape[0]) if mod.requires_grad else None)
        for m, _, _ in self.norms:
            m.mod = handle
        return mod

    def clear(self):
        for m, _, _ in self.norms:
            m.mod = None
