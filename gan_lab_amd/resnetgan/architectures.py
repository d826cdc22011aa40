"""ResNet GAN generators / discriminators on the HIP path (drop-in for
gan_lab/resnetgan/architectures.py:29-224): same class names, constructor arguments, module tree and
``state_dict`` keys; every tensor op runs in the hand-written kernels (gan_lab_amd.ops).  ``self_attention=True`` (not in
the reference; default off) adds a SAGAN block ``self_attn`` (attention.py) beside the unchanged module tree; ``cgan=True``
(not in the reference either; default off) with ``num_classes`` = K makes the networks class-conditional (conditional.py): every
generator BatchNorm carries (K, C) tables and the generator is called as ``g(z, labels)``, the critic gains the projection layer
``proj`` and is called as ``d(x, labels)``; a critic built with ``cgan='acgan'`` / ``'contra'`` / ``'reacgan'`` gains a classifier
head instead (``cls``, or ``embed`` and ``proxy`` with ``cond_embed`` = E), keeps the unconditional score and hands the feature to
the caller's loss with ``d(x, labels, return_features=True)``.  With ``cgan`` the reference's meaning of ``num_classes`` (a
one-hot concatenated to the input) does not apply: the inputs keep their widths.  ``hier_latent=True`` / ``shared_embed=E`` (not in the reference; default
off; generators only) are BigGAN's conditioning (hier_latent.py): both norms of every block become ``ModulatedBatchNorm2d`` whose
``gain`` / ``shift`` linears read the block's chunk of ``z`` and / or the row ``shared.weight[label]`` of one (K, E) embedding, the
first linear reads only the first chunk, the norm behind the last block is a plain ``BatchNorm2d`` and - with ``shared_embed`` -
no (K, C) table is left; all gains and shifts of a forward come from one launch of the generator's ``hier`` manager."""
from torch import nn

from .. import ops
from .._int import FMAP_SAMPLES, RES_INIT
from ..utils.custom_layers import Conv2dEx, Lambda, LinearEx, NormalizeLayer, Tanh, fused_sequential
from .base import GAN
from .resblocks import FastResBlock2dDownsample, ResBlock2d, ResBlock2d32Pix, _own_nl, _own_resampler

FMAP_G = 64
FMAP_D = 64
FMAP_G_INIT_32_FCTR = 1
FMAP_G_INIT_64_FCTR = 4
RES_FEATURE_SPACE = 4


def _run(seq, x, start=0, stop=None):
    """Children [start, stop) of a Sequential through the peephole executor, ResBlocks through their own forward."""
    run = []
    for m in list(seq)[start:stop]:
        if isinstance(m, (ResBlock2d, FastResBlock2dDownsample)):
            if run:
                x = fused_sequential(run, x)
                run = []
            x = m(x)
        else:
            run.append(m)
    return fused_sequential(run, x) if run else x


def _init_self_attention(net, self_attention, ni, equalized_lr):
    """``self_attention=True``: the SAGAN block as the attribute ``self_attn`` - NOT a child of the Sequential, so the
    module tree and ``state_dict`` keys without it are unchanged and only ``self_attn.*`` keys are added with it."""
    if self_attention:
        from ..attention import SelfAttention2d
        net.self_attn = SelfAttention2d(ni, equalized_lr=equalized_lr)
    else:
        net.self_attn = None


def _run_with_attention(net, seq, x, split):
    """``_run`` over ``seq`` with the network's attention block between children ``split - 1`` and ``split``."""
    if net.self_attn is None:
        return _run(seq, x)
    return _run(seq, net.self_attn(_run(seq, x, 0, split)), split)


def _need_labels(net, labels):
    if labels is None:
        raise TypeError(f'{type(net).__name__} was built with cgan=True: call it as net(input, labels) with one class label '
                        f'per sample')
    return labels


class _ResnetGenerator(GAN):
    ATTN_AFTER = None       # index of the first child of generator_model behind the attention block
    cgan = False
    hier = None             # hier_latent.HierModulation with hier_latent / shared_embed

    def _init_cgan(self, cgan, num_classes):
        """``cgan=True``: the conditional norms were built by the blocks / NormalizeLayer; remember them for label routing."""
        from ..utils.custom_layers import ConditionalBatchNorm2d
        self.cgan = bool(cgan)
        self._cond_norms = [m for m in self.modules() if isinstance(m, ConditionalBatchNorm2d)] if self.cgan else []
        assert not self.cgan or self.hier is not None or \
            len(self._cond_norms) == sum(isinstance(m, NormalizeLayer) for m in self.modules())

    def _init_hier(self, hier_latent, shared_embed, cgan, cond_classes, len_latent, num_classes, kw, blocks):
        """``hier_latent`` / ``shared_embed``, before the Sequential is built.  -> (its first child, the input width of the first
        linear, the keyword arguments of each of the ``blocks`` blocks, the classes of the last norm).  Both off: what the
        generator has always had.  Else the first linear reads the first chunk of z only, the blocks' norms are modulated and
        the last one is plain; ``_init_hier_manager`` finishes the job behind the Sequential."""
        from .. import hier_latent as hl
        if not isinstance(shared_embed, int) or isinstance(shared_embed, bool) or shared_embed < 0:
            raise ValueError(f'shared_embed must be an int >= 0 (got {shared_embed!r})')
        if shared_embed and not cgan:
            raise ValueError('shared_embed > 0 needs cgan=True (and num_classes >= 2): it embeds the class')
        self.hier_latent, self.shared_embed, self.hier = bool(hier_latent), shared_embed, None
        if not self.hier_latent and not shared_embed:
            return Lambda(lambda x: x.view(-1, len_latent + num_classes)), len_latent + num_classes, [kw] * blocks, cond_classes
        first, self._chunks = hl.chunk_layout(len_latent, blocks) if self.hier_latent else (len_latent, [(0, 0)] * blocks)
        if shared_embed:
            self.shared = nn.Embedding(cond_classes, shared_embed)      # parameter container only (key `shared.weight`)
        view = Lambda(lambda x: x.view(-1, len_latent)[:, :first]) if self.hier_latent else \
            Lambda(lambda x: x.view(-1, len_latent))
        return view, first, [dict(kw, num_classes=0, cond_dim=w + shared_embed) for _, w in self._chunks], 0

    def _init_hier_manager(self):
        if self.hier_latent or self.shared_embed:
            from .. import hier_latent as hl
            from ..utils.custom_layers import ModulatedBatchNorm2d
            blocks = [m for m in self.generator_model if isinstance(m, ResBlock2d)]
            norms = [(m, z_off, z_len) for blk, (z_off, z_len) in zip(blocks, self._chunks) for m in blk.modules()
                     if isinstance(m, ModulatedBatchNorm2d)]
            assert len(norms) == 2 * len(self._chunks)
            self.hier = hl.HierModulation(self, norms, self.len_latent, self.shared if self.shared_embed else None)

    def _forward_modulated(self, x, labels):
        if self.shared_embed:
            _need_labels(self, labels)
        elif labels is not None and not self.cgan:
            raise TypeError(f'{type(self).__name__} is not class-conditional (cgan=False) and takes no labels')
        z = x.view(-1, self.len_latent)
        self.hier(z, labels if self.shared_embed else None)
        try:
            return _run_with_attention(self, self.generator_model, z, self.ATTN_AFTER)
        finally:
            self.hier.clear()

    def forward(self, x, labels=None):
        if self.hier is not None:
            return self._forward_modulated(x, labels)
        if not self.cgan:
            if labels is not None:
                raise TypeError(f'{type(self).__name__} is not class-conditional (cgan=False) and takes no labels')
            return _run_with_attention(self, self.generator_model, x, self.ATTN_AFTER)
        # the batch's labels reach the conditional norms as an attribute for the length of this forward: the Sequential, the
        # peephole executor and the blocks stay label-free (the backward has its own copy, saved by the op)
        _need_labels(self, labels)
        for m in self._cond_norms:
            m.labels = labels
        try:
            return _run_with_attention(self, self.generator_model, x, self.ATTN_AFTER)
        finally:
            for m in self._cond_norms:
                m.labels = None


class Generator32PixResnet(_ResnetGenerator):
    """32-pixel ResNet generator with optional class conditioning (architectures.py:29-59).  ``self_attention``: a SAGAN
    block on the 16x16 map, after the second block."""
    ATTN_AFTER = 5

    def __init__(self, len_latent=128, fmap=FMAP_G * 2, upsampler=None, blur_type=None, nl=None, num_classes=0,
                 equalized_lr=False, self_attention=False, cgan=False, hier_latent=False, shared_embed=0):
        super().__init__(32)
        cond_classes, num_classes = _cgan_classes(cgan, num_classes)
        from ..utils.custom_layers import Upsample2x
        upsampler = _own_resampler(upsampler) if upsampler is not None else Upsample2x()
        nl = _own_nl(nl)
        self.len_latent, self.num_classes, self.equalized_lr = len_latent, num_classes, equalized_lr
        f0 = len_latent * FMAP_G_INIT_32_FCTR
        kw = dict(ks=3, norm_type='BatchNorm', upsampler=upsampler, init='He', nl=nl, equalized_lr=equalized_lr,
                  blur_type=blur_type, **({'num_classes': cond_classes} if cgan else {}))
        view, nin, kws, last_classes = self._init_hier(hier_latent, shared_embed, cgan, cond_classes, len_latent, num_classes,
                                                       kw, 3)
        self.generator_model = nn.Sequential(
            view,
            LinearEx(nin_feat=nin, nout_feat=f0 * RES_INIT ** 2, init='Xavier', equalized_lr=equalized_lr),
            Lambda(lambda x: x.view(-1, f0, RES_INIT, RES_INIT)),
            ResBlock2d32Pix(ni=f0, nf=fmap, **kws[0]),
            ResBlock2d32Pix(ni=fmap, nf=fmap, **kws[1]),
            ResBlock2d32Pix(ni=fmap, nf=fmap, **kws[2]),
            NormalizeLayer('BatchNorm', ni=fmap, num_classes=last_classes),
            nl,
            Conv2dEx(ni=fmap, nf=FMAP_SAMPLES, ks=3, stride=1, padding=1, init='Xavier', equalized_lr=equalized_lr),
            Tanh(),
        )
        _init_self_attention(self, self_attention, fmap, equalized_lr)
        self._init_hier_manager()
        self._init_cgan(cgan, cond_classes)


class Generator64PixResnet(_ResnetGenerator):
    """64-pixel ResNet generator with optional class conditioning (architectures.py:62-97).  ``self_attention``: a SAGAN
    block on the 32x32 map (2 * fmap channels), after the third block."""
    ATTN_AFTER = 6

    def __init__(self, len_latent=128, fmap=FMAP_G, upsampler=None, blur_type=None, nl=None, num_classes=0,
                 equalized_lr=False, self_attention=False, cgan=False, hier_latent=False, shared_embed=0):
        super().__init__(64)
        cond_classes, num_classes = _cgan_classes(cgan, num_classes)
        from ..utils.custom_layers import Upsample2x
        upsampler = _own_resampler(upsampler) if upsampler is not None else Upsample2x()
        nl = _own_nl(nl)
        self.len_latent, self.num_classes, self.equalized_lr = len_latent, num_classes, equalized_lr
        f0 = len_latent * FMAP_G_INIT_64_FCTR
        kw = dict(ks=3, norm_type='BatchNorm', upsampler=upsampler, init='He', nl=nl, equalized_lr=equalized_lr,
                  blur_type=blur_type, **({'num_classes': cond_classes} if cgan else {}))
        view, nin, kws, last_classes = self._init_hier(hier_latent, shared_embed, cgan, cond_classes, len_latent, num_classes,
                                                       kw, 4)
        self.generator_model = nn.Sequential(
            view,
            LinearEx(nin_feat=nin, nout_feat=f0 * RES_INIT ** 2, init='Xavier', equalized_lr=equalized_lr),
            Lambda(lambda x: x.view(-1, f0, RES_INIT, RES_INIT)),
            ResBlock2d(ni=f0, nf=8 * fmap, **kws[0]),
            ResBlock2d(ni=8 * fmap, nf=4 * fmap, **kws[1]),
            ResBlock2d(ni=4 * fmap, nf=2 * fmap, **kws[2]),
            ResBlock2d(ni=2 * fmap, nf=1 * fmap, **kws[3]),
            NormalizeLayer('BatchNorm', ni=1 * fmap, num_classes=last_classes),
            nl,
            Conv2dEx(ni=1 * fmap, nf=FMAP_SAMPLES, ks=3, stride=1, padding=1, init='He', equalized_lr=equalized_lr),
            Tanh(),
        )
        _init_self_attention(self, self_attention, 2 * fmap, equalized_lr)
        self._init_hier_manager()
        self._init_cgan(cgan, cond_classes)


def _cgan_classes(cgan, num_classes):
    """-> (classes of the conditional layers, one-hot width concatenated to the input).  ``cgan=True``: ``num_classes`` counts
    the classes of the tables / the projection and nothing is concatenated."""
    if not cgan:
        return 0, num_classes
    if not isinstance(num_classes, int) or num_classes < 2:
        raise ValueError(f'cgan=True needs num_classes >= 2 (got {num_classes!r})')
    return num_classes, 0


def _critic_mode(cgan):
    """The critic's ``cgan`` argument -> None, 'projection' (also True) or one of the classifier modes."""
    from ..conditional import HEAD_MODES
    if not cgan:
        return None
    if cgan is True or cgan == 'projection':
        return 'projection'
    if cgan in HEAD_MODES:
        return cgan
    raise ValueError(f"cgan must be False, True / 'projection', 'acgan', 'contra' or 'reacgan' (got {cgan!r})")


def _init_projection(critic, cgan, num_classes, nin_feat, equalized_lr, cond_embed=512):
    """The critic's conditioning heads, beside ``linear1`` and reading the same feature; built before ``_init_spectral_norm`` so
    that they get their u, v like every other layer.  ``cgan=True`` / ``'projection'``: the class embedding ``proj`` of the
    projection critic, a bias-free LinearEx.  ``'acgan'``: the classifier ``cls``.  ``'contra'`` / ``'reacgan'``: ``embed`` and the
    bias-free ``proxy``, whose (K, E) weight rows are the class proxies - read as a table, never applied as a layer."""
    critic.cond_mode = mode = _critic_mode(cgan)
    critic.proj = LinearEx(nin_feat=nin_feat, nout_feat=num_classes, include_bias=False, init='Xavier',
                           equalized_lr=equalized_lr) if mode == 'projection' else None
    if mode == 'acgan':
        critic.cls = LinearEx(nin_feat=nin_feat, nout_feat=num_classes, init='Xavier', equalized_lr=equalized_lr)
    elif mode in ('contra', 'reacgan'):
        from ..conditional import MAX_EMBED
        if not isinstance(cond_embed, int) or isinstance(cond_embed, bool) or not 1 <= cond_embed <= MAX_EMBED:
            raise ValueError(f'cond_embed must be an integer in [1, {MAX_EMBED}] (got {cond_embed!r})')
        critic.embed = LinearEx(nin_feat=nin_feat, nout_feat=cond_embed, init='Xavier', equalized_lr=equalized_lr)
        critic.proxy = LinearEx(nin_feat=cond_embed, nout_feat=num_classes, include_bias=False, init='Xavier',
                                equalized_lr=equalized_lr)


def _critic_forward(critic, x, labels, return_features=False):
    _check_spectral_norm(critic)
    if critic.cond_mode is None and labels is not None:
        raise TypeError(f'{type(critic).__name__} is not class-conditional (cgan=False) and takes no labels')
    if critic.cond_mode is not None:
        _need_labels(critic, labels)
    f = critic.features(x)
    out = critic.linear1(f).view(-1)
    if critic.proj is not None:
        proj = critic.proj
        weight = proj.linear.weight if proj.weight_override is None else proj.weight_override
        if proj.scale != 1.0:
            weight = ops.scale(weight, proj.scale)
        out = ops.class_projection(f, weight, labels, out)
    return (out, f) if return_features else out


def _init_spectral_norm(critic, spectral_norm):
    """``spectral_norm=True``: every Conv2dEx / LinearEx of the critic gets its ``weight_u`` / ``weight_v`` buffers; the
    normalised weights themselves come from a ``spectral_norm.SpectralNorm`` manager built over the critic's arena."""
    critic.spectral_norm = bool(spectral_norm)
    if critic.spectral_norm:
        from ..spectral_norm import register_uv
        register_uv(critic)


def _check_spectral_norm(critic):
    if critic.spectral_norm and critic.sn is None:
        raise RuntimeError('this critic was built with spectral_norm=True: attach a spectral_norm.SpectralNorm manager '
                           '(it owns the normalised weights) before calling it')


class Discriminator32PixResnet(GAN):
    """32-pixel ResNet discriminator / critic (architectures.py:103-133).  ``self_attention``: a SAGAN block on the 16x16
    map, after ``conv1``."""

    def __init__(self, fmap=FMAP_D * 2, pooler=None, blur_type=None, nl=None, num_classes=0, equalized_lr=False,
                 spectral_norm=False, self_attention=False, cgan=False, cond_embed=512):
        super().__init__(32)
        cond_classes, num_classes = _cgan_classes(cgan, num_classes)
        from ..utils.custom_layers import AvgPool2x
        pooler = _own_resampler(pooler) if pooler is not None else AvgPool2x()
        nl = _own_nl(nl)
        self.num_classes, self.equalized_lr = num_classes, equalized_lr
        self.view1 = Lambda(lambda x: x.view(-1, FMAP_SAMPLES + num_classes, self.res, self.res))
        self.conv1 = FastResBlock2dDownsample(ni=FMAP_SAMPLES + num_classes, nf=fmap, ks=3, pooler=pooler,
                                              init='Xavier', nl=nl, equalized_lr=equalized_lr, blur_type=blur_type)
        kw = dict(ks=3, norm_type='LayerNorm', init='He', nl=nl, equalized_lr=equalized_lr, blur_type=blur_type)
        self.resblocks = nn.Sequential(
            ResBlock2d32Pix(ni=fmap, nf=fmap, pooler=pooler, res=self.res // 2, **kw),
            ResBlock2d32Pix(ni=fmap, nf=fmap, res=self.res // 4, **kw),
            ResBlock2d32Pix(ni=fmap, nf=fmap, res=self.res // 4, **kw),
            nl,
            Lambda(ops.global_avg_pool),      # nn.AvgPool2d(kernel_size=res//4) on the (res//4)^2 map
            Lambda(lambda x: x.view(-1, fmap)),
        )
        self.linear1 = LinearEx(nin_feat=fmap, nout_feat=1, init='Xavier', equalized_lr=equalized_lr)
        _init_self_attention(self, self_attention, fmap, equalized_lr)
        _init_projection(self, cgan, cond_classes, fmap, equalized_lr, cond_embed)
        _init_spectral_norm(self, spectral_norm)      # after the block exists: its convolutions get u, v too

    def features(self, x):
        return _run_with_attention(self, self.resblocks, self.conv1(self.view1(x)), 0)

    def forward(self, x, labels=None, return_features=False):
        return _critic_forward(self, x, labels, return_features)


class Discriminator64PixResnet(GAN):
    """64-pixel ResNet discriminator / critic (architectures.py:157-187).  ``self_attention``: a SAGAN block on the 32x32
    map (2 * fmap channels), after the first block."""

    def __init__(self, fmap=FMAP_D, pooler=None, blur_type=None, nl=None, num_classes=0, equalized_lr=False,
                 spectral_norm=False, self_attention=False, cgan=False, cond_embed=512):
        super().__init__(64)
        cond_classes, num_classes = _cgan_classes(cgan, num_classes)
        from ..utils.custom_layers import AvgPool2x
        pooler = _own_resampler(pooler) if pooler is not None else AvgPool2x()
        nl = _own_nl(nl)
        self.num_classes, self.equalized_lr = num_classes, equalized_lr
        self.view1 = Lambda(lambda x: x.view(-1, FMAP_SAMPLES + num_classes, self.res, self.res))
        self.conv1 = Conv2dEx(ni=FMAP_SAMPLES + num_classes, nf=1 * fmap, ks=3, stride=1, padding=1, init='Xavier',
                              equalized_lr=equalized_lr)
        kw = dict(ks=3, norm_type='LayerNorm', pooler=pooler, init='He', nl=nl, equalized_lr=equalized_lr,
                  blur_type=blur_type)
        self.resblocks = nn.Sequential(
            ResBlock2d(ni=1 * fmap, nf=2 * fmap, res=self.res // 1, **kw),
            ResBlock2d(ni=2 * fmap, nf=4 * fmap, res=self.res // 2, **kw),
            ResBlock2d(ni=4 * fmap, nf=8 * fmap, res=self.res // 4, **kw),
            ResBlock2d(ni=8 * fmap, nf=8 * fmap, res=self.res // 8, **kw),
            Lambda(lambda x: x.view(-1, RES_FEATURE_SPACE ** 2 * 8 * fmap)),
        )
        self.linear1 = LinearEx(nin_feat=RES_FEATURE_SPACE ** 2 * 8 * fmap, nout_feat=1, init='Xavier',
                                equalized_lr=equalized_lr)
        _init_self_attention(self, self_attention, 2 * fmap, equalized_lr)
        _init_projection(self, cgan, cond_classes, RES_FEATURE_SPACE ** 2 * 8 * fmap, equalized_lr, cond_embed)
        _init_spectral_norm(self, spectral_norm)      # after the block exists: its convolutions get u, v too

    def features(self, x):
        return _run_with_attention(self, self.resblocks, self.conv1(self.view1(x)), 1)

    def forward(self, x, labels=None, return_features=False):
        return _critic_forward(self, x, labels, return_features)


class DiscriminatorAC32PixResnet(Discriminator32PixResnet):
    """Auxiliary-classifier variant, discriminator class-conditioning removed (architectures.py:136-154)."""

    def __init__(self, fmap=FMAP_D * 2, pooler=None, blur_type=None, nl=None, num_classes=0, equalized_lr=False):
        super().__init__(fmap, pooler, blur_type, nl, num_classes, equalized_lr)
        self.view1 = Lambda(lambda x: x.view(-1, FMAP_SAMPLES, self.res, self.res))
        self.conv1 = FastResBlock2dDownsample(ni=FMAP_SAMPLES, nf=fmap, ks=3, pooler=pooler, init='Xavier',
                                              nl=nl, equalized_lr=equalized_lr, blur_type=blur_type)
        self.linear_aux = LinearEx(nin_feat=fmap, nout_feat=num_classes, init='Xavier', equalized_lr=equalized_lr)

    def forward(self, x):
        f = self.features(x)
        return self.linear1(f).view(-1), self.linear_aux(f)


class DiscriminatorAC64PixResnet(Discriminator64PixResnet):
    """Auxiliary-classifier variant (architectures.py:190-207)."""

    def __init__(self, fmap=FMAP_D, pooler=None, blur_type=None, nl=None, num_classes=0, equalized_lr=False):
        super().__init__(fmap, pooler, blur_type, nl, num_classes, equalized_lr)
        self.view1 = Lambda(lambda x: x.view(-1, FMAP_SAMPLES, self.res, self.res))
        self.conv1 = Conv2dEx(ni=FMAP_SAMPLES, nf=1 * fmap, ks=3, stride=1, padding=1, init='Xavier',
                              equalized_lr=equalized_lr)
        self.linear_aux = LinearEx(nin_feat=RES_FEATURE_SPACE ** 2 * 8 * fmap, nout_feat=num_classes, init='Xavier',
                                   equalized_lr=equalized_lr)

    def forward(self, x):
        f = self.features(x)
        return self.linear1(f).view(-1), self.linear_aux(f)
