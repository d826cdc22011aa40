"""GANLearner on the HIP path (drop-in surface of gan_lab/resnetgan/learner.py).

Two roles, as in the reference:
  * base class of ProGANLearner / StyleGANLearner (:87-301, :780-946): supervision flags, resampler /
    nonlinearity selection, loss + gradient-penalty + optimiser + LR-scheduler plumbing;
  * the learner of the non-progressive ResNet GANs (BASELINE config #5, ``config.model ==
    'ResNet GAN'``): 32 / 64 pixel BatchNorm generator + LayerNorm critic, ``train()`` = per main
    iteration ``num_gen_iters`` generator iterations with the critic frozen, then ``num_disc_iters``
    critic iterations (:463-700), WGAN + WGAN-GP by default.
Every tensor op of the step runs in the hand-written kernels (gan_lab_amd.ops); parameters, gradients
and Adam moments live in flat arenas (optim.py); with torch.distributed initialised the gradients are
mean-all-reduced over RCCL (BatchNorm statistics stay per rank, like DDP without SyncBN).
``config.spectral_norm`` (ResNet GAN only) normalises every critic weight by its largest singular value
(spectral_norm.py) and ``loss='hinge'`` is its usual partner; ``config.self_attention`` ('g', 'd', 'gd'; ResNet GAN only) adds
SAGAN's self-attention block to the generator / critic (attention.py); ``config.cgan='projection'`` (ResNet GAN only, with
``config.num_classes`` >= 2) makes the pair class-conditional - conditional BatchNorm in the generator, a projection critic
(conditional.py) - and ``g_step`` / ``d_step`` then take the batch's labels; ``config.cgan='contra'`` / ``'reacgan'``
keep the critic's score unconditional and add ``config.cond_lambda`` times the loss of a classifier head on the critic's feature -
ContraGAN's 2C, ReACGAN's D2D-CE (csrc/cond_loss.hip) - to the critic step on the real rows and to the
generator step on the generated rows, per rank, with the unweighted terms in ``last_losses['cond_d']`` / ``['cond_g']``;
``config.ortho_reg`` / ``config.ortho_reg_d``
(ResNet GAN only) add the gradient of BigGAN's orthogonal regulariser to the generator's / critic's weight gradients before
the optimiser step (ortho_reg.py); ``config.hier_latent`` / ``config.shared_embed`` (ResNet GAN only) give the generator BigGAN's
conditioning - hierarchical latents and a shared class embedding modulating every block norm (hier_latent.py) - without touching
the critic or the label routing; ``config.use_ewma_gen`` / ``config.truncation`` / ``config.standing_stat_batches`` (ResNet GAN
only) are the sampling side - an averaged copy of the generator updated after every generator step, and ``generate()`` with the
truncation trick and standing statistics (sampling.py); ``config.cr_real`` / ``cr_fake`` / ``cr_latent_d`` / ``cr_latent_g``
(ResNet GAN only) add consistency regularisation - bCR on a flipped and shifted copy of the critic's inputs, zCR on a perturbed
latent - to the critic's and the generator's loss (consistency.py); all of them are off by default.
Validation metrics, image grids and plotting (:249-461, :950-1046) are outside the hot path."""
import os
import warnings

import torch

from .. import _lib, ops, parallel
from .._int import FMAP_SAMPLES, LearnerConfigCopy, get_current_configuration  # noqa: F401
from ..optim import ParamArena
from ..sampling import FROM_CONFIG
from ..utils import backprop_utils as bp
from ..utils.backprop_utils import configure_optimizer_for_gan
from ..utils.custom_layers import LeakyReLU, Tanh, make_downsampler, make_upsampler
from ..utils.latent_utils import gen_rand_latent_vars

NONREDEFINABLE_ATTRS = ('model', 'res_samples', 'res_dataset', 'len_latent', 'num_classes', 'class_condition',
                        'use_auxiliary_classifier', 'model_upsample_type', 'model_downsample_type',
                        'align_corners', 'blur_type', 'nonlinearity', 'use_equalized_lr',)
REDEFINABLE_FROM_LEARNER_ATTRS = ('batch_size', 'loss', 'gradient_penalty', 'optimizer', 'lr_sched',)


class GANLearner(object):
    def __init__(self, config):
        super().__init__()
        self._model = config.model
        self.pretrained_model = False
        dev = torch.device(config.dev)
        # GANLAB_HOST_LOGIC_ONLY=1 lets the CPU tests drive the learner's HOST logic (construction, growth events,
        # arenas, optimiser / EWMA bookkeeping, the data-parallel parameter broadcast over gloo).  It does not add a
        # CPU compute path: every tensor op of a step still raises in gan_lab_amd.ops for a non-GPU tensor.
        if dev.type != 'cuda' and os.environ.get('GANLAB_HOST_LOGIC_ONLY') != '1':
            raise RuntimeError(f"gan_lab_amd runs on the MI355X only (config.dev={config.dev!r}); there is no CPU "
                               f"path - use the reference or the test oracle for CPU runs")
        _lib.lib()  # fail now, loudly, if the kernel library is missing
        from .. import ops
        ops.set_compute_dtype(getattr(config, 'compute_dtype', 'f32'))   # 'bf16': BASELINE config #2
        # DiffAugment of every critic input (config.diffaugment; None = off: no draw, no launch, no stream advance)
        from .. import augment
        self.diffaug = augment.from_config(getattr(config, 'diffaugment', None))
        # ADA (config.ada; None = off likewise): the other augmentation of the critic inputs, at the same hook points, with
        # its probability and controller statistics in a device block (ada.py); the two exclude each other
        from .. import ada
        self.ada = ada.from_config(config)
        self.critic_aug = self.diffaug if self.diffaug is not None else self.ada
        # the set metrics' options ('swd' ... 'kid' in config.gen_metrics; validation.py): checked here, used by compute_metrics,
        # which keeps the evaluation objects across validation points: name -> (constructor arguments, objects)
        from .. import validation
        for s in validation.SCORERS:
            if not s.progressive_only:
                s.module.validate_config(config)
        self._metric_evals = {}
        # self-attention (config.self_attention; attention.py): a ResNet GAN option, and first order only - a critic with a
        # block excludes the gradient penalties
        from .. import attention
        self._attn_g, self._attn_d = attention.validate_config(config)

        self.curr_dataset_batch_num = 0
        self.curr_epoch_num = 1
        # supervised / unsupervised selection (resnetgan/learner.py:122-138)
        self.num_classes = 0
        self.cond_gen = self.cond_disc = self.ac = False
        self.num_classes_gen = self.num_classes_disc = 0
        if config.use_auxiliary_classifier or config.class_condition:
            # SURVEY.md §8f item 4.  No variant of these options runs in the reference (every combination raises in its
            # constructor or first iteration: tests/golden/probe_conditional.py -> tests/golden/conditional_probe.json),
            # so there is no behaviour to be in parity with.
            raise NotImplementedError('class_condition / use_auxiliary_classifier: no variant of these options runs in '
                                      'the reference (tests/golden/conditional_probe.json); not provided')
        # class conditioning of our own (config.cgan; conditional.py): conditional BatchNorm + a projection critic or a critic with
        # a classifier head and its loss (self._cond: the loss's weight and parameters, None in the other modes), ResNet GAN only
        from .. import conditional
        self.cgan = conditional.validate_config(config)
        self._cgan_mode = conditional.mode(config) if self.cgan else None
        self._cond = conditional.validate_loss_config(config)
        # BigGAN's generator conditioning (config.hier_latent / config.shared_embed; hier_latent.py): ResNet GAN only
        from .. import hier_latent
        self._hier_latent, self._shared_embed = hier_latent.validate_config(config)
        if not (config.res_samples <= config.res_dataset):
            raise ValueError(f'Resolution of generated images (config.res_samples = {config.res_samples}) must be '
                             f'less than\nor equal to resolution of dataset (config.res_dataset = '
                             f'{config.res_dataset}) at all times.\nPlease set config.res_samples <= '
                             f'config.res_dataset.')
        # resamplers (:147-176)
        self.gen_model_upsampler = make_upsampler(config.model_upsample_type, config.align_corners)
        self.disc_model_downsampler = make_downsampler(config.model_downsample_type, config.align_corners)
        # nonlinearity (:178-184)
        nl = config.nonlinearity.casefold()
        if nl == 'leaky relu':
            self.nl = LeakyReLU(negative_slope=config.leakiness)
        elif nl == 'relu':
            self.nl = LeakyReLU(negative_slope=0.)
        elif nl == 'tanh':
            self.nl = Tanh()
        else:
            raise ValueError("config does not support this nonlinearity.\nSupported nonlinearities are: "
                             "[ 'leaky relu', 'relu', 'tanh' ]")

        self.gen_model = None
        self.disc_model = None
        self.sn = None          # spectral_norm.SpectralNorm of the ResNet GAN critic (config.spectral_norm)
        self.gen_ema = None     # sampling.GeneratorEMA of the ResNet GAN generator (config.use_ewma_gen)
        # BigGAN's orthogonal regulariser (config.ortho_reg / config.ortho_reg_d; ortho_reg.py): managers over the arenas
        from .. import ortho_reg
        self._ortho_beta = ortho_reg.validate_config(config)
        # consistency regularisation (config.cr_*; consistency.py): None with every weight at 0 - nothing drawn, nothing launched
        from .. import consistency
        self.cr = consistency.validate_config(config)
        # feature quantisation of the critic (config.fq_*; quantize.py): the fields are checked here; the layer's kernels are not
        # in the package yet, so a valid fq_codes > 0 is refused and 0 builds nothing
        from .. import quantize
        quantize.require_layer(quantize.validate_config(config))
        # the power-spectrum regulariser of the progressive generators (config.spectrum_reg*; spectrum_reg.py): None with the weight
        # at 0 - nothing built, nothing launched; refused on a ResNet GAN config
        from .. import spectrum_reg
        self.spectrum_reg = spectrum_reg.from_config(config)
        self.ortho_g = self.ortho_d = None
        self._gradient_penalty = config.gradient_penalty
        self._optimizer = config.optimizer.casefold()
        self.opt_gen = self.opt_disc = None
        self._lr_sched = None
        self.sched_bool = False
        self.sched_stop_step = None
        self.scheduler_gen = self.scheduler_disc = None
        if config.lr_sched is not None:
            self._lr_sched = config.lr_sched.casefold()
            self.sched_bool = True
            self.sched_stop_step = 0
        self.valid_z = None
        self.curr_img_num = 0
        self.tot_num_epochs = None
        self.not_trained_yet = True
        self.ds_mean = self.ds_std = None
        self.data_config = None
        if self._model == 'ResNet GAN':
            self._init_resnet(config)

    # -- the non-progressive ResNet GAN (resnetgan/learner.py:98-120, :186-300) -------------------------
    def _init_resnet(self, config):
        from .architectures import (FMAP_D, FMAP_G, Discriminator32PixResnet, Discriminator64PixResnet,
                                    Generator32PixResnet, Generator64PixResnet)
        self.config = LearnerConfigCopy(config, self.__class__.__name__, NONREDEFINABLE_ATTRS,
                                        REDEFINABLE_FROM_LEARNER_ATTRS)
        self._is_data_configed = False
        self._update_data_config(raise_exception=False)
        self.batch_size = self.config.batch_size
        c = self.config
        if c.res_samples == 64:
            gen_cls, disc_cls, fmap_g, fmap_d = Generator64PixResnet, Discriminator64PixResnet, FMAP_G, FMAP_D
        elif c.res_samples == 32:
            gen_cls, disc_cls, fmap_g, fmap_d = Generator32PixResnet, Discriminator32PixResnet, FMAP_G * 2, FMAP_D * 2
        else:
            raise ValueError('GANLearner currently only supports 32 pixel and 64 pixel GAN architectures.\n'
                             'If a different generated sample resolution is desired, please use the\n'
                             'ProGAN or StyleGAN models featured in this package instead.')
        fmap_g = getattr(config, 'fmap_g', fmap_g)      # width override (tests / small runs)
        fmap_d = getattr(config, 'fmap_d', fmap_d)
        cgan_kw = {'cgan': True, 'num_classes': c.num_classes} if self.cgan else {'num_classes': 0}
        hier_kw = {k: v for k, v in (('hier_latent', self._hier_latent), ('shared_embed', self._shared_embed)) if v}
        self.gen_model = gen_cls(len_latent=c.len_latent, fmap=fmap_g, upsampler=self.gen_model_upsampler,
                                 blur_type=c.blur_type, nl=self.nl,
                                 equalized_lr=c.use_equalized_lr, **({'self_attention': True} if self._attn_g else {}),
                                 **cgan_kw, **hier_kw)
        from .. import spectral_norm
        sn_kw = {'spectral_norm': True} if spectral_norm.validate_config(config) else {}
        if self._attn_d:
            sn_kw['self_attention'] = True
        cgan_kw_d = dict(cgan_kw, cgan=self._cgan_mode, cond_embed=self._cond['embed']) if self._cond is not None else cgan_kw
        self.disc_model = disc_cls(fmap=fmap_d, pooler=self.disc_model_downsampler, blur_type=c.blur_type,
                                   nl=self.nl, equalized_lr=c.use_equalized_lr, **sn_kw, **cgan_kw_d)
        self.gen_model.to(c.dev)
        self.disc_model.to(c.dev)
        from .. import rng
        rng.seed_from_config(c.random_seed)
        assert self.gen_model.res == self.disc_model.res
        self.latent_distribution = c.latent_distribution
        self.reducer = parallel.GradReducer()
        self.log_every = getattr(config, 'log_every', 50)
        self.last_losses = {}
        self.last_metrics = {}      # compute_metrics: {'generator': {'prdc': {...}, 'fd': {...}, 'kid': {...}}}
        self._loss = config.loss.casefold()
        self._set_loss()
        self._make_arenas()
        self._set_optimizer()
        # the sampling side (config.use_ewma_gen / truncation / standing_stat_batches; sampling.py): the averaged generator
        from .. import sampling
        use_ema, ema_decay, ema_start, _, _ = sampling.validate_config(config)
        self.gen_ema = sampling.GeneratorEMA(self.gen_model, self.arena_g, ema_decay, ema_start) if use_ema else None
        if parallel.rank() == 0:
            print('-------- Initialized Model Configuration --------')
            print(self.config)
            print('-------------------------------------------------')
            print('\n    Ready to train!\n')

    def _make_arenas(self):
        self._graph_gen = getattr(self, '_graph_gen', 0) + 1    # captured step graphs point into the old arenas (graphs.py)
        self.arena_g = ParamArena(self.gen_model.named_parameters(), self.config.dev)
        self.arena_d = ParamArena(self.disc_model.named_parameters(), self.config.dev)
        parallel.broadcast_params(self.arena_g.flat)
        parallel.broadcast_params(self.arena_d.flat)
        if getattr(self.disc_model, 'spectral_norm', False):
            # the critic's normalised weights, u / v / sigma and their job table (spectral_norm.py): built over the new arena;
            # a new critic runs torch's 15 initial power iterations, a rebuild (checkpoint load) keeps the u, v it was given
            from ..spectral_norm import INIT_ITERS, SpectralNorm
            first = self.sn is None
            self.sn = SpectralNorm(self.disc_model, self.arena_d, init_iters=INIT_ITERS if first else 0)
            if parallel.is_dist():
                parallel.broadcast_params(self.sn.uv)       # u, v travel with the parameters
                self.sn.refresh(iterate=False)
        # the generator's modulation job table (hier_latent.py) points into its arena too: uploaded now, not inside a step
        if getattr(self.gen_model, 'hier', None) is not None and self.arena_g.flat.is_cuda:
            self.gen_model.hier.attach()
        # the orthogonal regulariser's job tables point into the arenas: rebuilt with them (no state of their own)
        from ..ortho_reg import OrthoReg
        beta_g, beta_d = self._ortho_beta
        self.ortho_g = OrthoReg(self.gen_model, self.arena_g, beta_g) if beta_g > 0 else None
        self.ortho_d = OrthoReg(self.disc_model, self.arena_d, beta_d) if beta_d > 0 else None
        # the averaged generator (sampling.py) reads the live parameters through their arena: re-pointed at a rebuilt one
        if getattr(self, 'gen_ema', None) is not None:
            self.gen_ema.rebind(self.gen_model, self.arena_g)

    def _set_optimizer(self):
        """resnetgan/learner.py:884-908, with every ``config.optimizer`` value built (the reference stops at Adam): the fused arena
        optimiser of that name through configure_optimizer_for_gan, which validates ``momentum`` / ``rmsprop_momentum``."""
        adam_gan = configure_optimizer_for_gan(self.config, optimizer=self._optimizer)
        self._graph_gen = getattr(self, '_graph_gen', 0) + 1
        self.opt_gen = adam_gan(params=list(self.gen_model.parameters()))
        self.opt_disc = adam_gan(params=list(self.disc_model.parameters()))

    def _set_scheduler(self):
        """resnetgan/learner.py:849-864."""
        if self._lr_sched == 'linear decay':
            self.scheduler_fn = lambda main_iter: 1. - (main_iter + self.sched_stop_step) * (1. / self.num_main_iters)
        elif self._lr_sched == 'custom':
            self.scheduler_fn = eval(self.config.lr_sched_custom)
        else:
            raise ValueError("config does not support this LR scheduler.\n"
                             "Currently supported LR Schedulers are: [ 'linear decay', 'custom' ]")
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            self.scheduler_gen = torch.optim.lr_scheduler.LambdaLR(self.opt_gen, self.scheduler_fn, last_epoch=-1)
            self.scheduler_disc = torch.optim.lr_scheduler.LambdaLR(self.opt_disc, self.scheduler_fn, last_epoch=-1)

    def set_requires_grad_disc(self, flag):
        for p in self.disc_model.parameters():
            p.requires_grad_(flag)
        if getattr(self, 'sn', None) is not None:
            self.sn.requires_grad_(flag)

    @property
    def use_step_graph(self):
        """config.use_step_graph / GANLAB_STEP_GRAPH: 1 = replay eligible iterations as HIP graphs (graphs.GraphedStep: the
        progressive learners), 0 = never, unset = where the step is launch-bound (resolutions up to 256).  The ResNet GAN's
        iteration is bound by its kernels (measured: 158.9 ms eager, 159.0 ms replayed) and always steps eagerly."""
        import os
        v = os.environ.get('GANLAB_STEP_GRAPH', getattr(self.config, 'use_step_graph', None))
        if v in (None, '', 'auto'):
            res = getattr(self.gen_model, 'curr_res', None) or self.config.res_samples
            return res <= 256
        return str(v).lower() not in ('0', 'false', 'no')

    # -- the hot path: one generator iteration, one critic iteration ------------------------------------
    def _augment(self, x, params):
        """The critic's view of ``x`` under ``self.critic_aug`` (DiffAugment or ADA) with ``params`` (None: a fresh draw)."""
        if params is None:
            params = self.critic_aug.draw(x.shape[0], x.shape[2], x.shape[3], x.device)
        return self.critic_aug(x, params)

    def _ada_update(self, d_real):
        """After the critic's forward of a D step: feed sign(D(real)) to the ADA controller (adaptive p only)."""
        if self.ada is not None and self.ada.adaptive:
            self.ada.update(d_real.detach())

    def _ada_checkpoint_fields(self):
        return {} if self.ada is None else {'ada_state': self.ada.state_dict()}

    def _restore_ada(self, ck):
        if self.ada is not None and ck.get('ada_state') is not None:
            self.ada.load_state_dict(ck['ada_state'])

    def _device_labels(self, labels, n, draw):
        """The labels of a step as ops take them (``config.cgan``; None without it): an (n,) int32 device tensor.  A CPU tensor
        (what the loaders yield) is range-checked on the host and uploaded; a device tensor is taken as it is - the kernels clamp,
        nothing is read back.  None: ``draw`` them uniformly from the project's Philox stream (the generator step), else raise."""
        if not self.cgan:
            if labels is not None:
                raise ValueError("labels were passed but config.cgan is None: this learner is not class-conditional")
            return None
        k = self.config.num_classes
        if labels is None:
            if not draw:
                raise ValueError(f"config.cgan={self._cgan_mode!r}: d_step needs the labels of the real batch (labels=...)")
            from .. import rng
            return rng.randint(n, k, self.config.dev)
        if isinstance(labels, torch.Tensor) and labels.is_cuda:
            if tuple(labels.shape) != (n,) or labels.dtype not in (torch.int32, torch.int64):
                raise ValueError(f'labels must be an int32 / int64 tensor of shape ({n},) (got {labels.dtype}, '
                                 f'{tuple(labels.shape)})')
            return labels.to(torch.int32)
        from .. import conditional
        return conditional.check_host_labels(labels, k, n).to(self.config.dev, non_blocking=True)

    def _gen(self, zb, labels):
        return self.gen_model(zb, labels) if self.cgan else self.gen_model(zb)

    def _disc(self, x, labels):
        return self.disc_model(x, labels) if self.cgan else self.disc_model(x)

    @property
    def _cond_on(self):
        """Does a step launch the classifier-based conditioning term (``config.cgan`` in 'contra' / 'reacgan' with
        ``config.cond_lambda`` > 0)?  With the weight at 0 the heads exist and nothing is launched."""
        return self._cond is not None and self._cond['weight'] > 0

    def _add_cond_term(self, loss, feat, labels, name):
        """``loss + cond_lambda * term`` with the term of the critic's classifier head on the feature rows ``feat`` (from the
        critic pass that produced the scores: the trunk is never run twice) and their labels; per rank, nothing is gathered."""
        from .. import conditional
        term = conditional.cond_term(self.disc_model, feat, labels, self._cond)
        self.last_losses[name] = term.detach()      # unweighted; a device tensor: no host synchronisation
        return loss + self._cond['weight'] * term

    def g_step(self, zb=None, aug_params=None, labels=None, cr_noise=None):
        """resnetgan/learner.py:545-597 (critic parameters frozen by the caller).  ``aug_params``: the DiffAugment rows
        of the generated batch (tests; drawn when None).  ``labels`` (``config.cgan``): the classes to generate, drawn
        uniformly on the device when None.  ``cr_noise`` (``config.cr_latent_g``): the latent perturbation n of
        ``z' = z + cr_sigma * n`` (tests; drawn when None)."""
        c = self.config
        self.arena_g.zero_grad()
        if self.sn is not None:
            self.sn.refresh(iterate=False)      # the critic's weights moved: sigma and W_sn follow, u and v stay
        if zb is None:
            zb = gen_rand_latent_vars(num_samples=self.batch_size * c.gen_bs_mult, length=c.len_latent,
                                      distribution=self.latent_distribution, device=c.dev)
        labels = self._device_labels(labels, zb.shape[0], draw=True)
        cr_term = None
        if self.cr is not None and self.cr.latent_g > 0:
            # zCR, generator side: ONE pass over [z; z'] (BatchNorm statistics over both halves; consistency.py); the first
            # half goes on to the critic, the term's gradient reaches both halves as a single (2N, C, H, W) cotangent
            n = zb.shape[0]
            both = self._gen(torch.cat((zb, self.cr.perturb(zb, cr_noise))),
                             torch.cat((labels, labels)) if labels is not None else None)
            cr_term = ops.cr_imsd(both)
            fake = both[:n]
        else:
            fake = self._gen(zb, labels)
        if self.critic_aug is not None:
            fake = self._augment(fake, aug_params)
        feat = None
        if self._cond_on:
            out, feat = self.disc_model(fake, labels, return_features=True)
        else:
            out = self._disc(fake, labels)
        # :573-578 - the minimax generator loss here is -BCE(D(G(z)), 0), like backprop_utils
        loss = self.loss_func_gen(out)
        if feat is not None:        # the classifier-based conditioning term on the generated rows, with the generator's labels
            loss = self._add_cond_term(loss, feat, labels, 'cond_g')
        if cr_term is not None:
            loss = loss - self.cr.latent_g * cr_term
            self.last_losses['cr_latent_g'] = cr_term.detach()      # unweighted; a device tensor: no host synchronisation
        self.reducer.arm(self.arena_g)
        with ops.direct_param_grads(ops.direct_grads_enabled()):      # first-use gradients land in the arena directly
            loss.backward()
        self.reducer.allreduce(self.arena_g.gflat)
        if self.ortho_g is not None:            # rank-independent, so added after the reduction: every rank adds the same term
            self.ortho_g.apply()
            self.last_losses['ortho_g'] = self.ortho_g.penalty      # a device tensor: no host synchronisation
        self.opt_gen.step()
        if self.gen_ema is not None:
            self.gen_ema.update()
        return loss.detach()

    def generate(self, zs=None, n=None, labels=None, truncation=FROM_CONFIG, time_average=True, standing_stats=False):
        """Images of the generator, sampled as BigGAN samples (sampling.py), under ``torch.no_grad()``.  ``zs``: the latents
        (n, len_latent); None: ``n`` (default: the batch size) fresh ones from the process stream, from the standard normal
        truncated to [-truncation, truncation] (default ``config.truncation``; None: untruncated).  ``labels`` (``config.cgan``):
        as in ``g_step``, drawn uniformly when None.  ``time_average``: sample the averaged generator where there is one
        (``config.use_ewma_gen``), else - and without one - the live generator in eval mode, whose train / eval state is put
        back afterwards.  ``standing_stats`` (True: ``config.standing_stat_batches`` batches, or their number): first re-estimate
        the BatchNorm statistics of the sampled network, which overwrites its running statistics."""
        from .. import rng, sampling
        c = self.config
        if truncation is FROM_CONFIG:
            truncation = getattr(c, 'truncation', None)
        if truncation is not None:
            truncation = ops.check_truncation(truncation, 'truncation')
        if zs is None:
            n = self.batch_size if n is None else int(n)
            if n < 1:
                raise ValueError(f'generate: n must be >= 1 (got {n})')
            zs = rng.randn((n, c.len_latent), c.dev) if truncation is None else \
                rng.trunc_randn((n, c.len_latent), truncation, c.dev)
        elif n is not None and int(n) != zs.shape[0]:
            raise ValueError(f'generate: {zs.shape[0]} latents were passed with n={n}')
        labels = self._device_labels(labels, zs.shape[0], draw=True)
        net = self.gen_ema.model if (time_average and self.gen_ema is not None) else self.gen_model
        was_training = net.training
        with torch.no_grad():
            try:
                if standing_stats:
                    batches = getattr(c, 'standing_stat_batches', 16) if standing_stats is True else standing_stats
                    draw = (lambda b: self._device_labels(None, b, draw=True)) if self.cgan else None
                    sampling.standing_stats(net, batches, self.batch_size, c.len_latent, labels_fn=draw, truncation=truncation)
                net.eval()
                return net(zs, labels) if self.cgan else net(zs)
            finally:
                net.train(was_training)

    def compute_metrics(self, metrics, metrics_type, z_valid_dl, valid_dl=None):
        """Validation metrics of the ResNet GAN over the validation latents and reals: ``'prdc'`` - improved precision / recall
        and density / coverage (prdc.py) -, ``'fd'`` - the Frechet distance (frechet.py) - and ``'kid'`` - the Kernel Inception
        Distance (kid.py); any other entry raises.  The generated set is
        ``generate(zs=zb, truncation=None, time_average=True)`` per batch of ``z_valid_dl`` (the averaged generator where there
        is one; with ``config.cgan`` the classes are drawn as ``generate`` draws them), the real set the batches of ``valid_dl``,
        both reduced to rows by ``prdc.features`` (at ``prdc_res`` / ``fd_res`` / ``kid_res``) and truncated to min(latents, reals)
        in whole batches; the images are generated once for all metrics.  The process stream is put back where it was, so an
        evaluation does not move the training run.  Returns the formatted lines; the numbers are kept in
        ``self.last_metrics['generator'][name]``."""
        from .. import rng, validation
        c = self.config
        metrics_type = metrics_type.casefold()
        if metrics_type not in ('generator', 'critic', 'discriminator'):
            raise Exception('Invalid metrics_type. Only "generator", "critic", or "discriminator" are accepted.')
        metrics = [m.casefold() for m in metrics]
        unsupported = [m for m in metrics if m not in [s.name for s in validation.ROW_SCORERS]]
        if unsupported:
            raise ValueError(f"the ResNet GAN learner computes 'prdc', 'fd' and 'kid' only; unsupported metrics: {unsupported}")
        if not metrics:
            return []
        first = "'" + metrics[0] + "'"
        if metrics_type != 'generator':
            raise ValueError(f"{first} is a generator metric: it compares the generated validation images with the validation "
                             f"reals and cannot be listed among the critic's metrics (config.disc_metrics)")
        if z_valid_dl is None or valid_dl is None:
            raise ValueError(f"{first} needs the validation latents and reals: pass z_valid_dl and valid_dl "
                             f"(train(train_dl, valid_dl, z_valid_dl))")
        n_use = min(len(z_valid_dl.dataset), len(valid_dl.dataset)) // self.batch_size * self.batch_size
        if n_use < 1:
            raise ValueError(f"{first} needs at least one whole batch of {self.batch_size} validation latents and reals (got "
                             f"{len(z_valid_dl.dataset)} and {len(valid_dl.dataset)})")
        scorers = [s(self, c.res_samples, len(z_valid_dl.dataset), valid_dl) for s in validation.ROW_SCORERS if s.name in metrics]
        offset, left, valid_iter = rng._STATE['offset'], n_use, iter(valid_dl)
        try:
            for zbatch in z_valid_dl:
                if left <= 0:
                    break
                zb = zbatch[0].to(c.dev).float()
                xb = next(valid_iter)[0].to(c.dev).float()
                if len(zb) != len(xb) or len(zb) > left:
                    raise ValueError(f"{first}: validation latents and reals must come in equal batches (got {len(zb)} and "
                                     f"{len(xb)} with {left} images to go)")
                xgen = self.generate(zs=zb, truncation=None, time_average=True)
                for s in scorers:
                    s.feed(len(zb), xgen, xb)
                left -= len(zb)
        finally:
            rng._STATE['offset'] = offset
        out, lines = {}, []
        for s in scorers:
            out[s.name], lines_of = s.finish()
            lines += lines_of
        self.last_metrics[metrics_type] = out
        return ['    ' + ('%-12s' % (name + ':')) + '%.4g' % v + '\n' for name, v in lines]

    def _pair_critic_batches(self, xgenb, xb):
        """May the critic see the generated and the real batch as one?  Only when no critic layer couples samples (a
        BatchNorm would take its statistics over both) and the output is the plain score.  GANLAB_RESNET_PAIR=0: A/B."""
        if os.environ.get('GANLAB_RESNET_PAIR') == '0' or xgenb.numel() != xb.numel():
            return False
        key, ok = getattr(self, '_pairable', (None, False))
        if key != id(self.disc_model):
            ok = not any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in self.disc_model.modules()) and \
                not hasattr(self.disc_model, 'linear_aux')
            self._pairable = (id(self.disc_model), ok)
        return ok

    def d_step(self, xb, zb=None, eps_interp=None, aug_params=None, labels=None, cr_noise=None, cr_params=None):
        """resnetgan/learner.py:606-672: generator frozen but in train mode (its BatchNorm running
        statistics keep moving, :621-622); no drift term on this path.  ``aug_params``: the DiffAugment rows, [0, B) for
        the generated batch and [B, 2B) for the real one (tests; drawn when None).  ``labels`` (``config.cgan``; required
        then): the real batch's classes; the generated batch is produced with the SAME labels, so that row i of a WGAN-GP
        interpolate lies between two images of one class.  ``cr_noise`` / ``cr_params`` (``config.cr_*``; tests, drawn when
        None): the latent perturbation n of ``z' = z + cr_sigma * n``, and the (2B, 4) int32 transform rows, [0, B) for the
        generated batch and [B, 2B) for the real one."""
        c = self.config
        labels = self._device_labels(labels, xb.shape[0], draw=False)
        self.arena_d.zero_grad()
        if self.sn is not None:
            self.sn.refresh(iterate=True)       # ONE power iteration per critic update (spectral_norm.py)
        if zb is None:
            zb = gen_rand_latent_vars(num_samples=self.batch_size, length=c.len_latent,
                                      distribution=self.latent_distribution, device=c.dev)
        if labels is not None and zb.shape[0] != labels.shape[0]:
            raise ValueError(f'd_step: {zb.shape[0]} latents for {labels.shape[0]} labelled real images')
        cr = self.cr
        xgen_p = None
        with torch.no_grad():
            if cr is not None and cr.latent_d > 0:
                # zCR, critic side: ONE generator pass over [z; z'] with the same labels - its BatchNorm statistics are taken
                # over both halves (consistency.py)
                both = self._gen(torch.cat((zb, cr.perturb(zb, cr_noise))),
                                 torch.cat((labels, labels)) if labels is not None else None)
                xgenb, xgen_p = both[:zb.shape[0]], both[zb.shape[0]:]
            else:
                xgenb = self._gen(zb, labels)
        n, aug = xgenb.shape[0], self.critic_aug
        # the further critic inputs of the consistency terms, in this order: T(x), T(G(z)), G(z') - only those with a weight
        extra = []
        if cr is not None:
            if cr.balanced:
                if xb.shape[0] != n:
                    raise ValueError(f'd_step: bCR needs as many real as generated images (got {xb.shape[0]} and {n})')
                cr_params = cr.draw_params(n, xb.device) if cr_params is None else cr.check_params(cr_params, n)
            if cr.real > 0:
                extra.append(('cr_real', cr.real, cr.transform(xb.reshape(xgenb.shape), cr_params[n:])))
            if cr.fake > 0:
                extra.append(('cr_fake', cr.fake, cr.transform(xgenb, cr_params[:n])))
            if xgen_p is not None:
                extra.append(('cr_latent_d', cr.latent_d, xgen_p))
        if aug is not None and aug_params is None:
            aug_params = aug.draw(n + xb.shape[0], xb.shape[2], xb.shape[3], xb.device)
        if self._pair_critic_batches(xgenb, xb):
            # one critic pass over [generated; real]: every critic layer is per-sample (LayerNorm), so the outputs are the
            # two separate passes' (resnetgan/learner.py:640-651) and each parameter gets ONE gradient contribution from
            # the pair instead of two - half the launches of the first-order critic work at this launch-bound size
            both = torch.cat((xgenb, xb.reshape(xgenb.shape)))
            if aug is not None:        # one launch over the pair: per sample, the same as two
                both = aug(both, aug_params)
                xgenb, xb = both[:n], both[n:]
            # the consistency terms' inputs ride along behind the pair: rows [0, 2n) stay [generated; real]
            parts = 2 + len(extra)
            if extra:
                both = torch.cat([both] + [x for _, _, x in extra])
            f_real = None
            if self._cond_on:
                out, feat = self.disc_model(both, torch.cat((labels,) * parts), return_features=True)
                f_real = feat[n:2 * n]      # the real rows only: generated rows and the consistency terms' rows stay out
            else:
                out = self._disc(both, torch.cat((labels,) * parts) if labels is not None else None)
            d_gen, d_real = out[:n], out[n:2 * n]
            d_extra = [out[(2 + i) * n:(3 + i) * n] for i in range(len(extra))]
        else:
            if aug is not None:
                xgenb, xb = aug(xgenb, aug_params[:n]), aug(xb, aug_params[n:])
            f_real = None
            d_gen = self._disc(xgenb, labels)
            if self._cond_on:
                d_real, f_real = self.disc_model(xb, labels, return_features=True)
            else:
                d_real = self._disc(xb, labels)
            d_extra = [self._disc(x, labels) for _, _, x in extra]
        loss = self.loss_func_disc(d_gen, d_real)
        for (name, weight, _), d_x in zip(extra, d_extra):
            term = ops.cr_msd(d_real if name == 'cr_real' else d_gen, d_x)
            loss = loss + weight * term
            self.last_losses[name] = term.detach()      # unweighted; a device tensor: no host synchronisation
        if f_real is not None:      # the classifier-based conditioning term on the real rows, with the real labels
            loss = self._add_cond_term(loss, f_real, labels, 'cond_d')
        self._ada_update(d_real)
        if self.gradient_penalty is not None:
            loss = loss + self.calc_gp(xgenb, xb, eps_interp=eps_interp, labels=labels)
        # With spectral normalisation the normalised layers' gradients reach the arena only in ``sn.backward()``, after the
        # sweep: no bucket of the critic arena may leave from inside the backward, so the reducer is not armed and
        # ``allreduce`` sends the whole arena afterwards.
        if self.sn is None:
            self.reducer.arm(self.arena_d)
        with ops.direct_param_grads(ops.direct_grads_enabled()):
            loss.backward()
        if self.sn is not None:
            self.sn.backward()
        self.reducer.allreduce(self.arena_d.gflat)
        if self.ortho_d is not None:
            self.ortho_d.apply()
            self.last_losses['ortho_d'] = self.ortho_d.penalty
        self.opt_disc.step()
        return loss.detach()

    def train(self, train_dl, valid_dl=None, z_valid_dl=None, num_main_iters=None, num_gen_iters=None,
              num_disc_iters=None):
        """GAN training, generator first (resnetgan/learner.py:463-700); re-entrant like the reference."""
        c = self.config
        num_main_iters = c.num_main_iters if num_main_iters is None else num_main_iters
        num_gen_iters = c.num_gen_iters if num_gen_iters is None else num_gen_iters
        num_disc_iters = c.num_disc_iters if num_disc_iters is None else num_disc_iters
        self.num_main_iters = num_main_iters
        self.dataset_sz = len(train_dl.dataset)
        self._update_data_config(raise_exception=False)
        self.gen_model.to(c.dev).train()
        self.disc_model.to(c.dev).train()
        if self.sched_bool:
            if not self.pretrained_model:
                self.sched_stop_step = 0
            self._set_scheduler()
        if self.not_trained_yet or self.pretrained_model:
            self.train_dataiter = iter(train_dl)
        if parallel.rank() == 0:
            print('STARTING FROM ITERATION 0:\n' if self.not_trained_yet else 'CONTINUING FROM WHERE YOU LEFT OFF:\n')
        if self.tot_num_epochs is None:
            per_epoch = max(self.dataset_sz // self.batch_size * self.batch_size, 1)
            self.tot_num_epochs = num_main_iters * self.batch_size * num_disc_iters // per_epoch + 1
        loss_d = loss_g = None
        # the validation metrics of this learner ('prdc' / 'fd' / 'kid' in config.gen_metrics; compute_metrics): with both
        # loaders only
        from .. import validation
        valid_metrics = [s.name for s in validation.ROW_SCORERS if s.module.wanted(c.gen_metrics)]
        want_valid = bool(valid_metrics) and valid_dl is not None and z_valid_dl is not None
        try:
            for itr in range(num_main_iters):
                # ---------------------------- TRAIN GENERATOR ----------------------------
                self.set_requires_grad_disc(False)
                for _ in range(num_gen_iters):
                    loss_g = self.g_step()
                if want_valid and ((itr + 1) % c.num_iters_valid == 0 or itr == 0):
                    vals = self.compute_metrics(metrics=valid_metrics, metrics_type='Generator', z_valid_dl=z_valid_dl,
                                                valid_dl=valid_dl)
                    if parallel.rank() == 0:
                        print('|\n', 'Generator Validation Metrics:\n', *vals)
                # -------------------------- TRAIN DISCRIMINATOR --------------------------
                self.set_requires_grad_disc(True)
                for _ in range(num_disc_iters):
                    batch = next(self.train_dataiter, None)
                    if batch is None:
                        self.curr_epoch_num += 1
                        self.train_dataiter = iter(train_dl)
                        batch = next(self.train_dataiter)
                    xb = batch[0].to(c.dev, non_blocking=True).float()
                    # config.cgan: the batch's labels, range-checked while they are still on the host (_device_labels)
                    loss_d = self.d_step(xb, labels=batch[1] if self.cgan else None)
                    self.curr_dataset_batch_num += 1
                    self.curr_img_num += self.batch_size
                if self.sched_bool:
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore')
                        self.scheduler_gen.step()
                        self.scheduler_disc.step()
                self.not_trained_yet = False
                if self.log_every and (itr % self.log_every == 0 or itr == num_main_iters - 1):
                    self.last_losses = dict(itr=itr, loss_d=float(loss_d) if loss_d is not None else None,
                                            loss_g=float(loss_g) if loss_g is not None else None,
                                            res=c.res_samples, batch=self.batch_size,
                                            **{k: v for k, v in self.last_losses.items() if k.startswith(('ortho_', 'cr_', 'cond_'))})
                    if parallel.rank() == 0:
                        print(('%9s' * 5) % (f'{self.curr_epoch_num}/{self.tot_num_epochs}',
                                             f'{c.res_samples}X{c.res_samples}',
                                             '%.4g' % (self.last_losses['loss_d'] or 0.),
                                             '%.4g' % (self.last_losses['loss_g'] or 0.), itr))
                if (itr + 1) % c.num_iters_save_model == 0:
                    self.save_model(c.save_model_dir / (self.model.casefold().replace(' ', '') + '_model.tar'))
        except KeyboardInterrupt:
            # resnetgan/learner.py: Ctrl-C saves the latest checkpoint before the run ends
            self.set_requires_grad_disc(True)
            self.reducer.abandon()          # no collective in the interrupt path (ranks are at different points)
            if not self.not_trained_yet:
                self.save_model(c.save_model_dir / (self.model.casefold().replace(' ', '') + '_model.tar'), sync=False)
                if parallel.rank() == 0:
                    print(f'\nTraining interrupted. Saved latest checkpoint into "{c.save_model_dir}/".\n')
            raise

    def save_model(self, save_path, sync=True, reference_format=False):
        """Checkpoint as plain data (key names follow resnetgan/learner.py:1076-1140).  ``sync=False``: no barrier
        behind rank 0's write (the interrupt path).  ``reference_format``: this learner writes plain-data checkpoints only;
        with spectral normalisation, self-attention, class conditioning or the hierarchical latent / shared embedding on the
        request is refused as a ValueError (the reference cannot hold u, v, the block, the tables or the modulation)."""
        from .. import spectral_norm
        spectral_norm.check_save_format(bool(getattr(self.config, 'spectral_norm', False)), reference_format)
        from .. import attention
        attention.check_save_format(getattr(self.config, 'self_attention', None), reference_format)
        from .. import conditional
        conditional.check_save_format(getattr(self.config, 'cgan', None), reference_format)
        from .. import hier_latent
        hier_latent.check_save_format(getattr(self.config, 'hier_latent', False), getattr(self.config, 'shared_embed', 0),
                                      reference_format)
        from .. import sampling
        sampling.check_save_format(self.gen_ema is not None, reference_format)
        from .. import optim
        optim.check_save_format(self._optimizer, reference_format)
        if reference_format:
            raise NotImplementedError('the ResNet GAN learner writes plain-data checkpoints only')
        if self.not_trained_yet:
            raise Exception('Please train your model for atleast 1 iteration before saving.')
        from .. import checkpoint as ckpt
        tcpu = lambda v: None if v is None else v.detach().cpu()  # noqa: E731
        sched_steps = max(self.scheduler_gen._step_count - 1, 0) if (self.sched_bool and self.scheduler_gen) else 0
        from .. import consistency, quantize
        ck = {
            'config': ckpt.saved_config_fields({k: v for k, v in
                                                conditional.saved_config_fields(consistency.saved_config_fields(
                                                    quantize.saved_config_fields(sampling.saved_config_fields(
                                                        optim.saved_config_fields(vars(self.config), self._optimizer))))).items()
                                                if not k.startswith('_') and
                                                isinstance(v, (int, float, str, bool, dict, list, tuple, type(None))) and
                                                not (k in ('self_attention', 'cgan') and v is None) and
                                                not (k in ('hier_latent', 'shared_embed') and not v)}),
            'gen_model_state_dict': {k: v.detach().cpu() for k, v in self.gen_model.state_dict().items()},
            'disc_model_state_dict': {k: v.detach().cpu() for k, v in self.disc_model.state_dict().items()},
            'opt_gen_state_dict': self.opt_gen.export_moments(self.gen_model.named_parameters()),
            'opt_disc_state_dict': self.opt_disc.export_moments(self.disc_model.named_parameters()),
            'sched_stop_step': (self.sched_stop_step or 0) + sched_steps if self.sched_bool else self.sched_stop_step,
            'lr_sched': self.lr_sched, 'optimizer': self.optimizer,
            'loss': self.loss, 'gradient_penalty': self.gradient_penalty, 'batch_size': self.batch_size,
            'curr_dataset_batch_num': self.curr_dataset_batch_num, 'curr_epoch_num': self.curr_epoch_num,
            'tot_num_epochs': self.tot_num_epochs, 'curr_img_num': self.curr_img_num,
            'not_trained_yet': self.not_trained_yet,
            'ds_mean': tcpu(self.ds_mean), 'ds_std': tcpu(self.ds_std), 'valid_z': tcpu(self.valid_z),
        }
        ck.update(self._ada_checkpoint_fields())
        if self.gen_ema is not None:        # the averaged generator: only with config.use_ewma_gen, else the keys of always
            ema = self.gen_ema.state_dict()
            ck['gen_ema_state_dict'], ck['ewma_updates'] = ema['model'], ema['updates']
        if parallel.rank() == 0:            # replicas are identical: one writer, atomically; everyone waits for the file
            ckpt.save_atomic(ck, save_path)
        if sync:
            parallel.barrier()

    def load_model(self, load_path, dev_of_saved_model='cpu'):
        from .. import checkpoint as ckpt
        ck = ckpt.load_checkpoint(load_path, dev_of_saved_model)
        from .. import optim
        optim.check_saved_optimizer(ck.get('optimizer'), self._optimizer)
        self.gen_model.load_state_dict(ck['gen_model_state_dict'])
        self.disc_model.load_state_dict(ck['disc_model_state_dict'])
        self.gen_model.to(self.config.dev)
        self.disc_model.to(self.config.dev)
        self._make_arenas()
        self._set_optimizer()
        self.opt_gen.import_moments(self.gen_model.named_parameters(), ck['opt_gen_state_dict'])
        self.opt_disc.import_moments(self.disc_model.named_parameters(), ck['opt_disc_state_dict'])
        for k in ('sched_stop_step', 'batch_size', 'curr_dataset_batch_num', 'curr_epoch_num', 'tot_num_epochs',
                  'curr_img_num', 'not_trained_yet'):
            setattr(self, k, ck[k])
        if ck.get('ds_mean') is not None and ck.get('ds_std') is not None:
            self.ds_mean, self.ds_std = ck['ds_mean'].float().cpu(), ck['ds_std'].float().cpu()
        if ck.get('valid_z') is not None:
            self.valid_z = ck['valid_z'].to(self.config.dev)
        self._restore_ada(ck)
        if self.gen_ema is not None:
            if ck.get('gen_ema_state_dict') is not None:
                self.gen_ema.load_state_dict({'model': ck['gen_ema_state_dict'], 'updates': ck.get('ewma_updates', 0)})
            else:       # a checkpoint from before the option (or saved without it): the average starts from the loaded generator
                self.gen_ema.reset()
        self.pretrained_model = True

    # -- gradient penalty (resnetgan/learner.py:780-827) ------------------------------------------------
    def calc_gp(self, gen_data, real_data, eps_interp=None, labels=None):
        """Method that takes care of all gradient regularizers (double backward through HIP kernels).  ``labels``
        (``config.cgan``): the critic is evaluated as a closure over the batch's labels."""
        disc = self.disc_model if labels is None else (lambda x: self.disc_model(x, labels))
        return bp.calc_gp(disc, self.gradient_penalty, gen_data, real_data, lda=self.config.lda,
                          gamma=self.config.gamma, eps_interp=eps_interp)

    # -- redefinable-from-learner properties (:831-946) -------------------------------------------------
    @property
    def lr_sched(self):
        return self._lr_sched

    @lr_sched.setter
    def lr_sched(self, new_lr_sched):
        self._lr_sched = None
        self.sched_bool = False
        self.scheduler_gen = self.scheduler_disc = None
        if new_lr_sched is not None:
            self._lr_sched = new_lr_sched.casefold()
            self.sched_bool = True
            if not self.pretrained_model:
                self.sched_stop_step = 0

    @property
    def optimizer(self):
        return self._optimizer

    @optimizer.setter
    def optimizer(self, new_optimizer):
        self._optimizer = new_optimizer.casefold()
        self._set_optimizer()

    @property
    def gradient_penalty(self):
        return self._gradient_penalty.casefold() if self._gradient_penalty is not None else None

    @gradient_penalty.setter
    def gradient_penalty(self, new_gradient_penalty):
        if new_gradient_penalty is not None and getattr(self, '_attn_d', False):
            raise ValueError('the critic has a self-attention block (config.self_attention): the double backward of a gradient '
                             'penalty through attention is not provided; keep gradient_penalty=None (hinge + spectral norm)')
        self._gradient_penalty = new_gradient_penalty.casefold() if new_gradient_penalty is not None else None

    @property
    def loss(self):
        return self._loss

    @loss.setter
    def loss(self, new_loss):
        self._loss = new_loss.casefold()
        self._set_loss()

    def _set_loss(self):
        if self._loss not in ('wgan', 'nonsaturating', 'minimax',) and \
                not (self._loss == 'hinge' and self._model == 'ResNet GAN'):
            raise ValueError("config does not support this loss.\nCurrently supported Loss Functions are: "
                             "[ 'wgan', 'nonsaturating', 'minimax' ] (ResNet GAN: also 'hinge')")
        # the BCE targets are constants folded into the loss kernels (no cached ones/zeros tensors,
        # cf. resnetgan/learner.py:937-938)
        self.loss_func_gen = lambda outb: bp.loss_gen(self._loss, outb)
        self.loss_func_disc = lambda outb, yb: bp.loss_disc(self._loss, outb, yb)

    @property
    def model(self):
        return self._model

    @model.setter
    def model(self, new_model):
        raise AttributeError(
            f"{self.__class__.__name__}().model attribute cannot be changed once {self.__class__.__name__} is "
            f"instantiated.\nInstead, please run 'python config.py {new_model}' and then instantiate a new "
            f"{self.__class__.__name__}.")

    # -- data config (resnetgan/learner.py:1051-1072) ----------------------------------------------------
    def _update_data_config(self, raise_exception=True):
        dc = get_current_configuration('data_config', raise_exception=raise_exception)
        if dc is not None:
            self.data_config = dc
            if not self.pretrained_model and getattr(dc, 'ds_mean', None) is not None:
                self.ds_mean = torch.FloatTensor(dc.ds_mean).unsqueeze(dim=1).unsqueeze(dim=2)
                self.ds_std = torch.FloatTensor(dc.ds_std).unsqueeze(dim=1).unsqueeze(dim=2)
        self._is_data_configed = self.data_config is not None
