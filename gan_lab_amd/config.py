#!/usr/bin/env python3
"""Model configuration CLI / factory (drop-in surface of gan_lab/config.py).

``python -m gan_lab_amd.config stylegan --loss=nonsaturating --gradient_penalty=r1 ...`` parses the
same arguments with the same defaults as the reference (config.py:81-325), post-processes them the
same way (:337-376: torch.device, seeding, ``bs_dict`` rebuilt from ``--batch_size`` with 512 ->
bs//2 and 1024 -> bs//4) and pickles the Namespace to ``<this dir>/.config.p`` with the pointer file
``~/.configs_dir.txt`` (:408-412), which ``get_current_configuration('config')`` reads back.
``make_config(model, **overrides)`` builds the same Namespace in-process (tests, bench.py).
New, optional fields (ignored by the reference): ``log_every``, ``compute_dtype`` ('f32' = the reference's
arithmetic, 'bf16' = BASELINE config #2: bf16-compute 3x3 convolutions with fp32 storage / masters), ``diffaugment``
(None = off, or a DiffAugment policy such as 'color,translation,cutout' applied to every critic input: augment.py;
validated when the learner is built), ``ada`` (None = off, or an ADA policy, a comma-separated subset of blit, geom,
color, filter, noise, cutout in that order such as 'blit,geom,color' or 'blit,geom,color,filter,noise,cutout': ada.py) with
``ada_p`` (initial, or fixed, augmentation probability), ``ada_target`` (the r_t the controller steers to; None =
fixed p), ``ada_interval`` (critic iterations per adjustment) and ``ada_kimg`` (thousands of images for p to travel 0 -> 1);
``'swd'`` as an entry of ``gen_metrics`` (the sliced Wasserstein distance of swd.py between the validation reals and the generated
validation images) with ``swd_nhoods`` (neighbourhoods per image and level), ``swd_dir_repeats`` x ``swd_dirs_per_repeat``
(projection directions) and ``swd_seed``, validated when the learner is built; ``'msssim'`` as an entry of ``gen_metrics`` (the
multi-scale structural similarity of msssim.py between adjacent pairs of the generated validation images: the paper's
mode-collapse indicator, lower = more diverse) with ``msssim_range``, the dynamic range L behind C1 = (0.01 L)^2 and
C2 = (0.03 L)^2.  Images are scored in the network's own space, normalised by the dataset's mean and standard deviation, so the
natural range depends on the dataset: the default 2.0 fits images spanning [-1, 1]; compare a run's ``msssim fake`` with its own
``msssim real`` line rather than with numbers from another dataset or range; ``'spectrum'`` as an entry of ``gen_metrics`` (the
radial power-spectrum distance of spectrum.py between the generated validation images and the validation reals, in dB over all
radii and over the upper half of them: the number that moves when an upsample, a blur or a low-precision plane bends the
high-frequency tail) with ``spectrum_window``: ``'hann'`` (the default) tapers each image with a periodic Hann window before the
transform, so that the jump between opposite image borders does not leak a 1/f^2 cross into every radius; ``'none'`` transforms
the image as it is (right for periodic textures, and the setting under which a circular shift leaves the profile unchanged);
``'prdc'`` as an entry of ``gen_metrics`` (improved precision / recall and density / coverage of prdc.py between the generated
validation images and the validation reals: k-nearest-neighbour statistics that separate fidelity from diversity and need no
pretrained network; all three models) with ``prdc_k`` (the neighbour that sets a row's radius, in [1, 16], default 5) and
``prdc_res`` (a power of two >= 4, default 32: images are reduced by 2x2 means to at most this size and flattened into the feature
rows), validated when the learner is built;
``'fd'`` and ``'kid'`` as entries of ``gen_metrics`` (all three models): the Frechet distance (frechet.py) and the Kernel Inception
Distance (kid.py: the unbiased MMD^2 under the cubic polynomial kernel, over the whole sets and as mean / standard deviation over
blocks of ``kid_block`` rows, default 1000, >= 2) between the generated validation images and the validation reals.  The feature
rows are ``prdc.features`` of the images at ``fd_res`` (default 16: 768 features for RGB, so the host-side eigenproblems of the
distance stay well under a second) and ``kid_res`` (default 32), powers of two >= 4 like ``prdc_res``; with rows of a pretrained
embedding fed to ``frechet.Frechet`` / ``kid.KID`` by hand the numbers are FID and KID proper.  Validated when the learner is
built;
``spectral_norm`` (ResNet GAN only; False = off): every Conv2dEx / LinearEx weight of the critic is divided by its largest
singular value, estimated by one power iteration per critic update (spectral_norm.py; excludes ``use_equalized_lr``; validated
when the learner is built), and ``loss='hinge'`` (ResNet GAN only) is the loss usually trained with it - with both on,
``gradient_penalty=None`` is a sane setting; ``self_attention`` (ResNet GAN only; None = off, ``'g'``, ``'d'`` or ``'gd'``;
``--self_attention=none`` on the command line) adds a SAGAN self-attention block (attention.py: fused exact-fp32 kernels, the
attention map is never stored) to the generator and / or the critic - on the 32x32 map of the 64-pixel networks, the 16x16 map
of the 32-pixel ones.  The block is first order: ``'d'`` requires ``gradient_penalty=None`` (hinge loss + spectral normalisation
is the recipe it belongs to), ``'g'`` works with every loss and penalty; on ProGAN / StyleGAN any value but None raises when the
learner is built; ``cgan`` (ResNet GAN only; None = off, else ``'projection'``, ``'contra'`` or ``'reacgan'``;
``--cgan=none`` on the command line) with ``num_classes`` >= 2 makes the pair class-conditional (conditional.py): class-conditional
BatchNorm in the generator in every mode and, with ``'projection'``, a projection critic - the SNGAN-projection / SAGAN / BigGAN
way - on HIP kernels of their own; the inputs keep their widths and the learner's steps take the batch's labels
(``DeviceImageLoader(labels=...)`` or any loader that yields ``(x, label)``).  It is independent of ``class_condition`` /
``use_auxiliary_classifier`` (the reference's own conditioning, which never ran and keeps raising), works with every loss, penalty
and augmentation and with ``spectral_norm`` / ``self_attention``; any other value, a progressive model or ``num_classes`` < 2
raises when the learner is built.  ``'contra'`` (ContraGAN's conditional contrastive loss 2C, Kang & Park 2020) and
``'reacgan'`` (ReACGAN's data-to-data cross-entropy D2D-CE, Kang et al. 2021) are classifier-based conditional GANs (AC-GAN's
value ``'acgan'`` is still refused: conditional.py): the critic's score stays unconditional, a head on the critic's feature - an
embedding of width ``cond_embed`` (int E, default 512, in [1, 1024]) with one proxy per class - carries the loss, and both
steps add ``cond_lambda`` (float, default 1.0, finite and >= 0; 0 builds the heads and launches nothing) times it: the critic step
on the real rows, the generator step on the generated rows (csrc/cond_loss.hip; per rank, embeddings are not gathered across
ranks).  ``cond_temperature`` (float, default 1.0, > 0) divides the cosine similarities of the two contrastive losses;
``cond_margin_pos`` / ``cond_margin_neg`` (floats, defaults 0.98 / 0.02, the second below the first) are D2D-CE's margins m_p and
m_n.  The papers train ContraGAN with temperature 1.0 on CIFAR-10 and ReACGAN with 0.5 there and 0.98 / 0.02 margins; these are
the user's choice and nothing was tuned here.  A value outside these ranges raises when the learner is built and names its field;
ProGAN / StyleGAN have none of the five fields; ``ortho_reg`` / ``ortho_reg_d`` (ResNet GAN only; 0 =
off) are the strengths beta of BigGAN's orthogonal regulariser (Brock et al. 2019, eq. 3; ortho_reg.py) on the generator's / the
critic's Conv2dEx and LinearEx weights: at every generator (critic) update the gradient ``4 beta ((Wm Wm^T) o (1 - I)) Wm`` of
``beta |(Wm Wm^T) o (1 - I)|_F^2`` is added to the parameter gradients by batched fp32 matrix-core kernels, after the all-reduce
and before the optimiser step; normalisation affines, the class tables, biases and attention's ``gamma`` are exempt.  BigGAN
trains with 1e-4 on the generator and 0 on the critic (BigGAN-PyTorch's ``ortho()`` applies half this gradient for the same
number); a negative or non-finite value raises when the learner is built, and ProGAN / StyleGAN have no such field;
``hier_latent`` (bool) / ``shared_embed`` (int E; ResNet GAN only, both off by default) are BigGAN's generator conditioning
(Brock et al. 2019; hier_latent.py): with ``hier_latent`` the latent is split over the first linear and the residual blocks
(``chunk = len_latent // (B + 1)``, B = 3 at 32 pixels, 4 at 64; the first linear reads the first ``len_latent - B * chunk``
entries, so 128 is 28 + 4 x 25 at 64 pixels), with ``shared_embed`` = E > 0 (needs a ``cgan`` mode; BigGAN uses 128) the
class is embedded once into ``shared.weight`` (num_classes, E); both norms of every block then take their gain and bias from
bias-free linears of ``[z_b, e(y)]`` (without labels: self-modulation, Chen et al. 2019), computed for the whole network in one
launch, and the (num_classes, C) tables are gone.  ``len_latent < B + 1``, a negative value, ``shared_embed`` without ``cgan`` or
a progressive model raises when the learner is built, and ProGAN / StyleGAN have no such field;
for the ResNet GAN, ``use_ewma_gen`` (bool, default False there; the progressive models' own field of this name is untouched) /
``ewma_decay`` (0.9999; in [0, 1)) / ``ewma_start`` (0; >= 0) keep BigGAN's averaged generator (sampling.py): a copy of the
generator whose parameters and BatchNorm buffers follow ``avg = d avg + (1 - d) live`` after every generator update, in two
launches, with ``d = 0`` (a plain copy) while fewer than ``ewma_start`` updates have happened and ``d = ewma_decay`` afterwards;
``truncation`` (None = off, else > 0) is the default threshold of ``learner.generate()``'s truncation trick - latents from the
standard normal truncated to [-t, t] by inverse CDF on the project's Philox stream - and ``standing_stat_batches`` (16; >= 1)
the default number of batches over which ``generate(standing_stats=True)`` re-estimates every BatchNorm's statistics as a plain
average; a value outside these ranges raises when the learner is built, and ProGAN / StyleGAN have none of the four new fields;
``cr_real`` / ``cr_fake`` / ``cr_latent_d`` / ``cr_latent_g`` (ResNet GAN only; 0 = off) are the weights of consistency
regularisation (consistency.py): bCR (Zhang et al. 2020) adds ``cr_real * msd(D(x), D(T(x))) + cr_fake * msd(D(G(z)), D(T(G(z))))``
to the critic's loss, ``T`` a horizontal flip (``cr_flip``, default True) and a shift by up to ``cr_shift`` pixels per axis with
zero fill (None = ``res_samples // 8``: 4 at 32 pixels, 8 at 64; ``--cr_shift=none`` on the command line), drawn afresh for every
image from the project's Philox stream; zCR (Zhao et al. 2020) adds ``cr_latent_d * msd(D(G(z)), D(G(z')))`` to the critic's loss
and ``- cr_latent_g * imsd(G(z), G(z'))`` to the generator's, ``z' = z + cr_sigma * n`` (``cr_sigma`` 0.03) with a fresh normal
``n``; ``msd`` is the batch mean of squared score differences, ``imsd`` the mean over all elements of squared image differences.
ICR's CIFAR-10 BigGAN setting is 10 / 10 / 5 / 0.5.  The terms are first order in the critic and compose with every loss and
penalty, ``spectral_norm``, ``self_attention`` and ``cgan``; with all four weights at 0 nothing is built, drawn or launched.  A
negative or non-finite weight, ``cr_sigma <= 0`` with a latent weight on, ``cr_shift`` outside [0, res_samples), or a positive
weight together with ``diffaugment`` / ``ada`` raises when the learner is built, and ProGAN / StyleGAN have no such field;
``fq_codes`` (ResNet GAN only; int K, 0 = off, else in [1, 4096]) / ``fq_decay`` (float, default 0.8, in [0, 1)) / ``fq_commit``
(float, default 1.0, finite and >= 0) are the fields of FQ-GAN's feature quantisation of the critic (Zhao et al. 2020;
quantize.py): K dictionary rows that replace every spatial feature vector of one critic layer by the nearest of them, the decay of
the moving averages the dictionary follows the features with, and the weight of the commitment term in the critic's loss.  The
layer is first order, so ``fq_codes > 0`` excludes every ``gradient_penalty`` (hinge loss + spectral normalisation is the recipe).
FQ-BigGAN uses 2^10 codes, decay 0.8 and weight 1.0; these are the user's choice and nothing was tuned here.  A value outside these
ranges, or a gradient penalty beside ``fq_codes > 0``, raises ValueError when the learner is built and names its field.  The layer's
kernels are not in the package yet: a valid ``fq_codes > 0`` is still refused (NotImplementedError, as ``cgan='acgan'`` is) and 0
builds nothing; ProGAN / StyleGAN have none of the three fields.
``'ppl'`` as an entry of ``gen_metrics`` (ProGAN and StyleGAN): the perceptual path length of ppl.py - the StyleGAN paper's measure
of how smooth the latent space is - of the generator the other metrics score: the mean squared image change per squared latent step
along interpolation paths between ``ppl_samples`` (default 1024, >= 2) pairs of latents, after the distances outside the 1st .. 99th
percentile are dropped.  ``ppl_space`` (``--ppl_space=none`` on the command line) is ``'z'`` (spherical paths between latents),
``'w'`` (straight paths in StyleGAN's W; refused on ProGAN, which has none) or None: ``'w'`` for StyleGAN, ``'z'`` for ProGAN.
``ppl_sampling`` is ``'full'`` (the step is taken at a uniformly drawn point of the path) or ``'end'`` (at its start);
``ppl_epsilon`` (default 1e-4, finite, in (0, 1)) the step; ``ppl_seed`` (an integer in [0, 2**63)) fixes the latents, the points
and the per-layer noise, so two evaluations of one generator agree bit for bit.  The image distance is ``ops.pyramid_mse`` over
every level the resolution allows, not LPIPS (no pretrained network ships here): compare a run with itself, not with published
numbers.  The metric needs no validation reals and is not available while a resolution fades in (its line then says so).  A
value outside these ranges, or ``'ppl'`` among ``disc_metrics``, raises ValueError when the learner is built and names its field;
the ResNet GAN has none of the five fields.
``optimizer`` (all three models) is ``'adam'`` (the default, unchanged), ``'rmsprop'``, ``'momentum'``, ``'sgd'`` or ``'oadam'``
(optimistic Adam, Daskalakis et al. 2018); each is a fused arena optimiser of optim.py, one launch per update, and works with the
LR schedules, step graphs and checkpoints like Adam.  The mapping of fields: ``lr_base``, ``eps`` and ``wd`` are shared by all;
``'adam'`` and ``'oadam'`` read ``beta1`` / ``beta2``; ``'rmsprop'`` reads alpha = ``beta2`` (torch.optim.RMSprop's smoothing
constant; ``beta1`` is unused) and its momentum from ``rmsprop_momentum`` (float, default 0.0, in [0, 1)) alone; ``'momentum'`` is
SGD with the coefficient ``momentum`` (float, default 0.9, in [0, 1), and > 0 for this optimiser); ``'sgd'`` is plain SGD and reads
neither.  ``beta2``'s default differs by model (0.99 for ProGAN / StyleGAN, 0.9 for the ResNet GAN), so RMSprop's alpha does too;
these are the user's choice and nothing was tuned here.  A value outside these ranges raises ValueError when the learner is built and
names its field; a checkpoint saved under one optimiser does not load under another, ``reference_format=True`` needs ``'adam'``,
and files saved under ``'adam'`` do not carry the two new fields.
``spectrum_reg`` (ProGAN and StyleGAN; float, 0 = off, finite and >= 0) adds the power-spectrum regulariser of spectrum_reg.py
(Durall et al. 2020) to the generator's loss: ``spectrum_reg`` times the mean over a band of radii of the squared difference of the
natural logarithms of the generated batch's radial power spectrum and a target profile, which the critic step keeps as a moving
average over the real batches with ``spectrum_reg_decay`` (float, default 0.99, in [0, 1); the first batch copies).
``spectrum_reg_band`` is ``'hf'`` (the default: radii R/4+1 .. R/2, where up-convolution artifacts live) or ``'all'`` (1 .. R/2), the
'spectrum' metric's own two bands, and the window is that metric's ``spectrum_window``.  The term is computed on the un-augmented
images, per rank, from 16x16 on (the 4x4 and 8x8 phases launch nothing); the target restarts at a growth event and travels in
checkpoints only while the option is on; with the option on the learner steps eagerly (no step graphs).  The paper's weight depends
on its loss normalisation; these are the user's choice and nothing was tuned here.  A negative or non-finite weight, another band or
a decay outside [0, 1) raises ValueError when the learner is built and names its field; the ResNet GAN has none of the three fields.
``--gradient_penalty=none`` on the command line means no penalty (None), as ``make_config(gradient_penalty=None)`` does.
"""
import argparse
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from ._int import str2bool

BS = 64
NIMG_TRANSITION = 600000
_HERE = os.path.abspath(os.path.dirname(__file__))
_MODELS = {'resnetgan': 'ResNet GAN', 'resnet gan': 'ResNet GAN', 'progan': 'ProGAN', 'stylegan': 'StyleGAN'}


def _float_or_none(v):
    """CLI type of an optional float: 'none' (any case) -> None."""
    return None if v is None or str(v).casefold() == 'none' else float(v)


def _int_or_none(v):
    """CLI type of an optional integer: 'none' (any case) -> None."""
    return None if v is None or str(v).casefold() == 'none' else int(v)


def _str_or_none(v):
    """CLI type of an optional name: 'none' (any case) -> None, else casefolded."""
    return None if v is None or str(v).casefold() == 'none' else str(v).casefold()


def _spec(model_type):
    """(name, type, default[, choices]) rows; booleans use str2bool like the reference."""
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    rows = [
        ('dev', str.casefold, dev), ('n_gpu', int, 1), ('enable_cudnn_autotuner', bool, False),
        ('random_seed', int, -1), ('gen_bs_mult', int, 1), ('num_gen_iters', int, 1),
        ('loss', str.casefold, 'wgan'), ('gradient_penalty', _str_or_none, 'wgan-gp'), ('lda', float, 10.),
        ('gamma', float, 1.), ('lr_sched_custom', str.casefold, None), ('optimizer', str.casefold, 'adam'),
        ('beta1', float, 0.), ('eps', float, 1.e-8), ('wd', float, 0.), ('align_corners', bool, False),
        ('model_upsample_type', str.casefold, 'nearest'), ('model_downsample_type', str.casefold, 'average'),
        ('latent_distribution', str.casefold, 'normal'), ('num_classes', int, 0), ('class_condition', bool, False),
        ('use_auxiliary_classifier', bool, False), ('ac_disc_scale', float, 1.), ('ac_gen_scale', float, .1),
        ('num_iters_valid', int, 1000), ('metrics_dev', str.casefold, 'cpu'),
        ('gen_metrics', list, ['generator loss', 'fake realness', 'image grid']),
        ('disc_metrics', list, ['discriminator loss', 'fake realness', 'real realness']),
        ('img_grid_sz', int, 4), ('img_grid_show_labels', bool, True),
        ('save_samples_dir', Path, Path(_HERE + '/samples/')), ('num_iters_save_model', int, 1000),
        ('save_model_dir', Path, Path(_HERE + '/models/')), ('num_workers', int, 0),
        ('pin_memory', bool, dev == 'cuda'), ('log_every', int, 50), ('compute_dtype', str.casefold, 'f32'),
        ('diffaugment', str, None),
        ('ada', str, None), ('ada_p', float, 0.0), ('ada_target', _float_or_none, 0.6), ('ada_interval', int, 4),
        ('ada_kimg', float, 500.0),
        ('swd_nhoods', int, 128), ('swd_dir_repeats', int, 4), ('swd_dirs_per_repeat', int, 128), ('swd_seed', int, 0),
        ('msssim_range', float, 2.0), ('spectrum_window', str.casefold, 'hann'),
        ('prdc_k', int, 5), ('prdc_res', int, 32),
        ('fd_res', int, 16), ('kid_res', int, 32), ('kid_block', int, 1000),
        ('self_attention', _str_or_none, None), ('cgan', _str_or_none, None),
        ('momentum', float, 0.9), ('rmsprop_momentum', float, 0.0),
    ]
    if model_type == 'ResNet GAN':
        rows += [('batch_size', int, BS), ('num_main_iters', int, 300000), ('num_disc_iters', int, 5),
                 ('lr_base', float, .0001), ('lr_sched', str.casefold, None), ('beta2', float, .9),
                 ('res_samples', int, 64), ('res_dataset', int, 64), ('blur_type', str.casefold, None),
                 ('eps_drift', float, 0.), ('len_latent', int, 128), ('nonlinearity', str.casefold, 'relu'),
                 ('leakiness', float, .01), ('use_equalized_lr', bool, False), ('spectral_norm', bool, False),
                 ('ortho_reg', float, 0.), ('ortho_reg_d', float, 0.), ('hier_latent', bool, False), ('shared_embed', int, 0),
                 ('use_ewma_gen', bool, False), ('ewma_decay', float, 0.9999), ('ewma_start', int, 0),
                 ('truncation', _float_or_none, None), ('standing_stat_batches', int, 16),
                 ('cr_real', float, 0.), ('cr_fake', float, 0.), ('cr_latent_d', float, 0.), ('cr_latent_g', float, 0.),
                 ('cr_sigma', float, 0.03), ('cr_shift', _int_or_none, None), ('cr_flip', bool, True),
                 ('cond_lambda', float, 1.0), ('cond_embed', int, 512), ('cond_temperature', float, 1.0),
                 ('cond_margin_pos', float, 0.98), ('cond_margin_neg', float, 0.02),
                 ('fq_codes', int, 0), ('fq_decay', float, 0.8), ('fq_commit', float, 1.0)]
    else:
        rows += [('batch_size', int, BS),
                 ('bs_dict', dict, {4: BS, 8: BS, 16: BS, 32: BS, 64: BS, 128: BS, 256: BS, 512: BS // 2,
                                    1024: BS // 4}),
                 ('num_disc_iters', int, 1), ('nimg_transition', int, NIMG_TRANSITION), ('lr_base', float, .001),
                 ('lr_sched', str.casefold, 'resolution dependent'), ('beta2', float, .99),
                 ('res_samples', int, 1024), ('res_dataset', int, 1024), ('blur_type', str.casefold, 'binomial'),
                 ('bit_exact_resampling', bool, False), ('eps_drift', float, .001), ('len_latent', int, 512),
                 ('nonlinearity', str.casefold, 'leaky relu'), ('leakiness', float, .2),
                 ('use_equalized_lr', bool, True), ('normalize_z', bool, True), ('mbstd_group_size', int, 4),
                 ('use_ewma_gen', bool, True),
                 ('ppl_samples', int, 1024), ('ppl_space', _str_or_none, None), ('ppl_sampling', str.casefold, 'full'),
                 ('ppl_epsilon', float, 1e-4), ('ppl_seed', int, 0),
                 ('spectrum_reg', float, 0.), ('spectrum_reg_band', str.casefold, 'hf'), ('spectrum_reg_decay', float, 0.99)]
        if model_type == 'ProGAN':
            rows += [('num_main_iters', int, (NIMG_TRANSITION // BS) * 20),
                     ('lr_fctr_dict', dict, {4: 1., 8: 1., 16: 1., 32: 1., 64: 1., 128: 1., 256: 1., 512: 1.,
                                             1024: 1.5}),
                     ('init_res', int, 4), ('use_pixelnorm', bool, True)]
        else:
            rows += [('num_main_iters', int, (NIMG_TRANSITION // BS) * 18),
                     ('lr_fctr_dict', dict, {4: 1., 8: 1., 16: 1., 32: 1., 64: 1., 128: 1.5, 256: 2., 512: 3.,
                                             1024: 3.}),
                     ('init_res', int, 8), ('len_dlatent', int, 512), ('mapping_num_fcs', int, 8),
                     ('mapping_lrmul', float, .01), ('use_noise', bool, True), ('use_pixelnorm', bool, False),
                     ('use_instancenorm', bool, True), ('pct_mixing_reg', float, .9),
                     ('beta_trunc_trick', float, .995), ('psi_trunc_trick', float, .7),
                     ('cutoff_trunc_trick', int, 4)]
    return rows


def _model_type(name):
    key = name.casefold().replace('-', '').replace('_', '')
    if key not in _MODELS:
        raise ValueError("Invalid model inputted. Currently supported models: resnetgan, progan, stylegan")
    return _MODELS[key]


def _postprocess(config, model_type, seed=True):
    """config.py:337-376."""
    config.dev = torch.device(config.dev)
    if config.pin_memory and config.dev != torch.device('cuda'):
        raise ValueError('--pin_memory should be set to `False` if not using CUDA.')
    if seed:
        if config.random_seed == -1:
            np.random.seed(None)
            torch.seed()
        elif 0 <= config.random_seed < 2 ** 32:
            np.random.seed(config.random_seed)
            torch.manual_seed(config.random_seed)
        else:
            raise ValueError("--random_seed must either be -1 for random seeding or be in the range [0,2**32) to "
                             "accommodate numpy's and torch's seeding specifications.")
    if model_type in ('ProGAN', 'StyleGAN',):
        _bs = config.batch_size
        config.bs_dict = {4: _bs, 8: _bs, 16: _bs, 32: _bs, 64: _bs, 128: _bs, 256: _bs, 512: _bs // 2,
                          1024: _bs // 4}
        if config.mbstd_group_size < -1 or not config.mbstd_group_size:
            raise ValueError("--mbstd_group_size must either be -1 to indicate not applying minibatch standard "
                             "deviation or a positive integer indicating the group size for the minibatch standard "
                             "deviation layer.")
    config.model = model_type
    return config


def make_config(model, seed=False, **overrides):
    """Namespace with the reference defaults for `model` ('stylegan' | 'progan'), then `overrides`,
    then the reference post-processing.  ``bs_dict`` may be overridden explicitly AFTER the rebuild
    (the reference only allows that through ``learner.config.bs_dict``)."""
    mt = _model_type(model)
    ns = argparse.Namespace(**{name: default for name, _, default in _spec(mt)})
    bs_dict = overrides.pop('bs_dict', None)
    for k, v in overrides.items():
        if not hasattr(ns, k):
            raise AttributeError(f'unknown config field {k!r} for {mt}')
        setattr(ns, k, v)
    ns = _postprocess(ns, mt, seed=seed)
    if bs_dict is not None:
        ns.bs_dict = dict(bs_dict)
    return ns


def main(argv=None):
    top = argparse.ArgumentParser(description='Configure a GAN model (gan-lab compatible).')
    top.add_argument('model', type=str)
    first, rest = top.parse_known_args(argv)
    mt = _model_type(first.model)
    parser = argparse.ArgumentParser()
    parser.add_argument('model', type=str)
    for name, typ, default in _spec(mt):
        if typ is bool:
            parser.add_argument('--' + name, type=str2bool, nargs='?', const=True, default=default)
        elif typ in (list, dict):
            parser.add_argument('--' + name, type=typ, default=default)
        else:
            parser.add_argument('--' + name, type=typ, default=default)
    config = parser.parse_args(argv)
    config = _postprocess(config, mt, seed=True)
    config.save_samples_dir.mkdir(parents=True, exist_ok=True)
    config.save_model_dir.mkdir(parents=True, exist_ok=True)
    with open(str(Path.home() / '.configs_dir.txt'), 'wb') as f:
        f.write(_HERE.encode())
    with open(_HERE + '/.config.p', 'wb') as f:
        pickle.dump(config, f, protocol=3)
    return config


if __name__ == '__main__':
    main()
