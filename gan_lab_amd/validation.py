"""The set metrics of the learners' validation ('swd', 'msssim', 'spectrum', 'prdc', 'fd', 'kid', 'ppl' in config.gen_metrics):
ONE ordered table, ``SCORERS``, and per metric a scorer - the learner's side of the metric module.

A scorer class says what the metric refuses (``refuse``); an instance is one evaluation at one resolution: the constructor decides how
many generated and real images it still wants (``fake_left`` / ``real_left``; 0 where the resolution has no result) and builds or
reuses the evaluation objects, ``feed`` takes one batch, ``finish`` returns ``(dict for last_metrics, [(line name, value)])``.
``compute_metrics`` of both learners is the loop over the scorers: the learner owns the images (which generator, the fade-in of
the reals, the process stream), the scorer everything that differs between metrics.  Adding a metric: one scorer, one table row.
"""
from . import frechet, kid, msssim, ppl, prdc, spectrum, swd
from ._metric_common import wanted


class Scorer(object):
    name = module = None        # the entry of config.gen_metrics (its config fields are '<name>_*') and the metric's module
    about = 'it compares the generated validation images with the validation reals'
    reals = 'required'          # 'required': refuses valid_dl=None; 'optional': scores the reals when given; None: reads none
    progressive_only = False    # options checked when a progressive learner is built, not by every learner

    @classmethod
    def refuse(cls, learner, metrics_type, valid_dl):
        if metrics_type != 'generator':
            raise ValueError(f"'{cls.name}' is a generator metric: {cls.about} and cannot be listed among the critic's metrics "
                             f"(config.disc_metrics)")
        if cls.reals == 'required' and valid_dl is None:
            raise ValueError(f"'{cls.name}' needs the validation reals: pass valid_dl (train(train_dl, valid_dl, z_valid_dl))")

    def __init__(self, learner, res):
        self.learner, self.res = learner, res
        self.fake_left = self.real_left = 0

    def _whole_batches(self, n_z, valid_dl):
        """Images per set: min(latents, reals) truncated to whole batches, so that both sets hold the same count."""
        bs = self.learner.batch_size
        n_use = min(n_z, len(valid_dl.dataset)) // bs * bs
        if n_use < 1:
            raise ValueError(f"'{self.name}' needs at least one whole batch of {bs} validation latents and reals (got "
                             f"{n_z} and {len(valid_dl.dataset)})")
        return n_use

    def _evaluations(self, make, *kwargs):
        """``make(**kw)`` for each of ``kwargs``, reset: the learner keeps them (``_metric_evals[name]``) across validation points
        for as long as the constructor arguments stay what they are."""
        cache = self.learner._metric_evals
        if cache.get(self.name, (None,))[0] != kwargs:
            cache[self.name] = (kwargs, tuple(make(**kw) for kw in kwargs))
        for ev in cache[self.name][1]:
            ev.reset()
        return cache[self.name][1]

    def wants_fake(self, k):
        """Does a batch of ``k`` generated images go in?  ``wants_real``: of ``k`` reals."""
        return self.fake_left > 0

    def wants_real(self, k):
        return self.real_left > 0

    def feed(self, k, fake, real):
        if self.wants_fake(k):
            self.feed_fake(fake)
            self.fake_left -= k
        if self.wants_real(k):
            self.feed_real(real)
            self.real_left -= k

    def _nan_line(self, why):
        return [(self.name, f'nan ({why}; the current resolution is {self.res}x{self.res})')]


class Swd(Scorer):
    name, module = 'swd', swd

    def __init__(self, learner, res, n_z, valid_dl):
        super().__init__(learner, res)
        self.ev = None
        if res < swd.MIN_RES:            # the pyramid has no level
            return
        c, n = learner.config, self._whole_batches(n_z, valid_dl)
        self.ev, = self._evaluations(swd.SlicedWasserstein, dict(
            res=res, n_images=n, nhoods_per_image=c.swd_nhoods, dir_repeats=c.swd_dir_repeats,
            dirs_per_repeat=c.swd_dirs_per_repeat, seed=c.swd_seed, device=c.dev))
        self.fake_left = self.real_left = n

    def feed_fake(self, x):
        self.ev.feed_fake(x)

    def feed_real(self, x):
        self.ev.feed_real(x)

    def finish(self):
        if self.ev is None:
            return {'levels': [], 'swd': [], 'mean': float('nan')}, \
                self._nan_line(f'the pyramid starts at {swd.MIN_RES}x{swd.MIN_RES}')
        out = self.ev.result()
        return out, [(f'swd {r}x{r}', v) for r, v in zip(out['levels'], out['swd'])] + [('swd mean', out['mean'])]


class Msssim(Scorer):
    """The fakes are counted over the latents alone and the reals are optional; whole batches only (a batch is an even number of
    images, so pairs never straddle batches): a partial batch is skipped, where the other metrics refuse it."""
    name, module = 'msssim', msssim
    about = 'it compares generated validation images with each other'
    reals = 'optional'

    @classmethod
    def refuse(cls, learner, metrics_type, valid_dl):
        super().refuse(learner, metrics_type, valid_dl)
        if learner.batch_size % 2:
            raise ValueError(f"'msssim' scores adjacent pairs of a validation minibatch: config.batch_size must be even at "
                             f"this resolution, got {learner.batch_size}")

    def __init__(self, learner, res, n_z, valid_dl):
        super().__init__(learner, res)
        self.ev_fake = self.ev_real = None
        if res < msssim.MIN_RES:         # there is no fifth level
            return
        c, bs = learner.config, learner.batch_size
        n_fake = n_z // bs * bs
        if n_fake < 1:
            raise ValueError(f"'msssim' needs at least one whole batch of {bs} validation latents (got {n_z})")
        n_real = min(n_z, len(valid_dl.dataset)) // bs * bs if valid_dl is not None else 0
        evs = self._evaluations(msssim.MultiScaleSSIM, *(dict(res=res, n_images=n, data_range=c.msssim_range, device=c.dev)
                                                         for n in (n_fake, n_real) if n))
        self.ev_fake, self.ev_real = evs if n_real else (evs[0], None)
        self.fake_left, self.real_left = n_fake, n_real

    def wants_fake(self, k):
        return self.fake_left > 0 and k == self.learner.batch_size

    def wants_real(self, k):
        return self.real_left > 0 and k == self.learner.batch_size

    def feed_fake(self, x):
        self.ev_fake.feed(x)

    def feed_real(self, x):
        self.ev_real.feed(x)

    def finish(self):
        """'msssim real' scores the faded-in validation reals: the number to compare 'msssim fake' against."""
        if self.ev_fake is None:
            return {'msssim': float('nan'), 'pairs': 0, 'per_level': [[], float('nan')]}, \
                self._nan_line(f'five levels need {msssim.MIN_RES}x{msssim.MIN_RES}')
        out = self.ev_fake.result()
        lines = [('msssim fake', out['msssim'])]
        if self.ev_real is not None:
            out['real'] = self.ev_real.result()
            lines.append(('msssim real', out['real']['msssim']))
        return out, lines


class Spectrum(Scorer):
    name, module = 'spectrum', spectrum

    def __init__(self, learner, res, n_z, valid_dl):
        super().__init__(learner, res)
        self.ev_fake = self.ev_real = None
        if res < spectrum.MIN_RES or res > spectrum.MAX_RES:         # the kernels have no transform
            return
        c, n = learner.config, self._whole_batches(n_z, valid_dl)
        kw = dict(res=res, n_images=n, window=c.spectrum_window, device=c.dev)
        self.ev_fake, self.ev_real = self._evaluations(spectrum.PowerSpectrum, kw, kw)
        self.fake_left = self.real_left = n

    def feed_fake(self, x):
        self.ev_fake.feed(x)

    def feed_real(self, x):
        self.ev_real.feed(x)

    def finish(self):
        """The dict holds both profiles in dB, for plotting, and the two distances."""
        if self.ev_fake is None:
            nan = float('nan')
            return {'spectrum': nan, 'hf': nan, 'fake_db': [], 'real_db': [], 'images': 0}, \
                self._nan_line(f'the transform covers {spectrum.MIN_RES}x{spectrum.MIN_RES} to '
                               f'{spectrum.MAX_RES}x{spectrum.MAX_RES}')
        out = spectrum.distance(self.ev_fake, self.ev_real)
        return out, [('spectrum', out['spectrum']), ('spectrum hf', out['hf'])]


class _Rows(Scorer):
    """'prdc', 'fd' and 'kid' score rows: the images reduced by 2x2 means to at most ``config.<name>_res`` pixels (prdc.features).
    ``evaluation(config, dim, n)``: the class and its constructor arguments; ``lines``: the keys of the result that are reported."""

    def __init__(self, learner, res, n_z, valid_dl):
        super().__init__(learner, res)
        c, n = learner.config, self._whole_batches(n_z, valid_dl)
        self.rows_res = getattr(c, self.name + '_res')
        self.ev, = self._evaluations(*self.evaluation(c, prdc.feature_dim(3, res, self.rows_res), n))
        self.fake_left = self.real_left = n

    def feed_fake(self, x):
        self.ev.feed_fake(prdc.features(x, self.rows_res))

    def feed_real(self, x):
        self.ev.feed_real(prdc.features(x, self.rows_res))

    def finish(self):
        out = self.ev.result()
        return out, [(key, out[key]) for key in self.lines]


class Prdc(_Rows):
    name, module, lines = 'prdc', prdc, ('precision', 'recall', 'density', 'coverage')

    def evaluation(self, c, dim, n):
        return prdc.PRDC, dict(dim=dim, n_real=n, n_fake=n, k=c.prdc_k, device=c.dev)


class Fd(_Rows):
    name, module, lines = 'fd', frechet, ('fd',)

    def evaluation(self, c, dim, n):
        return frechet.Frechet, dict(dim=dim, device=c.dev)


class Kid(_Rows):
    name, module, lines = 'kid', kid, ('kid',)

    def evaluation(self, c, dim, n):
        return kid.KID, dict(dim=dim, n_real=n, n_fake=n, block=c.kid_block, device=c.dev)


class Ppl(Scorer):
    """The degenerate case: no batch goes in, ``finish`` does the work - ``ppl.generator_path_length`` of the generator the learner
    scores (the time-averaged one when ``use_ewma_gen`` is on) over ``config.ppl_samples`` pairs in batches of the current batch
    size.  It needs no validation data and leaves the training stream where it was."""
    name, module = 'ppl', ppl
    about = "it measures the generator's latent space"
    reals = None
    progressive_only = True

    def __init__(self, learner, res, n_z, valid_dl):
        super().__init__(learner, res)

    def finish(self):
        L = self.learner
        samples, space, sampling, epsilon, seed = ppl.validate_config(L.config)
        if L.gen_model.fade_in_phase:
            return {'ppl': float('nan'), 'space': space}, \
                [('ppl', 'nan (not available while a resolution fades in: the image then blends two resolutions)')]
        out = ppl.generator_path_length(L, samples, space, sampling=sampling, epsilon=epsilon, batch=L.batch_size, seed=seed)
        out['space'] = space
        return out, [('ppl', out['ppl'])]


# THE table.  Its order is the order of the refusals, of the constructions and of the report ...
SCORERS = (Swd, Msssim, Spectrum, Prdc, Fd, Kid, Ppl)
# ... and every batch is fed in the same order but for 'msssim', which goes last
FEED_ORDER = tuple(s for s in SCORERS if s is not Msssim) + (Msssim,)
NAMES = tuple(s.name for s in SCORERS)
ROW_SCORERS = tuple(s for s in SCORERS if issubclass(s, _Rows))           # what the ResNet GAN learner computes


def uses_reals(metrics):
    """Does any metric listed in ``metrics`` read the validation reals (``valid_dl``)?"""
    return any(s.reals and wanted(metrics, s.name) for s in SCORERS)


def in_feed_order(scorers):
    return sorted(scorers, key=lambda s: FEED_ORDER.index(type(s)))
