"""CPU tests of the fused arena optimisers beside Adam.  tests/optim_reference.py - what tests/test_gpu_optim.py holds the kernels
to - is tied to ``torch.optim.RMSprop`` / ``torch.optim.SGD`` in float64 and, for optimistic Adam, to a literal transcription of
the paper's algorithm; the wrong forms a kernel could silently be are shown to leave the fp32 error bound; and the configuration
surface: the fields, the command line, every refusal by field name, checkpoints' config under Adam, the optimiser-mismatch
refusal on load, and a learner built with every ``optimizer`` value."""
import numpy as np
import pytest
import torch

import optim_reference as ref
from pointwise_reference import adam_run

OPTIMIZERS = ('adam', 'rmsprop', 'momentum', 'sgd', 'oadam')
COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)


# ---- the restatements against torch.optim ----------------------------------------------------------------------------------------
def _torch_params(n=23):
    """Three parameters: an ordinary one, one whose gradient is zero in every step, one whose ``grad`` stays None."""
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=torch.float64)) for _ in range(3)]
    grads = [[torch.randn(n, generator=g, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), None] for _ in range(5)]
    return ps, grads


def _drive(opt, ps, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.clone()
        opt.step()


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('momentum', [0.0, 0.9])
def test_rmsprop_reference_equals_torch(momentum, wd):
    ps, grads = _torch_params()
    start = [p.detach().numpy().copy() for p in ps]
    lr, alpha, eps = 1e-2, 0.9, 1e-8
    _drive(torch.optim.RMSprop(ps, lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=momentum), ps, grads)
    for i in range(3):
        p, sq, buf = start[i], np.zeros(23), np.zeros(23)
        for gs in grads:
            if gs[i] is not None:
                p, sq, buf = ref.rmsprop_reference(p, gs[i].numpy(), sq, buf, lr, alpha, eps, wd, momentum)
        err = np.abs(p - ps[i].detach().numpy()).max()
        print(f'param {i}: {err:.3e}')
        assert err <= 1e-13
    assert np.array_equal(start[2], ps[2].detach().numpy())            # grad None: untouched
    assert (np.array_equal(start[1], ps[1].detach().numpy())) == (wd == 0.0)      # zero gradient: only weight decay moves it


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('momentum', [0.0, 0.9])
def test_sgd_reference_equals_torch(momentum, wd):
    ps, grads = _torch_params()
    start = [p.detach().numpy().copy() for p in ps]
    lr = 1e-2
    _drive(torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=wd, dampening=0, nesterov=False), ps, grads)
    for i in range(3):
        p, buf, first = start[i], np.zeros(23), True
        for gs in grads:
            if gs[i] is not None:
                p, buf = ref.sgd_reference(p, gs[i].numpy(), buf, lr, wd, momentum, first)
                first = False
        err = np.abs(p - ps[i].detach().numpy()).max()
        print(f'param {i}: {err:.3e}')
        assert err <= 1e-13
    assert np.array_equal(start[2], ps[2].detach().numpy())


def test_optimistic_adam_equals_the_papers_algorithm_and_starts_with_twice_adams_step():
    """Daskalakis et al. 2018, Algorithm 1, transcribed: theta_t = theta_{t-1} - 2 eta mhat_t / (sqrt(vhat_t) + eps)
    + eta mhat_{t-1} / (sqrt(vhat_{t-1}) + eps), mhat = m / (1 - b1^t), vhat = v / (1 - b2^t), with the term of t - 1 zero at t = 1."""
    p0, grads = ref.inputs(1000, steps=5)
    lr, b1, b2, eps = 1e-3, 0.5, 0.99, 1e-8
    theta, m, v, last = p0.astype(np.float64), np.zeros(1000), np.zeros(1000), np.zeros(1000)
    p, mm, vv, prev = p0.astype(np.float64), np.zeros(1000), np.zeros(1000), np.zeros(1000)
    for t, g in enumerate(grads, 1):
        g = g.astype(np.float64)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g ** 2
        mhat, vhat = m / (1 - b1 ** t), v / (1 - b2 ** t)
        now = mhat / (np.sqrt(vhat) + eps)
        theta = theta - 2 * lr * now + lr * last
        last = now
        p, mm, vv, prev = ref.oadam_reference(p, g, mm, vv, prev, lr, b1, b2, eps, 0.0, 1 - b1 ** t, 1 - b2 ** t)
        assert np.abs(p - theta).max() <= 1e-13 * max(np.abs(theta).max(), 1.0), t
    out, _, _ = ref.run('oadam', p0, grads[:1], lr=lr, b1=b1, b2=b2, eps=eps, wd=0.0)
    adam_p, _, _, _ = adam_run(p0, grads[:1], lr, b1, b2, eps, 0.0)
    step_o, step_a = out['p'] - p0, adam_p - p0
    assert np.abs(step_o - 2 * step_a).max() <= 1e-12 * np.abs(step_a).max() and np.abs(step_a).max() > 1e-4


# ---- wrong forms leave the bound -------------------------------------------------------------------------------------------------
WRONG = [('rmsprop', 'eps_inside', dict(lr=1e-3, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0)),
         ('rmsprop', 'eps_inside', dict(lr=1e-3, alpha=0.9, eps=1e-8, wd=1e-2, momentum=0.9)),
         ('sgd', 'dampening', dict(lr=1e-3, wd=0.0, momentum=0.9)),
         ('sgd', 'first_ignored', dict(lr=1e-3, wd=1e-2, momentum=0.9)),
         ('oadam', 'prev_first', dict(lr=1e-3, b1=0.0, b2=0.99, eps=1e-8, wd=0.0)),
         ('oadam', 'prev_first', dict(lr=1e-3, b1=0.5, b2=0.999, eps=1e-8, wd=1e-2))]


@pytest.mark.parametrize('kind,variant,hp', WRONG, ids=[f'{k}-{v}-{i}' for i, (k, v, _) in enumerate(WRONG)])
def test_wrong_variants_leave_the_bound(kind, variant, hp):
    """eps inside the root, dampening applied, ``first`` ignored (a stale buffer is updated instead of replaced: the GPU test
    starts SGD from such a buffer too) and prev updated before use, at the GPU test's inputs: each leaves the right recurrence's
    fp32 error bound after 5 steps by more than a factor 10 somewhere in p or the state."""
    for n in (1023, 4100):
        p0, grads = ref.inputs(n, steps=5)
        state = dict(buf=np.random.default_rng(n).standard_normal(n).astype(np.float32)) if kind == 'sgd' else None
        good, err, _ = ref.run(kind, p0, grads, state=state, **hp)
        bad, _, _ = ref.run(kind, p0, grads, variant=variant, state=state, **hp)
        worst = max((np.abs(bad[k] - good[k]) / np.maximum(err[k], 1e-300)).max() for k in good
                    if not (kind == 'rmsprop' and k == 'buf' and hp['momentum'] == 0))
        print(f'{kind} {variant} n={n}: up to {worst:.3g} x the bound')
        assert worst > 10


def test_bounds_are_a_few_ulps_per_step():
    """The bounds the GPU test uses are not vacuous: after 8 steps the median bound on p is below 40 ulps of max(|p|, lr)."""
    for kind, hp in (('rmsprop', WRONG[0][2]), ('rmsprop', WRONG[1][2]), ('sgd', WRONG[2][2]), ('oadam', WRONG[5][2])):
        p0, grads = ref.inputs(4100)
        out, err, local = ref.run(kind, p0, grads, **hp)
        rel = err['p'] / np.maximum(np.abs(out['p']), 1e-3) / ref.U
        print(f'{kind}: bound on p after 8 steps: median {np.median(rel):.1f}, max {rel.max():.1f} ulps of max(|p|, lr)')
        assert np.median(rel) <= 40 and (local['p'] <= err['p']).all()


def test_float32_restatement_stays_inside_the_bound():
    """The CPU's fp32 evaluation (one rounding per operation) of each formula stays inside the bound derived for fp32."""
    for kind, _, hp in WRONG:
        p0, grads = ref.inputs(1023)
        want, err, _ = ref.run(kind, p0, grads, **hp)
        got, _, _ = ref.run(kind, p0, grads, dtype=np.float32, **hp)
        for k in want:
            assert got[k].dtype == np.float32
            ratio = (np.abs(got[k].astype(np.float64) - want[k]) / np.maximum(err[k], 1e-300)).max()
            print(f'{kind} {k}: fp32 error / bound {ratio:.3f}')
            assert ratio <= 1.0


# ---- configuration ---------------------------------------------------------------------------------------------------------------
def _config(model='resnetgan', **kw):
    from gan_lab_amd.config import make_config
    base = COMMON if model == 'resnetgan' else dict(dev='cpu', pin_memory=False)
    return make_config(model, **{**base, **kw})


def test_fields_defaults_and_cli(monkeypatch, tmp_path):
    from gan_lab_amd import config
    for model in ('ResNet GAN', 'ProGAN', 'StyleGAN'):
        rows = {row[0]: row[1:] for row in config._spec(model)}
        assert rows['momentum'] == (float, 0.9) and rows['rmsprop_momentum'] == (float, 0.0)
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['stylegan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(args)
    assert (c.optimizer, c.momentum, c.rmsprop_momentum) == ('adam', 0.9, 0.0)
    c = config.main(args + ['--optimizer=RMSprop', '--momentum', '0.5', '--rmsprop_momentum=0.25'])
    assert (c.optimizer, c.momentum, c.rmsprop_momentum) == ('rmsprop', 0.5, 0.25)
    assert 'rmsprop_momentum' in config.__doc__ and 'nothing was tuned here' in config.__doc__


def test_factory_maps_the_fields_and_refuses_by_name():
    from gan_lab_amd import optim
    from gan_lab_amd.utils.backprop_utils import configure_optimizer_for_gan
    w = [torch.nn.Parameter(torch.zeros(3))]
    cfg = _config(optimizer='rmsprop', beta2=0.95, eps=1e-6, wd=0.5, lr_base=0.25, rmsprop_momentum=0.3, momentum=0.7)
    opt = configure_optimizer_for_gan(cfg)(params=w)
    assert type(opt) is optim.FusedRMSprop
    assert opt.defaults == dict(lr=0.25, alpha=0.95, eps=1e-6, weight_decay=0.5, momentum=0.3)     # momentum only via rmsprop_momentum
    opt = configure_optimizer_for_gan(_config(optimizer='momentum', momentum=0.7, lr_base=0.25, wd=0.5))(params=w)
    assert type(opt) is optim.FusedSGD and opt.defaults == dict(lr=0.25, momentum=0.7, weight_decay=0.5)
    opt = configure_optimizer_for_gan(_config(optimizer='sgd', momentum=0.7))(params=w)
    assert type(opt) is optim.FusedSGD and opt.defaults['momentum'] == 0.0
    opt = configure_optimizer_for_gan(_config(optimizer='oadam', beta1=0.5))(params=w)
    assert type(opt) is optim.FusedOptimisticAdam and opt.defaults['betas'] == (0.5, 0.9)
    assert type(configure_optimizer_for_gan(_config())(params=w)) is optim.FusedAdam
    assert type(configure_optimizer_for_gan(_config(), optimizer='SGD')(params=w)) is optim.FusedSGD
    for kw, match in ((dict(momentum=1.0), 'momentum'), (dict(momentum=-0.1), 'momentum'), (dict(momentum='0.9'), 'momentum'),
                      (dict(rmsprop_momentum=1.0), 'rmsprop_momentum'), (dict(rmsprop_momentum=-1e-3), 'rmsprop_momentum'),
                      (dict(rmsprop_momentum=True), 'rmsprop_momentum'), (dict(optimizer='momentum', momentum=0.0), 'momentum'),
                      (dict(optimizer='lion'), "'oadam'")):
        for opt_name in ((kw['optimizer'],) if 'optimizer' in kw else OPTIMIZERS):      # the ranges hold under every optimiser
            with pytest.raises(ValueError, match=match):
                configure_optimizer_for_gan(_config(**{**kw, 'optimizer': opt_name}))
    with pytest.raises(ValueError, match='eps'):
        optim.FusedRMSprop(w, eps=0.0)


def test_checkpoint_config_is_unchanged_under_adam():
    from gan_lab_amd import checkpoint, optim
    for model in ('resnetgan', 'progan', 'stylegan'):
        off = vars(_config(model))
        assert {'momentum', 'rmsprop_momentum'} <= set(off)
        kept = optim.saved_config_fields(dict(off))
        assert kept == {k: v for k, v in off.items() if k not in ('momentum', 'rmsprop_momentum')}
        for name in OPTIMIZERS[1:]:
            on = vars(_config(model, optimizer=name, momentum=0.5))
            assert optim.saved_config_fields(dict(on)) == on
            assert optim.saved_config_fields(dict(off), name) == off          # the learner's own value decides
        assert optim.saved_config_fields(dict(on), 'adam') == {k: v for k, v in on.items() if 'momentum' not in k}
    ref_cfg = checkpoint.reference_config_fields(_config('progan'))
    assert 'momentum' not in ref_cfg and 'rmsprop_momentum' not in ref_cfg and ref_cfg['optimizer'] == 'adam'


def test_state_of_another_optimiser_is_refused():
    from gan_lab_amd import optim
    with pytest.raises(ValueError, match="optimizer='rmsprop'.*optimizer='adam'"):
        optim.check_saved_optimizer('rmsprop', 'adam')
    with pytest.raises(ValueError, match="optimizer='adam'.*optimizer='oadam'"):
        optim.check_saved_optimizer(None, 'oadam')                       # files older than the field were written under Adam
    optim.check_saved_optimizer('RMSprop', 'rmsprop')
    optim.check_saved_optimizer(None, 'adam')
    with pytest.raises(ValueError, match="reference_format=True needs optimizer='adam'.*'sgd'"):
        optim.check_save_format('sgd', True)
    optim.check_save_format('sgd', False)
    optim.check_save_format('adam', True)
    # the optimisers themselves refuse a foreign state record, naming both sides
    w = torch.nn.Parameter(torch.zeros(3))
    w.grad = torch.zeros(3)
    named = [('w', w)]
    rms = optim.FusedRMSprop([w]).export_moments(named)
    assert sorted(rms) == ['momentum_buffer', 'square_avg', 'step']
    assert sorted(optim.FusedSGD([w]).export_moments(named)) == ['momentum_buffer', 'step']
    assert sorted(optim.FusedOptimisticAdam([w]).export_moments(named)) == ['exp_avg', 'exp_avg_sq', 'prev_dir', 'step']
    assert optim.FusedAdam([w]).export_moments(named) == dict(step=0, exp_avg={}, exp_avg_sq={})
    with pytest.raises(ValueError, match="optimizer='adam'.*optimizer='rmsprop'"):
        optim.FusedAdam([w]).import_moments(named, rms)
    with pytest.raises(ValueError, match="optimizer='rmsprop'.*optimizer='adam'"):
        optim.FusedRMSprop([w]).import_moments(named, dict(step=3, exp_avg={}, exp_avg_sq={}))
    assert optim.optimizer_of_state(optim.FusedSGD([w]).export_moments(named)) == 'momentum/sgd'


def test_host_scalars_follow_the_three_float_block():
    """What graphs.GraphedStep uploads per replay: slot 0 = lr for all; (bc1, bc2) for oadam; ``first`` in slot 1 for SGD."""
    from gan_lab_amd import optim
    w = torch.nn.Parameter(torch.zeros(3))
    for opt in (optim.FusedRMSprop([w], lr=0.5), optim.FusedSGD([w], lr=0.5, momentum=0.9),
                optim.FusedOptimisticAdam([w], lr=0.5, betas=(0.5, 0.9))):
        with pytest.raises(RuntimeError, match='before the first eager step'):
            opt.host_scalars()
        opt.state['_fused'] = {id(opt.param_groups[0]): dict(step=0, runs=[], sig=())}
        first, second = opt.host_scalars(), opt.host_scalars()
        assert opt.host_scalars(advance=False) == second and first[0] == second[0] == 0.5
        if opt.NAME == 'rmsprop':
            assert first == second == (0.5, 0.0, 0.0)
        elif opt.NAME == 'sgd':
            assert first == (0.5, 1.0, 0.0) and second == (0.5, 0.0, 0.0)
        else:
            assert first == (0.5, 1 - 0.5, 1 - 0.9) and second == (0.5, 1 - 0.5 ** 2, 1 - 0.9 ** 2)
        two = type(opt)([{'params': [torch.nn.Parameter(torch.zeros(2))]}, {'params': [torch.nn.Parameter(torch.zeros(2))]}])
        two.dev_scalars = 1234
        with pytest.raises(RuntimeError, match='exactly one parameter group'):
            two.step()


# ---- learners --------------------------------------------------------------------------------------------------------------------
def _resnet_learner(monkeypatch, **kw):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = _config(batch_size=4, len_latent=32, log_every=0, **kw)
    cfg.fmap_g = cfg.fmap_d = 16
    return GANLearner(cfg)


def _progressive_learner(monkeypatch, model, **kw):
    from gan_lab_amd import progressive as P
    from gan_lab_amd.progan.learner import ProGANLearner
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    extra = dict(len_dlatent=16, mapping_num_fcs=2, init_res=8, cutoff_trunc_trick=1) if model == 'stylegan' else dict(init_res=4)
    cfg = _config(model, res_samples=16, res_dataset=16, batch_size=4, len_latent=16, **extra, **kw)
    return (StyleGANLearner if model == 'stylegan' else ProGANLearner)(cfg)


@pytest.mark.parametrize('name', OPTIMIZERS)
@pytest.mark.parametrize('model', ['resnetgan', 'progan', 'stylegan'])
def test_learner_constructs_with_every_optimizer(monkeypatch, model, name):
    from gan_lab_amd import optim
    L = _resnet_learner(monkeypatch, optimizer=name) if model == 'resnetgan' else _progressive_learner(monkeypatch, model,
                                                                                                        optimizer=name)
    for opt in (L.opt_gen, L.opt_disc):
        assert type(opt) is optim.OPTIMIZERS[name] and isinstance(opt, torch.optim.Optimizer)
        assert opt.defaults.get('momentum', 0.0) == (0.9 if name == 'momentum' else 0.0)
    assert L.optimizer == name


def test_learner_refuses_bad_fields_and_unknown_optimizers(monkeypatch):
    with pytest.raises(ValueError, match='rmsprop_momentum'):
        _resnet_learner(monkeypatch, optimizer='rmsprop', rmsprop_momentum=1.5)
    with pytest.raises(ValueError, match='momentum'):
        _resnet_learner(monkeypatch, optimizer='momentum', momentum=0.0)
    with pytest.raises(ValueError, match="'oadam'"):
        _progressive_learner(monkeypatch, 'progan', optimizer='adagrad')


def test_checkpoints_name_their_optimizer_and_refuse_another(monkeypatch, tmp_path):
    """A plain-data file saved under RMSprop carries the two fields and loads under RMSprop; under Adam it is refused with both
    names; a file saved under Adam carries neither field; reference_format under RMSprop is refused."""
    from gan_lab_amd import checkpoint
    path_r, path_a = str(tmp_path / 'rms.tar'), str(tmp_path / 'adam.tar')
    L = _resnet_learner(monkeypatch, optimizer='rmsprop', rmsprop_momentum=0.5)
    L.not_trained_yet = False
    L.save_model(path_r)
    ck = checkpoint.load_checkpoint(path_r)
    assert ck['optimizer'] == 'rmsprop' and ck['config']['rmsprop_momentum'] == 0.5 and ck['config']['momentum'] == 0.9
    assert sorted(ck['opt_gen_state_dict']) == ['momentum_buffer', 'square_avg', 'step']
    L.load_model(path_r)
    A = _resnet_learner(monkeypatch)
    with pytest.raises(ValueError, match="optimizer='rmsprop'.*optimizer='adam'"):
        A.load_model(path_r)
    A.not_trained_yet = False
    A.save_model(path_a)
    ck = checkpoint.load_checkpoint(path_a)
    assert ck['optimizer'] == 'adam' and not [k for k in ck['config'] if 'momentum' in k]
    with pytest.raises(ValueError, match="optimizer='adam'.*optimizer='rmsprop'"):
        L.load_model(path_a)
    with pytest.raises(ValueError, match="reference_format=True needs optimizer='adam'"):
        L.save_model(path_r, reference_format=True)
    P = _progressive_learner(monkeypatch, 'progan', optimizer='oadam')
    with pytest.raises(ValueError, match="reference_format=True needs optimizer='adam'"):
        P.save_model(str(tmp_path / 'p.tar'), reference_format=True)
    P.save_model(str(tmp_path / 'p.tar'))
    ck = checkpoint.load_checkpoint(str(tmp_path / 'p.tar'))
    assert ck['optimizer'] == 'oadam' and ck['config']['momentum'] == 0.9 and 'prev_dir' in ck['opt_gen_state_dict']
    with pytest.raises(ValueError, match="optimizer='oadam'.*optimizer='adam'"):
        _progressive_learner(monkeypatch, 'progan').load_model(str(tmp_path / 'p.tar'))
