"""Host-side tests of latent-space projection (gan_lab_amd/project.py): the float64 reference (tests/project_reference.py) against
itself and against torch.optim.Adam, the schedule at the points where its value can be derived by hand, and every refusal that needs
no GPU."""
import math

import pytest
import torch

import project_reference as ref


# ---- 1: the reference against itself -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,weights', [((2, 1, 4, 4), [1., 1., 1.]), ((2, 3, 16, 16), [1., .5, .25, 2., 4.]),
                                           ((1, 2, 64, 64), [0., 0., 0., 0., 0., 1.]), ((3, 3, 32, 32), [1.] * 6)])
def test_autograd_gradient_equals_the_analytic_formula(shape, weights):
    g = torch.Generator().manual_seed(0)
    x, t = torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
    auto, formula = ref.pyramid_grad_autograd(x, t, weights), ref.pyramid_grad_analytic(x, t, weights)
    assert (auto - formula).abs().max() <= 1e-14 * formula.abs().max()
    up = torch.tensor([2., 0., -1.][:shape[0]], dtype=torch.float64)
    scaled = ref.pyramid_grad_autograd(x, t, weights, upstream=up)
    assert (scaled - formula * up.view(-1, 1, 1, 1)).abs().max() <= 1e-14 * formula.abs().max()
    terms = ref.pyramid_terms(x, t, len(weights))
    assert terms.shape == (shape[0], len(weights))
    assert torch.allclose(terms[:, 0], ((x - t) ** 2).mean(dim=(1, 2, 3)), rtol=1e-14)
    assert torch.allclose(ref.pyramid_loss(x, t, weights), (terms * torch.tensor(weights, dtype=torch.float64)).sum(1), rtol=1e-14)


def test_schedule_at_the_derivable_points():
    n, w_std = 1000, 3.0
    lr, scale = ref.schedule(0, n, w_std)
    assert lr.item() == 0.0                                               # the ramp-up starts at zero
    assert abs(scale.item() - w_std * 0.05) <= 1e-15                      # the full exploration noise
    for step in (50, 400, 750):                                           # between the ramps: t in [0.05, 0.75]
        assert abs(ref.schedule(step, n, w_std)[0].item() - 0.1) <= 1e-15
    for step in (750, 900, 1000):                                         # t >= noise_ramp_length
        assert ref.schedule(step, n, w_std)[1].item() == 0.0
    assert 0.0 < ref.schedule(25, n, w_std)[0].item() < 0.1 and 0.0 < ref.schedule(900, n, w_std)[0].item() < 0.1
    assert abs(ref.schedule(1000, n, w_std)[0].item()) <= 1e-15           # the cosine ramp-down ends at zero
    lr, scale = ref.schedule(875, n, w_std, lr0=0.2, initial_noise_factor=0.1, noise_ramp_length=1.0)
    assert abs(lr.item() - 0.2 * 0.5) <= 1e-15                            # half-way down the cosine: r = 0.5
    assert abs(scale.item() - w_std * 0.1 * 0.125 ** 2) <= 1e-15
    assert ref.schedule(3, 8, 1.0, torch.float32)[0].dtype == torch.float32


@pytest.mark.parametrize('space', ['w', 'w+'])
def test_one_step_against_torch_adam(space):
    g = torch.Generator().manual_seed(1)
    n, layers, d, num_steps = 2, 6, 16, 8
    shape = (n, d) if space == 'w' else (n, layers, d)
    w0 = torch.randn(shape, generator=g, dtype=torch.float64)
    grads = [torch.randn(n, layers, d, generator=g, dtype=torch.float64) for _ in range(3)]
    noise = torch.randn(shape, generator=g, dtype=torch.float64)
    state = dict(w_opt=w0.clone(), m=torch.zeros_like(w0), v=torch.zeros_like(w0), step=0)
    p = w0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.1, betas=(ref.BETA1, ref.BETA2), eps=ref.EPS)
    for k, grad in enumerate(grads):
        for group in opt.param_groups:
            group['lr'] = ref.schedule(k, num_steps, 1.0)[0].item()
        p.grad = grad.sum(1) if space == 'w' else grad.clone()
        opt.step()
        out = ref.project_step(state, grad, noise, 0.7, num_steps)
        assert state['step'] == k + 1
        assert torch.allclose(state['w_opt'], p.detach(), rtol=1e-12, atol=1e-14)
        scale = ref.schedule(k + 1, num_steps, 0.7)[1]
        want = p.detach() + scale * noise
        assert torch.allclose(out, want.unsqueeze(1).expand(n, layers, d) if space == 'w' else want, rtol=1e-12, atol=1e-14)
    assert not torch.equal(state['w_opt'], w0)


def test_w_moments_reference():
    ws = 100 + torch.randn(1000, 16, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    avg, std = ref.w_moments(ws)
    assert torch.allclose(avg, ws.mean(0), rtol=1e-14)
    assert abs(std.item() - math.sqrt(((ws - ws.mean(0)) ** 2).sum().item() / 1000)) <= 1e-13
    assert 3.5 < std.item() < 4.5                                         # sqrt(D) for unit-variance rows


# ---- 2: the refusals that need no GPU --------------------------------------------------------------------------------------------
@pytest.fixture
def learner(monkeypatch):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd import progressive as P
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    old = (P.FMAP_BASE, P.FMAP_MAX)
    P.FMAP_BASE, P.FMAP_MAX = 64, 16
    try:
        cfg = make_config('stylegan', dev='cpu', pin_memory=False, res_samples=16, res_dataset=16, init_res=16, batch_size=4,
                          len_latent=16, len_dlatent=16, mapping_num_fcs=2, cutoff_trunc_trick=None,
                          num_iters_save_model=10 ** 9, log_every=0)
        L = StyleGANLearner(cfg)
        L.ds_mean, L.ds_std = torch.full((3,), .5), torch.full((3,), .5)
        yield L
    finally:
        P.FMAP_BASE, P.FMAP_MAX = old


BAD = [(dict(steps=0), 'steps'), (dict(steps=2.5), 'steps'), (dict(steps=True), 'steps'),
       (dict(space='z'), 'space'), (dict(space='W'), 'space'),
       (dict(noise_mode='random'), 'noise_mode'),
       (dict(levels=0), 'levels'), (dict(levels=6), 'levels'), (dict(levels=2.0), 'levels'),      # 16x16 allows five
       (dict(weights=[]), 'weights'), (dict(weights=[1.] * 6), 'weights'), (dict(weights=[1., -1.]), 'weights'),
       (dict(weights=[float('nan')]), 'weights'), (dict(weights=[0., 0.]), 'weights'), (dict(weights='ab'), 'weights'),
       (dict(levels=3, weights=[1., 1.]), 'weights'),
       (dict(w_avg_samples=0), 'w_avg_samples'), (dict(seed=-1), 'seed'), (dict(seed=1.5), 'seed'),
       (dict(lr0=-0.1), 'lr0'), (dict(lr0=float('inf')), 'lr0'), (dict(initial_noise_factor=-1.), 'initial_noise_factor'),
       (dict(lr_rampdown_length=0.), 'lr_rampdown_length'), (dict(lr_rampup_length=1.5), 'lr_rampup_length'),
       (dict(noise_ramp_length=float('nan')), 'noise_ramp_length'), (dict(momentum=0.9), 'momentum')]


@pytest.mark.parametrize('kw,match', BAD, ids=[f'{m}-{i}' for i, (_, m) in enumerate(BAD)])
def test_bad_arguments_are_refused_by_name(learner, kw, match):
    with pytest.raises(ValueError, match=match):
        learner.project(torch.rand(2, 3, 16, 16), **kw)


def test_bad_targets_and_learner_states_are_refused(learner):
    for bad in (torch.rand(2, 3, 8, 8), torch.rand(2, 3, 32, 32), torch.rand(2, 1, 16, 16), torch.rand(3, 16, 16),
                torch.rand(0, 3, 16, 16), [[0.]]):
        with pytest.raises(ValueError, match='targets'):
            learner.project(bad)
    learner.gen_model.fade_in_phase = True
    try:
        with pytest.raises(ValueError, match='fade_in_phase'):
            learner.project(torch.rand(2, 3, 16, 16))
        with pytest.raises(ValueError, match='fade_in_phase'):
            learner.gen_model.synthesis(torch.zeros(2, 16))
    finally:
        learner.gen_model.fade_in_phase = False
    learner.ds_std = None
    with pytest.raises(ValueError, match='ds_mean'):
        learner.project(torch.rand(2, 3, 16, 16))


def test_synthesis_refuses_misshapen_dlatents(learner):
    g = learner.gen_model
    assert len(g.gen_layers) == 6
    for bad in (torch.zeros(2, 5, 16), torch.zeros(2, 6, 8), torch.zeros(2, 8), torch.zeros(16), None):
        with pytest.raises(ValueError, match='ws'):
            g.synthesis(bad)


def test_only_stylegan_learns_to_project():
    from gan_lab_amd.progan.learner import ProGANLearner
    from gan_lab_amd.resnetgan.learner import GANLearner
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    assert hasattr(StyleGANLearner, 'project')
    assert not hasattr(ProGANLearner, 'project') and not hasattr(GANLearner, 'project')


def test_option_defaults_and_ops_have_no_cpu_path():
    from gan_lab_amd import ops, project
    weights, hyper = project.check_options(1024, 1000, 'w', None, None, 'const', 10000, 0, {})
    assert weights == (1.,) * 6 and hyper == (0.1, 0.05, 0.25, 0.05, 0.75, 1000.)
    assert project.check_options(8, 5, 'w+', None, None, 'none', 1, 3, dict(lr0=0.2))[0] == (1.,) * 4
    assert project.check_options(16, 5, 'w', 2, None, 'none', 1, 3, {})[0] == (1., 1.)
    assert project.check_options(16, 5, 'w', None, [0., 2.], 'none', 1, 3, {})[0] == (0., 2.)
    assert [ops.pyramid_max_levels(r) for r in (4, 8, 16, 32, 1024)] == [3, 4, 5, 6, 6]
    for r in (2, 48, 2048, 16.0):
        with pytest.raises(ValueError, match='power of two'):
            ops.pyramid_max_levels(r)
    assert project._substream(0, 0) != project._substream(0, 1) != project._substream(1, 0)
    a = torch.zeros(1, 1, 4, 4)
    for call in (lambda: ops.pyramid_mse(a, a, [1.]), lambda: ops.w_moments(torch.zeros(4, 4)),
                 lambda: ops.project_step(a[0], None, a[0], a[0], torch.zeros(1).int(), a[0], torch.zeros(()), a[0],
                                          (0.1, 0.05, 0.25, 0.05, 0.75, 8.))):
        with pytest.raises(TypeError, match='no CPU fallback'):
            call()
