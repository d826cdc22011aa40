"""Host-side tests of feature quantisation (Zhao et al., ICML 2020, FQ-GAN).  The configuration surface (gan_lab_amd/quantize.py):
the ``fq_*`` fields, the command line, every refusal of the learner, checkpoints' config while the option is off.  And the
arithmetic as tests/fq_reference.py states it in plain torch: the reference against an independent composition (``torch.cdist`` /
``argmin`` / ``F.one_hot`` / autograd), the tie rule, the optimality and gap measures a GPU test of the layer will use, and the
smoothing on a code that was never used.  The layer itself is not in the package yet: a valid request for it is refused."""
import pytest
import torch
import torch.nn.functional as F

import fq_reference as ref

COMMON = dict(dev='cpu', pin_memory=False, res_samples=32, res_dataset=32)
FIELDS = ('fq_codes', 'fq_decay', 'fq_commit')
HINGE = dict(loss='hinge', gradient_penalty=None)


def _config(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', **{**COMMON, **kw})


def _build(monkeypatch, **kw):
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.resnetgan.learner import GANLearner
    cfg = _config(batch_size=4, len_latent=32, log_every=0, **kw)
    cfg.fmap_g = cfg.fmap_d = 16
    return GANLearner(cfg)


# ---- 0: config fields, the command line, the learner's refusals ---------------------------------------------------------------
def test_defaults_and_cli_round_trip(monkeypatch, tmp_path):
    from gan_lab_amd import config, quantize
    cfg = _config()
    assert tuple(getattr(cfg, f) for f in FIELDS) == (0, 0.8, 1.0)
    assert quantize.validate_config(cfg) is None                          # fq_codes = 0: the feature is off
    rows = {row[0]: row[1:] for row in config._spec('ResNet GAN')}
    assert rows['fq_codes'] == (int, 0) and rows['fq_decay'] == (float, 0.8) and rows['fq_commit'] == (float, 1.0)
    for model in ('ProGAN', 'StyleGAN'):
        assert not any(row[0].startswith('fq_') for row in config._spec(model))
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['resnetgan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(args)
    assert tuple(getattr(c, f) for f in FIELDS) == (0, 0.8, 1.0)
    c = config.main(args + ['--fq_codes=1024', '--fq_decay', '0.9', '--fq_commit=0.25'])
    assert tuple(getattr(c, f) for f in FIELDS) == (1024, 0.9, 0.25) and isinstance(c.fq_codes, int)
    assert quantize.validate_config(_config(fq_codes=1024, **HINGE)) == dict(codes=1024, decay=0.8, commit=1.0)
    assert quantize.validate_config(_config(fq_codes=1, fq_decay=0., fq_commit=0., **HINGE)) == dict(codes=1, decay=0., commit=0.)
    assert quantize.validate_config(_config(fq_codes=4096, **HINGE))['codes'] == 4096
    assert 'fq_codes' in config.__doc__ and 'nothing was tuned here' in config.__doc__


def test_checkpoint_config_is_unchanged_while_off():
    from gan_lab_amd import quantize
    assert not any(k.startswith('fq_') for k in quantize.saved_config_fields(vars(_config())))
    on = quantize.saved_config_fields(vars(_config(fq_codes=16, **HINGE)))
    assert all(f in on for f in FIELDS)


BAD = [(dict(fq_codes=-1), 'fq_codes'), (dict(fq_codes=4097), 'fq_codes'), (dict(fq_codes=2.5), 'fq_codes'),
       (dict(fq_codes=True), 'fq_codes'), (dict(fq_codes='16'), 'fq_codes'),
       (dict(fq_codes=16, fq_decay=1.0), 'fq_decay'), (dict(fq_codes=16, fq_decay=-0.1), 'fq_decay'),
       (dict(fq_decay=float('nan')), 'fq_decay'), (dict(fq_codes=16, fq_decay='0.8'), 'fq_decay'),
       (dict(fq_codes=16, fq_commit=-1.), 'fq_commit'), (dict(fq_commit=float('inf')), 'fq_commit'),
       (dict(fq_codes=16, fq_commit=True), 'fq_commit'),
       (dict(fq_codes=16, gradient_penalty='wgan-gp'), 'gradient_penalty'),
       (dict(fq_codes=16, loss='wgan', gradient_penalty='r1'), 'gradient_penalty')]


@pytest.mark.parametrize('kw,match', BAD, ids=[f'{m}-{i}' for i, (_, m) in enumerate(BAD)])
def test_invalid_values_raise_when_the_learner_is_built(monkeypatch, kw, match):
    from gan_lab_amd import quantize
    kw = {**HINGE, **kw}
    with pytest.raises(ValueError, match=match):
        quantize.validate_config(_config(**kw))
    with pytest.raises(ValueError, match=match):
        _build(monkeypatch, **kw)


def test_a_valid_request_is_refused_until_the_kernels_exist_and_off_builds_nothing(monkeypatch):
    from gan_lab_amd import quantize
    with pytest.raises(NotImplementedError, match='fq_codes=16'):
        _build(monkeypatch, fq_codes=16, **HINGE)
    quantize.require_layer(None)
    off = _build(monkeypatch, **HINGE)
    assert not any('fq' in k for k in off.disc_model.state_dict()) and not hasattr(off.disc_model, 'fq')


@pytest.mark.parametrize('model', ['progan', 'stylegan'])
def test_progressive_models_have_no_such_field(model):
    from gan_lab_amd import quantize
    from gan_lab_amd.config import make_config
    for field in FIELDS:
        with pytest.raises(AttributeError, match=field):
            make_config(model, **{field: 1})
    cfg = make_config(model, dev='cpu', pin_memory=False, gradient_penalty=None)
    assert quantize.validate_config(cfg) is None
    cfg.fq_codes = 16                                # set behind make_config's back
    with pytest.raises(ValueError, match='ResNet GAN'):
        quantize.validate_config(cfg)


def _data(shape, k, seed):
    g = torch.Generator().manual_seed(seed)
    n, c, hh, ww = shape
    embed = torch.randn(k, c, generator=g, dtype=torch.float64)
    pick = torch.randint(0, k, (n, hh, ww), generator=g)
    h = ref.unrows(embed[pick.reshape(-1)], shape) + 0.05 * torch.randn(shape, generator=g, dtype=torch.float64)
    return h, embed


# ---- 1: the reference against an independent composition ---------------------------------------------------------------------
@pytest.mark.parametrize('shape,k', [((1, 1, 1, 1), 1), ((3, 20, 5, 5), 70), ((2, 33, 1, 1), 5), ((2, 16, 4, 4), 9)])
def test_reference_equals_a_cdist_one_hot_composition(shape, k):
    h, embed = _data(shape, k, 3)
    gap, scale = ref.gaps(h, embed)
    assert bool((gap >= 1e-4 * scale).all())                         # gap-clear: both compositions must pick the same codes
    g = torch.Generator().manual_seed(4)
    embed_avg, cluster = torch.randn(k, shape[1], generator=g, dtype=torch.float64), torch.rand(k, generator=g, dtype=torch.float64)
    dout, dcommit, decay = torch.randn(shape, generator=g, dtype=torch.float64), 0.7, 0.8
    got = ref.run(h, embed, embed_avg, cluster, decay, dout, dcommit)
    # the independent composition: cdist / argmin / one_hot / autograd
    hr = h.clone().requires_grad_(True)
    flat = hr.permute(0, 2, 3, 1).reshape(-1, shape[1])
    idx = torch.cdist(flat.detach(), embed).argmin(1)
    assert torch.equal(got['idx'].reshape(-1).long(), idx)
    assert got['idx'].dtype == torch.int32 and tuple(got['idx'].shape) == (shape[0], shape[2], shape[3])
    onehot = F.one_hot(idx, k).double()
    q = (onehot @ embed).reshape(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
    out = hr + (q - hr).detach()
    commit = (q.detach() - hr).pow(2).mean()
    (out * dout).sum().backward(retain_graph=True)
    (commit * dcommit).backward()
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-14)      # noqa: E731
    assert close(got['out'], out.detach()) and close(got['commit'], commit.detach()) and close(got['dh'], hr.grad)
    n_k, s_k = onehot.sum(0), onehot.t() @ flat.detach()
    cs = decay * cluster + (1 - decay) * n_k
    ea = decay * embed_avg + (1 - decay) * s_k
    n = cs.sum()
    e = ea / ((cs + 1e-5) / (n + k * 1e-5) * n)[:, None]
    p = n_k / n_k.sum()
    ppl = torch.exp(-(p * torch.log(p + 1e-300)).sum())
    assert close(got['cluster_size'], cs) and close(got['embed_avg'], ea) and close(got['embed'], e)
    assert close(got['perplexity'], ppl)
    # without the commitment cotangent the gradient passes unchanged
    assert torch.equal(ref.backward(h, embed, got['idx'], dout, None), dout)
    # the float32 run (the CPU yardstick) picks the same codes on gap-clear data and stays close
    cpu = ref.run(h.float(), embed.float(), embed_avg.float(), cluster.float(), decay, dout.float(), dcommit, torch.float32)
    assert torch.equal(cpu['idx'], got['idx'])
    for name in ('out', 'commit', 'dh', 'embed', 'embed_avg', 'cluster_size', 'perplexity'):
        assert cpu[name].dtype == torch.float32 and torch.allclose(cpu[name].double(), got[name], rtol=1e-4, atol=1e-5), name


# ---- 2: the tie rule -------------------------------------------------------------------------------------------------------------
def test_the_lowest_code_wins_a_tie():
    embed = torch.tensor([[1., 0.], [3., 0.], [1., 0.], [-1., 0.], [3., 0.]])      # rows 0 = 2 and 1 = 4 are duplicates
    h = torch.tensor([[1., 0.], [2., 0.], [0., 0.], [3., 1.], [0., 5.]]).t().reshape(1, 2, 5, 1).contiguous()
    # rows: (1,0) -> code 0 (= 2); (2,0) equidistant from 0 and 1 -> 0; (0,0) equidistant from 0, 2, 3 -> 0; (3,1) -> 1 (= 4);
    # (0,5) equidistant from 0, 2, 3 -> 0
    for dtype in (torch.float64, torch.float32):
        assert ref.assign(h, embed, dtype).reshape(-1).tolist() == [0, 0, 0, 1, 0]
    s = torch.tensor([[2., 1., 1., 3.], [0., 0., 0., 0.], [5., 4., 3., 3.]])
    assert ref.first_argmin(s).tolist() == [1, 0, 2]


# ---- 3: the measures of a GPU test ------------------------------------------------------------------------------------------------
def test_gap_and_optimality_measures():
    embed = torch.tensor([[0., 0.], [4., 0.], [0., 3.]], dtype=torch.float64)
    h = torch.tensor([[1., 0.], [2., 0.], [0., 2.]], dtype=torch.float64).t().reshape(1, 2, 3, 1).contiguous()
    # scores |e|^2 - 2 <h, e>: row (1,0): 0, 8, 9; row (2,0): 0, 0, 9 (a tie); row (0,2): 0, 16, -3
    gap, scale = ref.gaps(h, embed)
    assert gap.tolist() == [8., 0., 3.] and scale.tolist() == [1., 4., 13.]
    best = ref.assign(h, embed)
    assert best.reshape(-1).tolist() == [0, 0, 2]
    excess, scale = ref.optimality(h, embed, best)
    assert excess.tolist() == [0., 0., 0.]
    other = torch.tensor([1, 1, 0], dtype=torch.int32).reshape(1, 3, 1)
    excess, scale = ref.optimality(h, embed, other)
    assert excess.tolist() == [8., 0., 3.] and scale.tolist() == [17., 20., 13.]      # |h|^2 + max(|e_chosen|^2, |e_best|^2)
    one = ref.gaps(h, embed[:1])
    assert bool(torch.isinf(one[0]).all())


# ---- 4: the smoothing ------------------------------------------------------------------------------------------------------------
def test_an_unused_code_stays_finite():
    h, embed = _data((2, 6, 3, 3), 4, 5)
    embed = torch.cat((embed, 100. + torch.zeros(2, 6, dtype=torch.float64)))      # two codes far from every row
    for dtype in (torch.float64, torch.float32):
        e, ea, cs = embed.clone(), embed.clone(), torch.zeros(6, dtype=torch.float64)
        for _ in range(3):
            r = ref.run(h, e, ea, cs, 0.8, None, None, dtype)
            e, ea, cs = r['embed'], r['embed_avg'], r['cluster_size']
            assert int((cs[4:] == 0).sum()) == 2                     # never used ...
            assert bool(torch.isfinite(e).all()) and float(e[4:].abs().max()) > 0      # ... and still finite
        assert 1.0 <= float(r['perplexity']) <= 4.0 + 1e-6


def test_second_pass_uses_the_updated_dictionary():
    # the moving average holds the codes swapped: one update moves code 0 to 5.5 and code 1 to 4.5, and every row changes sides
    h = torch.tensor([1., 1., 9., 9.]).reshape(4, 1, 1, 1)
    embed, embed_avg, cluster = torch.tensor([[0.], [10.]]), torch.tensor([[20.], [0.]]), torch.tensor([2., 2.])
    first = ref.run(h, embed, embed_avg, cluster, 0.5, None, None)
    assert first['idx'].reshape(-1).tolist() == [0, 0, 1, 1] and first['cluster_size'].tolist() == [2., 2.]
    assert torch.allclose(first['embed'], torch.tensor([[5.5], [4.5]], dtype=torch.float64), rtol=1e-5)
    assert abs(float(first['perplexity']) - 2.0) <= 1e-12
    assert ref.assign(h, first['embed']).reshape(-1).tolist() == [1, 1, 0, 0]
