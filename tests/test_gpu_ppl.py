"""The perceptual path length on the GPU (csrc/ppl.hip, gan_lab_amd/ppl.py) against the float64 restatement
(tests/ppl_reference.py), with the same restatement in float32 on the CPU as the yardstick where a bound is relative, and the
learners' 'ppl' metric against a hand composition from the same ops."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ppl_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (3, 63), (257, 64), (4, 513), (2, 4096)]
EPS = 1e-4
SEED, OFFSET = 0x1234567890ABCDEF, 3


def ulp(x):
    """The spacing of float32 at |x| (float64 array in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)


def _slerp_errors(tag, a, b, t, got, d):
    """Assert the slerp bound on the points and on their difference; returns the float32 CPU restatement."""
    want = ref.endpoints(a, b, t, EPS, 'slerp').numpy()
    cpu = ref.endpoints(a, b, t, EPS, 'slerp', torch.float32).double().numpy()
    floor = 2 * float(ulp(np.sqrt(d)))
    assert np.isfinite(got).all()
    for name, g, c, w in (('points', got, cpu, want), ('difference', got[1] - got[0], cpu[1] - cpu[0], want[1] - want[0])):
        e_gpu, e_cpu = np.abs(g - w).max(), np.abs(c - w).max()
        print(f'slerp {tag} {name}: gpu {e_gpu:.3e}, float32 cpu {e_cpu:.3e}, ratio {e_gpu / max(e_cpu, 1e-300):.3f}, '
              f'floor {floor:.3e}')
        assert e_gpu <= max(2 * e_cpu, floor), name
    return cpu, floor


# ---- ppl_endpoints -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampling', ['full', 'end'])
@pytest.mark.parametrize('n,d', SHAPES)
def test_endpoints_draw_and_lerp(n, d, sampling):
    from gan_lab_amd import ops
    a, b = _rows(n, d, 10 * n + d)
    t, out = ops.ppl_endpoints(a.cuda(), b.cuda(), EPS, 'lerp', sampling, SEED, OFFSET)
    want_t = ref.uniforms(SEED, OFFSET, n) if sampling == 'full' else np.zeros(n)
    assert t.dtype == torch.float32 and tuple(t.shape) == (n,) and tuple(out.shape) == (2, n, d)
    assert np.array_equal(t.cpu().double().numpy(), want_t)                          # the restated draw, exactly
    want = ref.endpoints(a, b, want_t, EPS, 'lerp').numpy()
    err = np.abs(out.cpu().double().numpy() - want)
    print(f'lerp {sampling} ({n}, {d}): worst error {np.max(err / ulp(want)):.3f} ulp of the entry')
    assert (err <= ulp(want)).all()                                                  # 1 ulp per entry, of the entry itself


@pytest.mark.parametrize('sampling', ['full', 'end'])
@pytest.mark.parametrize('n,d', SHAPES)
def test_endpoints_slerp_against_float64(n, d, sampling):
    """The error against float64 of the points and of their difference ``out[1] - out[0]`` is at most twice the float32 CPU
    restatement's on the same inputs (both are valid orders of D-term fp32 dot products), with a floor of 2 ulps of sqrt(D)."""
    from gan_lab_amd import ops
    a, b = _rows(n, d, 20 * n + d)
    t, out = ops.ppl_endpoints(a.cuda(), b.cuda(), EPS, 'slerp', sampling, SEED, OFFSET)
    want_t = ref.uniforms(SEED, OFFSET, n) if sampling == 'full' else np.zeros(n)
    assert np.array_equal(t.cpu().double().numpy(), want_t)
    got = out.cpu().double().numpy()
    _slerp_errors(f'{sampling} ({n}, {d})', a, b, want_t, got, d)
    # every row sits on the sphere of radius sqrt(D)
    norms = np.sqrt((got ** 2).sum(-1))
    print(f'slerp {sampling} ({n}, {d}) norms: worst {np.max(np.abs(norms - np.sqrt(d)) / ulp(np.sqrt(d))):.3f} ulp of sqrt(D)')
    assert (np.abs(norms - np.sqrt(d)) <= 4 * ulp(np.sqrt(d))).all()


@pytest.mark.parametrize('d', sorted({d for _, d in SHAPES}))
def test_endpoints_slerp_fallback_rows(d):
    """Rows b = a, b = -a, b = 2a, a = 0 and b = 0 (and one ordinary row): both ends are a / |a| sqrt(D) - a itself where
    |a| = 0 -, finite, within the slerp bound of the float64 restatement of that rule."""
    from gan_lab_amd import ops
    a, b = _rows(6, d, 30 + d)
    b[0], b[1], b[2] = a[0], -a[1], 2 * a[2]
    a[3], b[4] = 0, 0
    t, out = ops.ppl_endpoints(a.cuda(), b.cuda(), EPS, 'slerp', 'full', SEED, OFFSET)
    got = out.cpu().double().numpy()
    _slerp_errors(f'fallback rows D={d}', a, b, ref.uniforms(SEED, OFFSET, 6), got, d)
    flat = [0, 1, 2, 3, 4] if d > 1 else [0, 1, 2, 3, 4, 5]          # D = 1: every pair is parallel or antipodal
    assert np.array_equal(got[0, flat], got[1, flat]) and (got[:, 3] == 0).all()
    if d > 1:
        assert not np.array_equal(got[0, 5], got[1, 5])
    # a / |a| sqrt(D) in fp32: |a|^2 summed (about an ulp), its root, the division, sqrt(D) and the product round once each -
    # under 4 ulps of an entry, and an entry is at most sqrt(D)
    a64 = a.double().numpy()
    for i in (0, 1, 2, 4):
        want = a64[i] / np.sqrt((a64[i] ** 2).sum()) * np.sqrt(d)
        assert (np.abs(got[0, i] - want) <= 4 * ulp(np.sqrt(d))).all()
    norms = np.sqrt((got ** 2).sum(-1))[:, [0, 1, 2, 4, 5]]
    assert (np.abs(norms - np.sqrt(d)) <= 4 * ulp(np.sqrt(d))).all()


def test_endpoints_short_draw_is_the_prefix_of_a_long_one():
    from gan_lab_amd import ops
    a, b = _rows(257, 8, 5)
    a, b = a.cuda(), b.cuda()
    t_long, out_long = ops.ppl_endpoints(a, b, EPS, 'slerp', 'full', SEED, 0)
    t_short, out_short = ops.ppl_endpoints(a[:5], b[:5], EPS, 'slerp', 'full', SEED, 0)
    assert torch.equal(t_short, t_long[:5]) and torch.equal(out_short, out_long[:, :5])
    t_off, _ = ops.ppl_endpoints(a[:5], b[:5], EPS, 'slerp', 'full', SEED, 100)
    assert torch.equal(t_off, t_long[100:105])
    again = ops.ppl_endpoints(a, b, EPS, 'slerp', 'full', SEED, 0)
    assert torch.equal(again[0], t_long) and torch.equal(again[1], out_long)          # bitwise reproducible
    assert not torch.equal(ops.ppl_endpoints(a, b, EPS, 'slerp', 'full', SEED + 1, 0)[0], t_long)


def test_endpoints_argument_checks():
    from gan_lab_amd import ops
    z = torch.zeros(4, 8, device='cuda')
    for args, name in (((z, z[:3], EPS, 'lerp'), 'equal'), ((z, z, EPS, 'nlerp'), 'mode'), ((z, z, EPS, 'lerp', 'mid'), 'sampling'),
                       ((z, z, 0.0, 'lerp'), 'epsilon'), ((z, z, EPS, 'lerp', 'full', 0, -1), 'offset'),
                       ((torch.zeros(2, 4097, device='cuda'),) * 2 + (EPS, 'lerp'), 'width'), ((z[0], z[0], EPS, 'lerp'), 'ppl_endpoints a')):
        with pytest.raises(ValueError, match=name):
            ops.ppl_endpoints(*args)
    with pytest.raises(TypeError, match='ppl_endpoints b'):
        ops.ppl_endpoints(z, z.double(), EPS, 'lerp')
    t, out = ops.ppl_endpoints(z.t()[:, :4], z.t()[:, :4], EPS, 'lerp')                # a non-contiguous view is copied
    assert tuple(out.shape) == (2, 8, 4)


# ---- row_sqdist --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(1, 1), (3, 7), (130, 4099)])
def test_row_sqdist(n, d):
    from gan_lab_amd import ops
    g = torch.Generator().manual_seed(n + d)
    xi, yi = torch.randint(-9, 10, (n, d), generator=g).float(), torch.randint(-9, 10, (n, d), generator=g).float()
    got = ops.row_sqdist(xi.cuda(), yi.cuda())
    assert torch.equal(got.cpu().double(), ref.row_sqdist(xi, yi))                    # integer rows: exact
    x, y = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    got = ops.row_sqdist(x.cuda(), y.cuda())
    want = ref.row_sqdist(x, y).numpy()
    err = np.abs(got.cpu().double().numpy() - want)
    print(f'row_sqdist ({n}, {d}): worst error {np.max(err / ulp(want)):.3f} ulp')
    assert (err <= ulp(want)).all()
    both = torch.cat([x, y]).cuda()                                                   # the halves of one tensor
    assert torch.equal(ops.row_sqdist(both[:n], both[n:]), got)
    out = torch.full((n + 2,), -1.0, device='cuda')
    assert ops.row_sqdist(both[:n], both[n:], out=out[1:n + 1]).data_ptr() == out[1:].data_ptr()
    assert torch.equal(out[1:n + 1], got) and out[0] == -1 and out[-1] == -1
    with pytest.raises(ValueError, match='equal'):
        ops.row_sqdist(both[:n], both[:n, :-1] if d > 1 else both)


# ---- trimmed_mean ------------------------------------------------------------------------------------------------------------
def _straddle(n, rng):
    """Random values with a block of equal values across each of the two bounds of the (1, 99) trim."""
    v = np.sort(rng.standard_normal(n).astype(np.float32))
    lo, hi = int(np.floor(0.01 * (n - 1))), int(np.ceil(0.99 * (n - 1)))
    w = max(2, n // 50)
    v[max(lo - w // 2, 0):lo + w] = v[lo]
    v[hi - w:min(hi + w // 2 + 1, n)] = v[hi]
    return rng.permutation(v)


@pytest.mark.parametrize('n', [1, 2, 100, 101, 1000, 4097, 2 ** 17 + 1])
def test_trimmed_mean(n):
    from gan_lab_amd import ops
    rng = np.random.default_rng(n)
    base = (rng.standard_normal(n) ** 2).astype(np.float32)
    cases = {'random': base, 'sorted': np.sort(base), 'reversed': np.sort(base)[::-1].copy(),
             'equal': np.full(n, 0.37, dtype=np.float32), 'straddle': _straddle(n, rng), 'signed': _straddle(n, rng) - 0.5}
    for name, v in cases.items():
        got = dict(zip(ops.PPL_RECORD, ops.trimmed_mean(torch.from_numpy(v).cuda()).cpu().tolist()))
        want = ref.trimmed_mean(v)
        assert (got['lo'], got['hi'], got['kept'], got['nonfinite']) == (want['lo'], want['hi'], want['kept'], 0), (name, got, want)
        assert abs(got['mean'] - want['mean']) <= 1e-12 * abs(want['mean']), (name, got['mean'], want['mean'])
        if name == 'straddle' and n >= 100:
            assert (v == want['lo']).sum() > 1 and (v == want['hi']).sum() > 1            # ties at both bounds, all kept
    v = torch.from_numpy(base).cuda()
    assert torch.equal(ops.trimmed_mean(v), ops.trimmed_mean(v))
    got = ops.trimmed_mean(v, 0.25, 0.5).cpu().tolist()
    want = ref.trimmed_mean(base, 0.25, 0.5)
    assert got[1:4] == [want['lo'], want['hi'], want['kept']] and abs(got[0] - want['mean']) <= 1e-12 * abs(want['mean'])
    for bad in (float('nan'), float('inf'), -float('inf')):
        w = base.copy()
        w[n // 2] = bad
        got = ops.trimmed_mean(torch.from_numpy(w).cuda()).cpu().tolist()
        assert np.isnan(got[0]) and got[4] == 1
    with pytest.raises(ValueError, match='q_lo'):
        ops.trimmed_mean(v, 0.6, 0.4)
    with pytest.raises(ValueError, match='non-empty'):
        ops.trimmed_mean(v[:0])


# ---- path_length on a linear map -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampling', ['full', 'end'])
def test_path_length_of_a_linear_map_is_its_closed_form(sampling):
    """``synth(w) = (w A).view(B, 3, 8, 8)`` under 'lerp': the two ends differ by ``eps (b - a) A`` whatever t is, so every
    ``distances[n] / eps^2`` is ``mean(((b - a) A)^2)``.  With eps = 2^-7 each end carries a relative rounding of 2^-24 against
    a step of 2^-7 of it - about 2^-16 = 1.5e-5 relative in the difference, twice that in its square; 1e-3 leaves an order of
    magnitude for the rows whose step is small beside the point it is taken at."""
    from gan_lab_amd import ops, ppl
    g = torch.Generator().manual_seed(2)
    n, d, eps = 40, 24, 2.0 ** -7
    a, b, m = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g), torch.randn(d, 192, generator=g) / d ** 0.5
    mc = m.cuda()
    calls = []

    def synth(w):
        calls.append(tuple(w.shape))
        return (w @ mc).view(-1, 3, 8, 8)

    out = ppl.path_length(synth, a.cuda(), b.cuda(), 'lerp', sampling=sampling, epsilon=eps, batch=16, weights=(1.0,), seed=5)
    assert calls == [(32, d), (32, d), (16, d)]                                       # ONE call per batch, on both ends
    want = (((b.double() - a.double()) @ m.double()) ** 2).mean(1).numpy()
    got = out['distances'].cpu().double().numpy() / eps ** 2
    print(f'linear map, {sampling}: worst relative error {np.max(np.abs(got - want) / want):.3e}')
    assert (np.abs(got - want) <= 1e-3 * want).all()
    rec = ref.trimmed_mean(out['distances'].cpu().numpy())
    assert (out['lo'], out['hi'], out['kept']) == (rec['lo'], rec['hi'], rec['kept']) and out['kept'] == n
    assert abs(out['ppl'] - rec['mean'] / eps ** 2) <= 1e-12 * out['ppl']
    emb = ppl.path_length(synth, a.cuda(), b.cuda(), 'lerp', sampling=sampling, epsilon=eps, batch=16,
                          embed=lambda x: x.flatten(1), seed=5)
    got = emb['distances'].cpu().double().numpy() / eps ** 2
    assert (np.abs(got - 192 * want) <= 1e-3 * 192 * want).all()
    # the batch size does not move a pair's t: the same distances, up to the matmul's own dependence on its row count
    one = ppl.path_length(synth, a.cuda(), b.cuda(), 'lerp', sampling=sampling, epsilon=eps, batch=64, weights=(1.0,), seed=5)
    assert np.allclose(one['distances'].cpu().numpy(), out['distances'].cpu().numpy(), rtol=1e-3)
    # the default weights: every level 8x8 allows
    full = ppl.path_length(synth, a.cuda(), b.cuda(), 'lerp', sampling=sampling, epsilon=eps, batch=16, seed=5)
    x = (torch.stack([a, b]).double() @ m.double()).view(2, n, 3, 8, 8)
    lv = ref.pyramid_mse(x[1], x[0], (1.0,) * ops.pyramid_max_levels(8)).numpy()
    assert (np.abs(full['distances'].cpu().double().numpy() / eps ** 2 - lv) <= 1e-3 * lv).all()


# ---- the learners ------------------------------------------------------------------------------------------------------------
def make_learner(kind, seed=1, **kw):
    from gan_lab_amd import progressive as P
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    common = dict(dev='cuda', pin_memory=False, res_samples=16, res_dataset=16, init_res=16, batch_size=16, len_latent=16,
                  nimg_transition=24, num_iters_save_model=10 ** 9, log_every=0, random_seed=seed)
    common.update(kw)
    old = (P.FMAP_BASE, P.FMAP_MAX)
    P.FMAP_BASE, P.FMAP_MAX = 256, 16
    torch.manual_seed(seed)                                  # the layers' initial weights come from torch's generator
    try:
        if kind == 'stylegan':
            L = StyleGANLearner(make_config('stylegan', len_dlatent=16, mapping_num_fcs=2, cutoff_trunc_trick=None, **common))
        else:
            L = ProGANLearner(make_config('progan', **common))
    finally:
        P.FMAP_BASE, P.FMAP_MAX = old
    with torch.no_grad():
        for k, p in L.gen_model.named_parameters():
            if k.endswith('bias') or k.endswith('noise_weight'):
                p.normal_(0, 0.3)
    L.ewma.flat.copy_(L.arena_g.flat)
    return L


def _snapshot(L):
    from gan_lab_amd import rng
    gens = [L.gen_model] + ([L.gen_model_lagged] if L.gen_model_lagged is not None else [])
    return {'state': [copy.deepcopy(g.state_dict()) for g in gens] + [copy.deepcopy(L.disc_model.state_dict())],
            'ewma': L.ewma.flat.clone(), 'modes': [[m.training for m in g.modules()] for g in gens],
            'flags': [[p.requires_grad for p in g.parameters()] for g in gens],
            'switches': [(getattr(g, '_use_noise', None), getattr(g, '_use_mixing_reg', None),
                          getattr(g, 'use_truncation_trick', None), getattr(g, 'w_ewma', None)) for g in gens],
            'lagged': L.gen_model_lagged, 'rng': dict(rng._STATE), 'torch': torch.get_rng_state(), 'numpy': np.random.get_state()[1]}


def _same(a, b):
    assert a['lagged'] is b['lagged'] and a['rng'] == b['rng'] and a['modes'] == b['modes'] and a['flags'] == b['flags']
    assert a['switches'] == b['switches'] and torch.equal(a['ewma'], b['ewma'])
    assert torch.equal(a['torch'], b['torch']) and np.array_equal(a['numpy'], b['numpy'])
    for sa, sb in zip(a['state'], b['state']):
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def _by_hand(gen, kind, space, n, batch, seed, sampling='full', eps=EPS):
    """The distances composed in the test from the same ops, with the same batching and the documented sub-streams."""
    from gan_lab_amd import ops, ppl
    dev = 'cuda'
    z = ops.randn((2 * n, gen.len_latent), ppl._substream(seed, 0), 0, dev)
    if space == 'w':
        z = gen.z_to_w(z)
    a, b = z[:n], z[n:]
    out = []
    for bi, i0 in enumerate(range(0, n, batch)):
        k = min(batch, n - i0)
        _, ends = ops.ppl_endpoints(a[i0:i0 + k], b[i0:i0 + k], eps, 'lerp' if space == 'w' else 'slerp', sampling,
                                    ppl._substream(seed, 1), i0)
        rows = ends.view(2 * k, -1)
        if kind == 'stylegan':
            sides = [4 * 2 ** (j // 2) for j in range(len(gen.gen_layers))]
            per = sum((s * s + 3) // 4 for s in sides)
            maps, off = [], bi * per
            for s in sides:
                maps.append(ops.randn((1, 1, s, s), ppl._substream(seed, 2), off, dev))
                off += (s * s + 3) // 4
            x = gen.synthesis(gen.z_to_w(rows) if space == 'z' else rows, noise=maps)
        else:
            x = gen(rows)
        out.append(ops.pyramid_mse(x[:k], x[k:], (1.0,) * ops.pyramid_max_levels(16))[0])
    return torch.cat(out)


@pytest.mark.parametrize('kind,space', [('stylegan', 'w'), ('stylegan', 'z'), ('progan', 'z')])
def test_learner_path_length(kind, space, capsys):
    from gan_lab_amd import ppl
    L = make_learner(kind, gen_metrics=['ppl'], disc_metrics=[], ppl_samples=40, ppl_space=space, ppl_seed=3)
    L.gen_model.train()
    before = _snapshot(L)
    first = ppl.generator_path_length(L, 40, space, batch=16, seed=3)
    _same(before, _snapshot(L))                              # the learner is exactly as found (no EWMA copy was left behind)
    assert L.gen_model_lagged is None and tuple(first['distances'].shape) == (40,)
    d = first['distances']
    assert torch.isfinite(d).all() and (d > 0).all() and np.isfinite(first['ppl']) and first['ppl'] > 0
    assert 38 <= first['kept'] <= 40 and first['lo'] <= first['hi']
    second = ppl.generator_path_length(L, 40, space, batch=16, seed=3)
    assert torch.equal(second['distances'], d) and second['ppl'] == first['ppl']     # bitwise
    other = ppl.generator_path_length(L, 40, space, batch=16, seed=4)
    assert not torch.equal(other['distances'], d)
    # a hand composition from the same ops with the same batching (16, 16 and a ragged 8), on the generator scored: the
    # time-averaged one, equal to the live one's values here
    gen = L.materialize_lagged_generator().to('cuda').eval()
    L.gen_model_lagged = None
    if kind == 'stylegan':
        gen.use_truncation_trick = False
    with torch.no_grad():
        hand = _by_hand(gen, kind, space, 40, 16, 3)
    assert torch.equal(hand, d)
    rec = ref.trimmed_mean(d.cpu().numpy())
    assert (first['lo'], first['hi'], first['kept']) == (rec['lo'], rec['hi'], rec['kept'])
    assert abs(first['ppl'] - rec['mean'] / EPS ** 2) <= 1e-12 * first['ppl']
    # 'end' sampling and the live generator are other numbers of the same kind
    end = ppl.generator_path_length(L, 40, space, sampling='end', batch=16, seed=3, time_average=False)
    assert torch.isfinite(end['distances']).all() and not torch.equal(end['distances'], d)
    with torch.no_grad():
        live = copy.deepcopy(L.gen_model).eval()
        if kind == 'stylegan':
            live.use_truncation_trick = False
        assert torch.equal(_by_hand(live, kind, space, 40, 16, 3, sampling='end'), end['distances'])

    # compute_metrics: the same number, and its line; no validation reals
    z_dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.randn(16, 16)), batch_size=16)
    capsys.readouterr()
    lines = L.compute_metrics(['ppl'], 'Generator', z_dl, None)
    print(*lines)
    shown = capsys.readouterr().out
    got = L.last_metrics['generator']['ppl']
    assert got['ppl'] == first['ppl'] and torch.equal(got['distances'], d) and got['space'] == space
    assert [ln.split(':')[0].strip() for ln in lines] == ['ppl'] and ('%.4g' % first['ppl']) in shown
    assert L.gen_model.training and L.disc_model.training

    # refusals
    with pytest.raises(ValueError, match='fade_in_phase'):
        L.gen_model.fade_in_phase = True
        try:
            ppl.generator_path_length(L, 40, space)
        finally:
            L.gen_model.fade_in_phase = False
    if kind == 'progan':
        with pytest.raises(ValueError, match="space='w'"):
            ppl.generator_path_length(L, 40, 'w')
    with pytest.raises(ValueError, match='n_samples'):
        ppl.generator_path_length(L, 1, space)


def test_compute_metrics_reports_nan_while_a_resolution_fades_in():
    L = make_learner('progan', gen_metrics=['ppl'], disc_metrics=[], ppl_samples=8)
    L.gen_model.fade_in_phase = True                         # the 16x16 stage of a learner grown from 4x4 has its prev_torgb
    L.gen_model.alpha = 0.5
    z_dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.randn(16, 16)), batch_size=16)
    lines = L.compute_metrics(['ppl'], 'Generator', z_dl, None)
    assert len(lines) == 1 and 'nan' in lines[0] and 'fades in' in lines[0]
    assert np.isnan(L.last_metrics['generator']['ppl']['ppl'])
