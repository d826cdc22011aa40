"""GPU tests of the fused arena optimisers beside Adam (csrc/optim.hip through ``ops.rmsprop_step`` / ``sgd_step`` / ``oadam_step``
and their ``_dev`` forms; ``optim.FusedRMSprop`` / ``FusedSGD`` / ``FusedOptimisticAdam``; both learners; graphs.GraphedStep) against
the float64 restatements of tests/optim_reference.py.

Every bound is a count of fp32 roundings on quantities of the float64 run, written out at the reference functions; what the
tests would catch is shown on the CPU in tests/test_optim_host.py.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import optim_reference as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 4100)        # below one 16-byte vector, exactly one, a scalar tail, several workgroups with a tail
LR, EPS = 1e-3, 1e-8
CONFIGS = [('rmsprop', dict(lr=LR, alpha=0.99, eps=EPS, wd=0.0, momentum=0.0)),
           ('rmsprop', dict(lr=LR, alpha=0.9, eps=EPS, wd=1e-2, momentum=0.9)),
           ('sgd', dict(lr=LR, wd=0.0, momentum=0.0)),
           ('sgd', dict(lr=LR, wd=1e-2, momentum=0.9)),
           ('oadam', dict(lr=LR, b1=0.0, b2=0.99, eps=EPS, wd=0.0)),
           ('oadam', dict(lr=LR, b1=0.5, b2=0.999, eps=EPS, wd=1e-2))]
IDS = [f'{k}-{i % 2}' for i, (k, _) in enumerate(CONFIGS)]


def _gpu(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda()


def _f64(t):
    return t.detach().double().cpu().numpy()


def _live(kind, hp):
    """The state buffers this configuration reads (RMSprop / SGD without momentum have no ``buf``)."""
    return tuple(k for k in ref.STATE[kind] if not (k == 'buf' and hp['momentum'] == 0))


def _stale_buf(kind, n):
    """SGD starts from a momentum buffer full of stale values: the first step must replace it, not update it."""
    return dict(buf=np.random.default_rng(n).standard_normal(n).astype(np.float32)) if kind == 'sgd' else None


def _gpu_run(kind, n, steps, hp, dev_block=None):
    """``steps`` steps of the op (or of its ``_dev`` form, the scalars in floats 3..5 of ``dev_block``) -> dict of tensors."""
    from gan_lab_amd import ops
    p0, grads = ref.inputs(n)
    live = _live(kind, hp)
    st = {k: torch.zeros(n, device='cuda') for k in live}
    for k, v in (_stale_buf(kind, n) or {}).items():
        if k in st:
            st[k] = _gpu(v)
    p = _gpu(p0)
    for t, g in enumerate(grads[:steps], 1):
        g = _gpu(g)
        if kind == 'oadam':
            scal = [hp['lr'], 1 - hp['b1'] ** t, 1 - hp['b2'] ** t]
        elif kind == 'sgd':
            scal = [hp['lr'], 1.0 if t == 1 else 0.0, 0.0]
        else:
            scal = [hp['lr'], 0.0, 0.0]
        if dev_block is not None:
            ops.set_step_scalars(dev_block, 0, [7.0, 8.0, 9.0] + scal)
            at = dev_block.data_ptr() + 28
        if kind == 'rmsprop':
            rest = (hp['alpha'], hp['eps'], hp['wd'], hp['momentum'])
            if dev_block is None:
                ops.rmsprop_step(p, g, st['sq'], st.get('buf'), hp['lr'], *rest)
            else:
                ops.rmsprop_step_dev(p, g, st['sq'], st.get('buf'), at, *rest)
        elif kind == 'sgd':
            if dev_block is None:
                ops.sgd_step(p, g, st.get('buf'), hp['lr'], hp['wd'], hp['momentum'], t == 1)
            else:
                ops.sgd_step_dev(p, g, st.get('buf'), at, hp['wd'], hp['momentum'])
        else:
            rest = (hp['b1'], hp['b2'], hp['eps'], hp['wd'])
            if dev_block is None:
                ops.oadam_step(p, g, st['m'], st['v'], st['prev'], hp['lr'], *rest, scal[1], scal[2])
            else:
                ops.oadam_step_dev(p, g, st['m'], st['v'], st['prev'], at, *rest)
    return dict(st, p=p)


def _ref_run(kind, n, steps, hp, dtype=np.float64):
    p0, grads = ref.inputs(n)
    return ref.run(kind, p0, grads[:steps], dtype=dtype, state=_stale_buf(kind, n), **hp)


@pytest.mark.parametrize('kind,hp', CONFIGS, ids=IDS)
def test_steps_against_float64(kind, hp):
    """One step and 8 steps of each kernel at every size; gradients hold exact zeros and entries near 1e-12, every state starts at
    zero (SGD's buffer at stale values that step 1 must replace).

    The absolute bound is the forward error analysis written at ``optim_reference.*_reference``, carried through the recurrence.
    Roundings counted per step (u = 2^-24 each):
      g' = g + wd p                     2   (product, sum; none with wd = 0)
      rmsprop: sq'                      4   (1 - alpha, g'^2, its product, the sum; alpha sq: 1 + the same sum)
               den = sqrt(sq') + eps    3   (root allowed one ulp = 2 u, sum)
               d = g' / den             2   (quotient allowed one ulp)
               buf' = mom buf + d       2   (product, sum)
               p' = p - lr x            2   (product, difference)                          15 with momentum and weight decay
      sgd:     buf' = mom buf + g'      2,  p' = p - lr buf'  2                              6 with momentum and weight decay
      oadam:   m' 3, v' 4 as Adam's;  den = sqrt(v') rsqrt(bc2) + eps  6 (root 2, rsqrt 2, product, sum);
               d = (m' / bc1) / den     4   (two quotients);  p' = p - (2 lr d - lr prev)   6 (2 lr, its product with d, lr prev,
               the inner difference: 3 + 2 on the terms, 1 on p')                           25 with weight decay
    FMA contraction only removes roundings.

    Over 8 steps the HIP error is also set against the error of the float32 restatement on the CPU, both measured from float64 in
    units of the per-step bound (the bound of the last step alone, from exact inputs).  The two evaluations round differently
    (contraction, the root and quotient forms), so element by element their errors are unrelated; what is comparable is the worst
    error over all elements of all sizes: worst HIP <= 2 x worst CPU + 1 per-step bound.
    Measured: see DESIGN.md 4.24."""
    worst = {'hip': 0.0, 'cpu': 0.0}
    for n in SIZES:
        for steps in (1, 8):
            want, err, local = _ref_run(kind, n, steps, hp)
            got = _gpu_run(kind, n, steps, hp)
            cpu, _, _ = _ref_run(kind, n, steps, hp, np.float32) if steps == 8 else (None, None, None)
            for k in ('p',) + _live(kind, hp):
                g = _f64(got[k])
                assert g.shape == want[k].shape and np.isfinite(g).all(), (k, n, steps)
                e = np.abs(g - want[k])
                ratio = np.where(e > 0, e / np.maximum(err[k], 1e-300), 0.0).max()
                print(f'{kind} n={n} steps={steps} {k}: max error {e.max():.3e}, worst error / bound {ratio:.3f}')
                assert (e <= err[k]).all(), (k, n, steps, float(ratio))
                if steps == 8:
                    unit = np.maximum(local[k], 1e-300)
                    ec = np.abs(cpu[k].astype(np.float64) - want[k])
                    worst['hip'] = max(worst['hip'], np.where(e > 0, e / unit, 0.0).max())
                    worst['cpu'] = max(worst['cpu'], np.where(ec > 0, ec / unit, 0.0).max())
            if steps == 8 and n >= 1023:
                p0, _ = ref.inputs(n)
                assert np.abs(want['p'] - p0).max() > 1e-4               # the steps moved the parameters
                zero_g = np.array([i for i in range(5, n, 7) if i % 11 != 3])    # (3 mod 11 holds the 1e-12 entries instead)
                if hp['wd'] == 0.0:                                      # zero gradient, no decay: the element never moves
                    assert np.array_equal(_f64(got['p'])[zero_g], p0.astype(np.float64)[zero_g])
    print(f'{kind}: worst error over 8 steps in per-step bounds: HIP {worst["hip"]:.3f}, CPU float32 {worst["cpu"]:.3f}, '
          f'ratio {worst["hip"] / max(worst["cpu"], 1e-300):.3f}')
    assert worst['hip'] <= 2 * worst['cpu'] + 1


@pytest.mark.parametrize('kind,hp', CONFIGS, ids=IDS)
def test_dev_forms_are_bitwise_the_host_scalar_forms(kind, hp):
    """The per-step scalars read from floats 3..5 of the step-scalar block (where graphs.GraphedStep keeps the generator's): lr for
    all three, (bc1, bc2) for oadam, ``first`` in slot 1 for SGD.  Two runs of the host form are bitwise equal too."""
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    for n in (1, 5, 4100):
        a, b, c = _gpu_run(kind, n, 5, hp), _gpu_run(kind, n, 5, hp, dev_block=block), _gpu_run(kind, n, 5, hp)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, n)
            assert torch.equal(a[k], c[k]), (k, n)


def test_unaligned_operands_take_the_scalar_path_and_agree():
    """A view that starts 4 bytes into its buffer is not 16-byte aligned: the launch walks it element by element, with the same
    result bit for bit."""
    from gan_lab_amd import ops
    n = 1023
    p0, grads = ref.inputs(n)
    outs = []
    for shift in (0, 1):
        bufs = [torch.zeros(n + 4, device='cuda') for _ in range(8)]
        p, g, m, v, prev, sq, rbuf, sbuf = (b[shift:shift + n] for b in bufs)
        p.copy_(_gpu(p0))
        g.copy_(_gpu(grads[0]))
        ops.oadam_step(p, g, m, v, prev, LR, 0.5, 0.999, EPS, 1e-2, 0.5, 0.001)
        ops.rmsprop_step(p, g, sq, rbuf, LR, 0.9, EPS, 1e-2, 0.9)
        ops.sgd_step(p, g, sbuf, LR, 1e-2, 0.9, False)
        outs.append([t.clone() for t in (p, m, v, prev, sq, rbuf, sbuf)])
        assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in outs[-1])
        for b in bufs:                                              # nothing outside the view was written
            assert float(b[:shift].abs().sum()) == 0 and float(b[shift + n:].abs().sum()) == 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_ops_reject_bad_operands():
    """The operand checks of ``_adam_operands`` (fp32, contiguous, on the GPU, equal numel) before the library is called; a null
    ``buf`` is None and is allowed exactly when momentum is 0."""
    from gan_lab_amd import ops
    ok = lambda n=8: torch.zeros(n, device='cuda')          # noqa: E731
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    ops.set_step_scalars(block, 0, [LR, 0.5, 0.1, LR, 0.5, 0.1])
    at = block.data_ptr() + 16
    bad_ops = [(torch.zeros(8), TypeError), (torch.zeros(8, device='cuda', dtype=torch.float64), TypeError),
               (np.zeros(8, dtype=np.float32), TypeError), (torch.zeros(16, device='cuda')[::2], ValueError), (ok(9), ValueError)]
    calls = [(4, lambda a: ops.rmsprop_step(*a, LR, 0.9, EPS, 0.0, 0.9)), (4, lambda a: ops.rmsprop_step_dev(*a, at, 0.9, EPS, 0.0, 0.9)),
             (3, lambda a: ops.sgd_step(*a, LR, 0.0, 0.9, True)), (3, lambda a: ops.sgd_step_dev(*a, at, 0.0, 0.9)),
             (5, lambda a: ops.oadam_step(*a, LR, 0.5, 0.9, EPS, 0.0, 0.5, 0.1)), (5, lambda a: ops.oadam_step_dev(*a, at, 0.5, 0.9, EPS, 0.0))]
    for count, call in calls:
        for slot in range(count):
            for bad, exc in bad_ops:
                args = [ok() for _ in range(count)]
                args[slot] = bad
                with pytest.raises(exc):
                    call(args)
        call([ok() for _ in range(count)])                          # the accepted form runs
    for bad in (None, 0, -4, 1.5, block):
        with pytest.raises(TypeError):
            ops.oadam_step_dev(ok(), ok(), ok(), ok(), ok(), bad, 0.5, 0.9, EPS, 0.0)
        with pytest.raises(TypeError):
            ops.sgd_step_dev(ok(), ok(), None, bad, 0.0, 0.0)
        with pytest.raises(TypeError):
            ops.rmsprop_step_dev(ok(), ok(), ok(), None, bad, 0.9, EPS, 0.0, 0.0)
    with pytest.raises(TypeError, match='momentum buffer'):
        ops.rmsprop_step(ok(), ok(), ok(), None, LR, 0.9, EPS, 0.0, 0.9)
    with pytest.raises(TypeError, match='momentum buffer'):
        ops.sgd_step(ok(), ok(), None, LR, 0.0, 0.9, True)
    with pytest.raises(ValueError, match='momentum'):
        ops.sgd_step(ok(), ok(), ok(), LR, 0.0, -0.5, True)
    ops.rmsprop_step(ok(), ok(), ok(), None, LR, 0.9, EPS, 0.0, 0.0)
    ops.sgd_step(ok(), ok(), None, LR, 0.0, 0.0, True)


# ---- the optimiser classes over an arena -----------------------------------------------------------------------------------------
def _make(name, params, lr=LR):
    from gan_lab_amd import optim
    if name == 'rmsprop':
        return optim.FusedRMSprop(params, lr=lr, alpha=0.9, eps=EPS, weight_decay=1e-2, momentum=0.9)
    if name == 'sgd':
        return optim.FusedSGD(params, lr=lr, momentum=0.9, weight_decay=1e-2)
    return optim.FusedOptimisticAdam(params, lr=lr, betas=(0.5, 0.999), eps=EPS, weight_decay=1e-2)


HP = {'rmsprop': CONFIGS[1][1], 'sgd': CONFIGS[3][1], 'oadam': CONFIGS[5][1]}


def _arena(seed=3):
    from gan_lab_amd.optim import ParamArena
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in (5, 8, 3)]
    named = list(zip('abc', params))
    return ParamArena(named, 'cuda'), named


def _fill_grads(arena, step, seed=11):
    g = torch.Generator().manual_seed(seed + step)
    for p in arena.params:
        p.grad.copy_(torch.randn(p.shape, generator=g).cuda())


@pytest.mark.parametrize('name', ['rmsprop', 'sgd', 'oadam'])
def test_arena_one_launch_padding_relayout_and_moments(name):
    """Three parameters of 5, 8 and 3 floats in one arena (offsets 0, 8, 16; floats 5..7 and 19 are padding): one launch per
    step, the padding stays zero in parameters and every state buffer, the parameters follow the float64 restatement, a re-layout
    (one parameter dropped, the arena rebuilt) carries every state buffer, and export -> import reproduces the next step bit for
    bit."""
    from gan_lab_amd import _lib
    from gan_lab_amd.optim import ParamArena
    arena, named = _arena()
    assert arena.total == 20 and arena.offsets == [0, 8, 16]
    pad = torch.tensor([5, 6, 7, 19], device='cuda')
    opt = _make(name, arena.params)
    start = arena.flat.clone()
    grads = []
    for step in range(3):
        _fill_grads(arena, step)
        grads.append(arena.gflat.clone())
        c0 = _lib.launch_count()
        opt.step()
        launched = _lib.launches_since(c0)
        assert len(launched) == 1 and 'optim_kernel' in launched[0][0], launched
        assert float(arena.flat[pad].abs().max()) == 0 and float(arena.gflat[pad].abs().max()) == 0
    run0 = opt.state['_fused'][id(opt.param_groups[0])]['runs']
    assert len(run0) == 1 and run0[0]['n'] == 19                     # the run ends with the last parameter's last float
    for key, _ in opt.STATE:
        assert float(run0[0][key][pad[:3]].abs().max()) == 0 and float(run0[0][key].abs().max()) > 0
    want, err, _ = ref.run(name, _f64(start), [_f64(g).astype(np.float32) for g in grads], **HP[name])
    e = np.abs(_f64(arena.flat) - want['p'])
    print(f'{name}: arena parameters after 3 steps: worst error / bound {np.where(e > 0, e / np.maximum(err["p"], 1e-300), 0).max():.3f}')
    assert (e <= err['p']).all()
    # export -> import into a fresh optimiser over the same arena: the next step is the same, bit for bit
    saved = opt.export_moments(named)
    assert saved['step'] == 3 and all(set(saved[ck]) == {'a', 'b', 'c'} for _, ck in opt.STATE)
    before = arena.flat.clone()
    _fill_grads(arena, 3)
    opt.step()
    after_a = arena.flat.clone()
    state_a = {key: run0[0][key].clone() for key, _ in opt.STATE}
    arena.flat.copy_(before)
    fresh = _make(name, arena.params)
    fresh.import_moments(named, saved)
    fresh.step()
    assert torch.equal(arena.flat, after_a)
    run1 = fresh.state['_fused'][id(fresh.param_groups[0])]['runs'][0]
    for key, _ in opt.STATE:
        assert torch.equal(run1[key], state_a[key]), key
    assert fresh.export_moments(named)['step'] == 4
    # re-layout: drop 'b', rebuild the arena over the survivors - the same optimiser object carries their state
    keep = [named[0], named[2]]
    old = {k: {key: run0[0][key][run0[0]['offs'][id(p)]:run0[0]['offs'][id(p)] + p.numel()].clone() for key, _ in opt.STATE}
           for k, p in keep}
    opt.param_groups[0]['params'] = [p for _, p in keep]
    small = ParamArena(keep, 'cuda')
    assert small.total == 12
    small.gflat.zero_()
    opt_state_before = {k: {key: v.clone() for key, v in d.items()} for k, d in old.items()}
    _fill_grads(small, 9)
    g_small = small.gflat.clone()
    p_small = small.flat.clone()
    opt.step()
    run2 = opt.state['_fused'][id(opt.param_groups[0])]['runs']
    assert len(run2) == 1 and run2[0]['n'] == 11 and opt.export_moments(keep)['step'] == 5
    # the step after the re-layout equals the restatement started from the carried state
    state = {key: np.zeros(12) for key, _ in opt.STATE}
    for (k, p), off in zip(keep, small.offsets):
        for key, _ in opt.STATE:
            state[key][off:off + p.numel()] = _f64(opt_state_before[k][key])
    h = {k: ref.f32(v) for k, v in HP[name].items()}
    if name == 'rmsprop':
        out = ref.rmsprop_reference(_f64(p_small), _f64(g_small), state['sq'], state['buf'], h['lr'], h['alpha'], h['eps'], h['wd'],
                                    h['momentum'])
    elif name == 'sgd':
        out = ref.sgd_reference(_f64(p_small), _f64(g_small), state['buf'], h['lr'], h['wd'], h['momentum'], False)
    else:
        out = ref.oadam_reference(_f64(p_small), _f64(g_small), state['m'], state['v'], state['prev'], h['lr'], h['b1'], h['b2'],
                                  h['eps'], h['wd'], ref.f32(1 - HP[name]['b1'] ** 5), ref.f32(1 - HP[name]['b2'] ** 5))
    got = _f64(small.flat)
    moved = np.abs(got - _f64(p_small)).max()
    e = np.abs(got - out[0]).max()
    print(f'{name}: step after the re-layout: moved {moved:.3e}, error {e:.3e}')
    assert moved > 1e-4 and e <= 1e-3 * moved             # a lost buffer changes the step by its own size (momentum 0.9, 4 steps of state)
    assert float(small.flat[torch.tensor([5, 6, 7, 11], device='cuda')].abs().max()) == 0


# ---- learners --------------------------------------------------------------------------------------------------------------------
def _resnet_learner(name, seed=7):
    from util import load_golden
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    gold = load_golden('resnet32.npz')          # the width, latent length and batch of test_gpu_resnet's own step checks
    cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      num_iters_save_model=10 ** 9, log_every=0, len_latent=int(gold['len_latent']), lr_base=LR, random_seed=seed,
                      optimizer=name, momentum=0.9, rmsprop_momentum=0.9, wd=1e-2, beta1=0.5)
    cfg.fmap_g, cfg.fmap_d = int(gold['fmap_g']), int(gold['fmap_d'])
    torch.manual_seed(seed)
    L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    return L


def _learner_hp(name, c):
    if name == 'rmsprop':
        return 'rmsprop', dict(lr=c.lr_base, alpha=c.beta2, eps=c.eps, wd=c.wd, momentum=c.rmsprop_momentum)
    if name in ('momentum', 'sgd'):
        return 'sgd', dict(lr=c.lr_base, wd=c.wd, momentum=c.momentum if name == 'momentum' else 0.0)
    return 'oadam', dict(lr=c.lr_base, b1=c.beta1, b2=c.beta2, eps=c.eps, wd=c.wd)


def _two_iterations(L, name, reals):
    """Two ``d_step`` + ``g_step`` iterations; the arena gradients each optimiser step consumed are fed to the float64 restatement
    from the initial parameters, and the learner's parameters must lie within the restatement's fp32 bound."""
    kind, hp = _learner_hp(name, L.config)
    start = {'d': _f64(L.arena_d.flat), 'g': _f64(L.arena_g.flat)}
    grads = {'d': [], 'g': []}
    for x in reals:
        L.set_requires_grad_disc(True)
        L.d_step(x)
        grads['d'].append(_f64(L.arena_d.gflat).astype(np.float32))
        L.set_requires_grad_disc(False)
        L.g_step()
        grads['g'].append(_f64(L.arena_g.gflat).astype(np.float32))
    torch.cuda.synchronize()
    for net, arena, opt in (('d', L.arena_d, L.opt_disc), ('g', L.arena_g, L.opt_gen)):
        runs = opt.state['_fused'][id(opt.param_groups[0])]['runs']
        assert opt.export_moments([])['step'] == 2
        want, err, _ = ref.run(kind, start[net], grads[net], **hp)
        got = _f64(arena.flat)
        covered = np.zeros(arena.total, dtype=bool)
        for r in runs:                                               # parameters outside every run (no gradient) must not move
            o = (r['start'] - arena.flat.data_ptr()) // 4
            covered[o:o + r['n']] = True
        e = np.abs(got - want['p'])
        ratio = np.where(e > 0, e / np.maximum(err['p'], 1e-300), 0.0)
        moved = np.abs(got - start[net]).max()
        print(f'{name} {net}: {len(runs)} run(s), moved {moved:.3e}, worst error / bound {ratio[covered].max():.3f}')
        assert moved > 1e-5 and (e[covered] <= err['p'][covered]).all()
        assert np.array_equal(got[~covered], start[net][~covered])


@pytest.mark.parametrize('name', ['rmsprop', 'momentum', 'sgd', 'oadam'])
def test_resnet_learner_steps_follow_the_restatement(name):
    L = _resnet_learner(name)
    g = torch.Generator().manual_seed(5)
    _two_iterations(L, name, [(torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).cuda() for _ in range(2)])


def _stylegan_learner(res, name, seed=21, **kw):
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    cfg = make_config('stylegan', dev='cuda', pin_memory=False, res_samples=res, res_dataset=res, init_res=res, batch_size=4,
                      len_latent=16, len_dlatent=16, mapping_num_fcs=2, cutoff_trunc_trick=None, nimg_transition=24,
                      num_iters_save_model=10 ** 9, log_every=0, random_seed=seed, loss='nonsaturating', gradient_penalty='r1',
                      optimizer=name, **kw)
    L = StyleGANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    L.beta = 0.99
    return L


def test_stylegan_learner_steps_follow_the_restatement():
    from gan_lab_amd import progressive as P
    P.FMAP_BASE, P.FMAP_MAX = 1024, 64
    try:
        torch.manual_seed(9)
        L = _stylegan_learner(8, 'rmsprop', rmsprop_momentum=0.5)
        g = torch.Generator().manual_seed(6)
        _two_iterations(L, 'rmsprop', [(torch.rand(4, 3, 8, 8, generator=g) * 2 - 1).cuda() for _ in range(2)])
    finally:
        P.FMAP_BASE, P.FMAP_MAX = 8192, 512


def test_graphed_step_equals_eager_under_rmsprop():
    """graphs.GraphedStep at the geometry of test_gpu_learner.test_graphed_step_equals_eager (StyleGAN, 32 pixels, batch 4): two
    eager warm-up iterations, then three replayed ones through ``ganlab_rmsprop_dev_f32``, against five eager iterations - parameters,
    every optimiser buffer, the EWMA generator and both losses bit for bit."""
    from gan_lab_amd import progressive as P, rng
    from gan_lab_amd.graphs import GraphedStep
    gen = torch.Generator().manual_seed(17)
    reals = [(torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(5)]

    def run(graphed):
        P.FMAP_BASE, P.FMAP_MAX = 1024, 64
        torch.manual_seed(9)
        np.random.seed(9)
        L = _stylegan_learner(32, 'rmsprop', rmsprop_momentum=0.5)
        torch.manual_seed(10)
        stepper = GraphedStep(L, warmup=2)
        losses = []
        for x in reals:
            if graphed:
                ld, lg = stepper(x)
            else:
                _, kw_d = stepper._mix_kwargs()
                ld = stepper._d_half(x, kw_d)
                _, kw_g = stepper._mix_kwargs()
                lg = stepper._g_half(kw_g)
            losses.append((float(ld), float(lg)))
        torch.cuda.synchronize()
        state = {'g': L.arena_g.flat.clone(), 'd': L.arena_d.flat.clone(), 'lag': L.ewma.flat.clone()}
        for tag, opt, model in (('og', L.opt_gen, L.gen_model), ('od', L.opt_disc, L.disc_model)):
            ex = opt.export_moments(list(model.named_parameters()))
            state[tag + '.step'] = torch.tensor(ex['step'])
            for ck in ('square_avg', 'momentum_buffer'):
                assert ex[ck]
                for k2, v in ex[ck].items():
                    state[f'{tag}.{ck}.{k2}'] = v
        return state, losses, (len(stepper.graphs) if graphed else 0), rng._STATE['offset']
    try:
        a, la, n_graphs, off_a = run(True)
        b, lb, _, off_b = run(False)
    finally:
        P.FMAP_BASE, P.FMAP_MAX = 8192, 512
    assert n_graphs >= 2, 'nothing was captured'
    assert off_a == off_b and la == lb
    assert int(a['og.step']) == int(b['og.step']) == 5
    for k in b:
        assert torch.equal(a[k], b[k]), k
