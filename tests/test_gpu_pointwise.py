"""GPU tests of the kernels every training run goes through (csrc/pointwise.hip; the draws of csrc/cond.hip and csrc/swd.hip)
against the float64 restatements of tests/pointwise_reference.py: the Philox stream element by element, the stream ledger of
gan_lab_amd/rng.py, Adam and the moving average, the scalar reductions and losses, the elementwise ops, and the Python guards
in front of the ops that take raw pointers.

Every bound is a count of fp32 roundings (u = 2^-24 each; FMA contraction only removes some) on quantities of the float64
reference, derived where it is used; every test prints ``worst error / bound`` per case before it asserts, and the figures
measured on the MI355X stand in the docstrings.  What each test would catch is shown on the CPU in
tests/test_pointwise_host.py by perturbing the reference."""
import math

import numpy as np
import pytest
import torch

import pointwise_reference as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEEDS = (0x5EED, 0x5A17ED0123456789)                     # the second has a non-zero high word
OFFSETS = (0, 12345, 2 ** 32 - 2, 2 ** 64 - 2)           # the counters carry into the high word / wrap to 0
GRID_CAP = 256 * 8 * 256                                 # threads of an elementwise launch: kMaxBlocks (csrc/pointwise.hip) x 256
RANDN_SIZES = (1, 3, 4, 5, 1023, 4099, 4 * GRID_CAP + 5)  # the last: a second trip of the grid-stride loop, with a tail
RANDN_BOUND = 8e-6


def _gpu(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda()


def _f64(t):
    return t.detach().double().cpu().numpy()


def _check(what, got, want, tol):
    """|got - want| <= tol elementwise (``tol`` an array or a number); prints the worst ratio first."""
    got, want = np.asarray(_f64(got) if isinstance(got, torch.Tensor) else got, dtype=np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err, tol = np.abs(got - want), np.broadcast_to(np.asarray(tol, dtype=np.float64), want.shape)
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    print(f'{what}: max error {err.max():.3e}, worst error / bound {ratio.max():.3f}')
    assert (err <= tol).all(), (what, float(err.max()), float(ratio.max()))
    return float(ratio.max())


# =============================================================================================================================== #
# the stream
# =============================================================================================================================== #
@pytest.mark.parametrize('offset', OFFSETS, ids=['0', '12345', '2p32m2', '2p64m2'])
@pytest.mark.parametrize('seed', SEEDS, ids=['lowseed', 'highseed'])
def test_randn_against_the_restated_stream(seed, offset):
    """Element 4i + 2k = rad cos, 4i + 2k + 1 = rad sin of words (2k, 2k + 1) of counter offset + i, |z - ref| <= 8e-6.
    Where the bound comes from: the fp32 angle 2 pi u2 carries at most 2^-24 2 pi = 3.7e-7 of rounding plus the fp32
    constant's 1.8e-7 (u2 <= 1); times rad <= sqrt(64 ln 2) = 6.66 that is 3.7e-6.  logf is good to an ulp of |ln u1| <= 22.2
    (1.9e-6), doubled and passed through the square root (1 / (2 rad)) it gives 2.9e-7 at the largest rad and at most 1e-6
    near rad = 0.35, below which the ulp of |ln u1| shrinks faster than rad; sqrtf, sincosf and the product add three
    ulps of rad, 1.2e-6.  Together below 6e-6.  Any mapping error - a swapped pair, a wrong word, a dropped counter word, a
    lost tail - is of order 1 (test_pointwise_host.test_randn_perturbations_are_far_outside_the_bound).
    Measured on the MI355X: 1.83e-6, the largest over all seeds, offsets and sizes."""
    from gan_lab_amd import ops
    n_big = RANDN_SIZES[-1]
    want = ref.randn_reference(seed, offset, n_big)
    worst = 0.0
    for n in RANDN_SIZES:
        got = ops.randn((n,), seed, offset, 'cuda')
        assert got.shape == (n,) and got.dtype == torch.float32
        err = np.abs(_f64(got) - want[:n]).max()
        worst = max(worst, err)
        print(f'seed {seed:#x} offset {offset} n={n}: max |z - ref| {err:.3e} (bound {RANDN_BOUND:.1e})')
    assert worst <= RANDN_BOUND


def test_randn_bitwise_properties():
    """A shorter draw is the prefix of a longer one; one counter on is four elements on; two runs agree; shapes only reshape."""
    from gan_lab_amd import ops
    for seed in SEEDS:
        for offset in OFFSETS:
            full = ops.randn((4099,), seed, offset, 'cuda')
            for n in (1, 3, 4, 5, 1023):
                assert torch.equal(ops.randn((n,), seed, offset, 'cuda'), full[:n]), (seed, offset, n)
            assert torch.equal(ops.randn((4095,), seed, (offset + 1) & ref.M64, 'cuda'), full[4:])
            assert torch.equal(ops.randn((4099,), seed, offset, 'cuda'), full)
            assert torch.equal(ops.randn((3, 5, 7), seed, offset, 'cuda').reshape(-1), full[:105])
    big = ops.randn((4 * GRID_CAP + 5,), SEEDS[1], 7, 'cuda')
    assert torch.equal(big[:4099], ops.randn((4099,), SEEDS[1], 7, 'cuda'))
    assert torch.equal(big[4 * GRID_CAP:], ops.randn((5,), SEEDS[1], 7 + GRID_CAP, 'cuda'))


@pytest.mark.parametrize('base', [1000, 2 ** 32 - 3, 2 ** 40 + 17, 2 ** 64 - 5], ids=['1000', '2p32m3', '2p40', '2p64m5'])
def test_randn_dev_equals_randn_at_base_plus_delta(base):
    from gan_lab_amd import ops
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    ops.set_step_scalars(block, base, [0.25, 0.5, 0.75])
    assert block.cpu().view(torch.int64)[0].item() == (base if base < 2 ** 63 else base - 2 ** 64)
    assert block.cpu().view(torch.float32)[4:10].tolist() == [0.25, 0.5, 0.75, 0.0, 0.0, 0.0]
    for delta in (0, 1, 5, 2 ** 20):
        for n in (1, 5, 4099):
            got = ops.randn_dev((n,), SEEDS[1], block, delta, 'cuda')
            assert torch.equal(got, ops.randn((n,), SEEDS[1], (base + delta) & ref.M64, 'cuda')), (base, delta, n)


@pytest.mark.parametrize('high', [1, 3, 1000, 2 ** 24])
def test_randint_against_the_restated_stream(high):
    from gan_lab_amd import ops
    for seed, offset in ((SEEDS[0], 0), (SEEDS[1], 2 ** 32 - 2), (SEEDS[1], 2 ** 64 - 2)):
        for n in (1, 5, 64, 1027):
            got = ops.randint(n, high, seed, offset, 'cuda')
            assert got.dtype == torch.int32 and got.shape == (n,)
            assert np.array_equal(got.cpu().numpy().astype(np.int64), ref.randint_reference(seed, offset, n, high)), (n, offset)


@pytest.mark.parametrize('N,n,S', [(3, 5, 1024), (7, 128, 16), (1, 1, 8)])
def test_swd_positions_against_the_restated_stream(N, n, S):
    from gan_lab_amd import ops
    for seed, offset in ((SEEDS[0], 0), (SEEDS[1], 2 ** 32 - 2), (SEEDS[1], 2 ** 64 - 2)):
        got = ops.swd_positions(N, n, S, seed, offset, 'cuda')
        assert got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy().astype(np.int64), ref.swd_positions_reference(seed, offset, N, n, S)), offset


@pytest.mark.parametrize('n_dirs', [1, 3, 130])
def test_swd_directions_against_the_restated_stream(n_dirs):
    """The kernel computes in fp64 and rounds once: |d - ref| <= 2^-23 |ref| per element (one fp32 rounding, 2^-24, and as
    much again for the last bits of the two fp64 libms, which matter only when they move the rounding).
    Measured: worst error / bound 0.496 (one rounding)."""
    from gan_lab_amd import ops
    for seed, offset in ((SEEDS[0], 0), (SEEDS[1], 2 ** 32 - 100), (SEEDS[1], 2 ** 64 - 100)):
        want = ref.swd_directions_reference(seed, offset, n_dirs)
        _check(f'swd_directions {n_dirs} at {offset}', ops.swd_directions(n_dirs, seed, offset, 'cuda'), want,
               2.0 ** -23 * np.abs(want))


def _ledger_sequence(state, mask):
    """(name, arguments of rng.name, arguments of ops.name before (seed, offset, device), arguments of CONSUMED[name])."""
    return [
        ('randn', ((3,),), ((3,),), (3,)),
        ('randn', ((5, 7),), ((5, 7),), (35,)),
        ('trunc_randn', ((3, 3), 0.8), ((3, 3), 0.8), (9,)),
        ('randint', (5, 10), (5, 10), (5,)),
        ('augment_params', (3, 32, 32), (3, 32, 32), (3,)),
        ('ada_params', (2, 32, 32, state, mask), (2, 32, 32, state, mask), (2,)),
        ('randn', ((1,),), ((1,),), (1,)),
        ('swd_positions', (3, 5, 64), (3, 5, 64), (3, 5)),
        ('swd_directions', (2,), (2,), (2,)),
        ('randint', (1, 3), (1, 3), (1,)),
        ('randn', ((2, 3, 11),), ((2, 3, 11),), (66,)),
    ]


_OPS_NAME = {'augment_params': 'diffaug_params'}


def test_stream_ledger_matches_what_the_kernels_consume():
    """One mixed sequence through ``rng.*``: every result is the direct ``ops.*`` call at the cumulative offset, bit for bit;
    every advance is the number of counters the restated draw reads, so the counters of a draw and of the next one at
    ``offset + count`` are disjoint sets; the restated consumers (randn, randint, swd_positions, swd_directions) reproduce
    the draw from exactly those counters.  The same sequence by device-resident offsets (``begin_device_offsets``; randn
    and augment_params only) gives the same tensors and the same advance."""
    from gan_lab_amd import ada, ops, rng
    saved = dict(rng._STATE)
    state = torch.tensor([0.6, 0, 0, 0], dtype=torch.float32, device='cuda')
    mask = ada.parse_policy('blit,geom,color')
    try:
        for start in (0, 2 ** 32 - 9):
            rng.manual_seed(31337)
            rng._STATE['offset'] = start
            seed, offset, eager = rng._STATE['seed'], start, []
            for name, rng_args, ops_args, count_args in _ledger_sequence(state, mask):
                out = getattr(rng, name)(*rng_args)
                count = rng._STATE['offset'] - offset
                direct = getattr(ops, _OPS_NAME.get(name, name))(*ops_args, seed, offset, 'cuda')
                assert torch.equal(out, direct), (name, offset)
                assert count == ref.CONSUMED[name](*count_args), (name, count)
                here, there = ref.counter_range(offset, count), ref.counter_range(offset + count, count)
                assert len(here) == count and not (here & there) and max(here) == offset + count - 1
                if name == 'randn':
                    n = int(np.prod(rng_args[0]))
                    assert np.abs(_f64(out).reshape(-1) - ref.randn_reference(seed, offset, n)).max() <= RANDN_BOUND
                    # the draw right behind it starts on the next counter: it shares no word with this draw's last group
                    nxt = ops.randn((4,), seed, offset + count, 'cuda')
                    assert np.abs(_f64(nxt) - ref.randn_reference(seed, offset + count, 4)).max() <= RANDN_BOUND
                elif name == 'randint':
                    assert np.array_equal(out.cpu().numpy(), ref.randint_reference(seed, offset, *rng_args))
                elif name == 'swd_positions':
                    assert np.array_equal(out.cpu().numpy(), ref.swd_positions_reference(seed, offset, *rng_args))
                elif name == 'swd_directions':
                    want = ref.swd_directions_reference(seed, offset, *rng_args)
                    assert (np.abs(_f64(out) - want) <= 2.0 ** -23 * np.abs(want)).all()
                eager.append((name, out))
                offset += count
            total = offset - start

            # device-resident offsets: the step-graph form
            rng.manual_seed(31337)
            rng._STATE['offset'] = start
            block = torch.zeros(16, dtype=torch.int32, device='cuda')
            ops.set_step_scalars(block, start, [])
            rng.begin_device_offsets(block)
            try:
                dev, want_adv = [], 0
                for name, rng_args, _, count_args in _ledger_sequence(state, mask):
                    if name in ('randn', 'augment_params'):
                        dev.append((name, getattr(rng, name)(*rng_args)))
                        want_adv += ref.CONSUMED[name](*count_args)
                for name, args in (('trunc_randn', ((4,), 0.5)), ('randint', (4, 3)), ('swd_positions', (1, 1, 8)),
                                   ('swd_directions', (1,))):
                    with pytest.raises(RuntimeError):
                        getattr(rng, name)(*args)
            finally:
                adv = rng.end_device_offsets()
            assert adv == want_adv == rng._STATE['offset'] - start
            # the same draws, eagerly, back to back from the same start
            rng.manual_seed(31337)
            rng._STATE['offset'] = start
            rng._STATE['offset'] = start
            it = iter(dev)
            for name, rng_args, _, _ in _ledger_sequence(state, mask):
                if name in ('randn', 'augment_params'):
                    nm, got = next(it)
                    assert nm == name and torch.equal(got, getattr(rng, name)(*rng_args)), name
            assert rng._STATE['offset'] - start == adv < total
    finally:
        rng._DEVICE_BASE['block'] = None
        rng._STATE.update(saved)


# =============================================================================================================================== #
# optimiser
# =============================================================================================================================== #
ADAM_CONFIGS = [(0.0, 0.99, 0.0), (0.5, 0.999, 0.0), (0.9, 0.999, 1e-2)]
ADAM_SIZES = (1, 1000, 4097, GRID_CAP + 5)
LR, EPS = 1e-3, 1e-8


def _adam_gpu(n, b1, b2, wd, dev_block=None):
    """Five steps of ops.adam_step (or adam_step_dev with the scalars in ``dev_block``) at tests' inputs -> p, m, v."""
    from gan_lab_amd import ops
    p0, grads = ref.adam_inputs(n)
    p, m, v = _gpu(p0), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    for t, g in enumerate(grads, 1):
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        if dev_block is None:
            ops.adam_step(p, _gpu(g), m, v, LR, b1, b2, EPS, wd, bc1, bc2)
        else:
            ops.set_step_scalars(dev_block, 0, [7.0, 8.0, 9.0, LR, bc1, bc2])
            ops.adam_step_dev(p, _gpu(g), m, v, dev_block.data_ptr() + 28, b1, b2, EPS, wd)
    return p, m, v


@pytest.mark.parametrize('n', ADAM_SIZES)
@pytest.mark.parametrize('b1,b2,wd', ADAM_CONFIGS)
def test_adam_step_against_float64(b1, b2, wd, n):
    """Five steps; p, m and v against ``pointwise_reference.adam_run``, whose bound is the forward error analysis written at
    ``adam_reference``: a few u per operation, carried through the recurrence (linear in the number of steps: tens of ulps of
    |p| after five).  Gradients hold exact zeros and entries near 1e-12 (v ~ 1e-27: eps decides the step).  Swapped betas,
    swapped bias corrections and decoupled weight decay leave this bound by factors of 50 to 1e9
    (test_pointwise_host.test_adam_wrong_variants_leave_the_bound).
    Measured: worst error / bound 0.90 (p), 0.31 (m), 0.50 (v)."""
    p0, grads = ref.adam_inputs(n)
    want_p, want_m, want_v, err = ref.adam_run(p0, grads, LR, b1, b2, EPS, wd)
    p, m, v = _adam_gpu(n, b1, b2, wd)
    _check('p', p, want_p, err['p'])
    _check('m', m, want_m, err['m'])
    _check('v', v, want_v, err['v'])
    assert np.abs(want_p - p0).max() > 1e-4            # the steps moved the parameters


@pytest.mark.parametrize('b1,b2,wd', ADAM_CONFIGS)
def test_adam_step_dev_is_bitwise_adam_step(b1, b2, wd):
    """(lr, bc1, bc2) read from floats 3..5 of the step-scalar block (where graphs.GraphedStep keeps the generator's)."""
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    for n in (1, 4097, GRID_CAP + 5):
        for a, b in zip(_adam_gpu(n, b1, b2, wd), _adam_gpu(n, b1, b2, wd, dev_block=block)):
            assert torch.equal(a, b), n


@pytest.mark.parametrize('beta', [0.0, 0.999, 1.0])
def test_ewma_step_against_float64(beta):
    """lag' = p (1 - beta) + lag beta with beta as the kernel receives it: 1 - beta is one rounding, each product one, the sum
    one - u (2 |p (1 - beta)| + |lag beta|) + u |lag'|.  beta = 0 copies p and beta = 1 keeps lag, bit for bit.
    Measured: worst error / bound 0.97."""
    from gan_lab_amd import ops
    b = ref.f32(beta)
    for n in (1, 777, 4097):
        gen = np.random.default_rng(n)
        lag0, p0 = gen.standard_normal(n).astype(np.float32), (3 * gen.standard_normal(n)).astype(np.float32)
        lag, p = _gpu(lag0), _gpu(p0)
        ops.ewma_step(lag, p, beta)
        A, B = p0.astype(np.float64) * (1.0 - b), lag0.astype(np.float64) * b
        _check(f'ewma n={n} beta={beta}', lag, A + B, U * (2 * np.abs(A) + np.abs(B) + np.abs(A + B)))
        assert torch.equal(p, _gpu(p0))
        if beta in (0.0, 1.0):
            assert torch.equal(lag, _gpu(p0 if beta == 0.0 else lag0))


def test_raw_pointer_ops_reject_bad_operands():
    """ops.adam_step / adam_step_dev / ewma_step / randn / randn_dev check their operands in Python (ops._inplace,
    ops._same_numel, ops._gpu_device) before the library is called: nothing here reaches a kernel."""
    from gan_lab_amd import ops
    ok = lambda n=8: torch.zeros(n, device='cuda')          # noqa: E731
    block = torch.zeros(16, dtype=torch.int32, device='cuda')
    scal = (1e-3, 0.5, 0.999, 1e-8, 0.0)
    bad_type = [torch.zeros(8), torch.zeros(8, device='cuda', dtype=torch.float64), torch.zeros(8, device='cuda').half(),
                np.zeros(8, dtype=np.float32), None]
    strided = torch.zeros(16, device='cuda')[::2]
    for slot in range(4):
        for bad, exc in [(b, TypeError) for b in bad_type] + [(strided, ValueError), (ok(9), ValueError)]:
            args = [ok(), ok(), ok(), ok()]
            args[slot] = bad
            with pytest.raises(exc):
                ops.adam_step(*args, *scal, 0.5, 0.001)
            with pytest.raises(exc):
                ops.adam_step_dev(*args, block.data_ptr() + 16, *scal[1:])
    for bad in (None, 0, -4, 1.5, block):
        with pytest.raises(TypeError):
            ops.adam_step_dev(ok(), ok(), ok(), ok(), bad, *scal[1:])
    for slot in range(2):
        for bad, exc in [(b, TypeError) for b in bad_type] + [(strided, ValueError), (ok(9), ValueError)]:
            args = [ok(), ok()]
            args[slot] = bad
            with pytest.raises(exc):
                ops.ewma_step(*args, 0.9)
    for dev in ('cpu', torch.device('cpu')):
        with pytest.raises(TypeError):
            ops.randn((4,), 1, 0, dev)
        with pytest.raises(TypeError):
            ops.randn_dev((4,), 1, block, 0, dev)
    for bad in (None, 12345, torch.zeros(16, dtype=torch.int32)):
        with pytest.raises(TypeError):
            ops.randn_dev((4,), 1, bad, 0, 'cuda')
    for bad in (torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(32, dtype=torch.int32, device='cuda')[::2]):
        with pytest.raises(ValueError):
            ops.randn_dev((4,), 1, bad, 0, 'cuda')
    t = ok()                                                # the accepted forms still run
    ops.adam_step(t, ok(), ok(), ok(), *scal, 0.5, 0.001)
    ops.ewma_step(t, ok(), 0.9)
    assert ops.randn((4,), 1, 0, torch.device('cuda')).shape == (4,)


# =============================================================================================================================== #
# reductions and losses
# =============================================================================================================================== #
def _sum_terms(n):
    """(terms per thread, threads) of sum_stage1: sum_blocks(n) = min(1024, ceil(n / 4096)) blocks of 256 threads."""
    blocks = min(1024, max(1, -(-n // 4096)))
    return -(-n // (256 * blocks)), 256 * blocks


@pytest.mark.parametrize('n', [1, 255, 4097, 2 ** 22 + 3])
def test_sum_and_sumsq_against_float64(n):
    """Data with mean 1 (no cancellation).  A thread adds ceil(n / threads) terms in a chain; wave shuffles, the block's four
    partials, the second stage and the scale add a fixed number of levels: (terms per thread + 16) u sum |x| (sum x^2 for
    the squares, whose products are exact inside an FMA).  The backward is scale_dev: out = (a gout) x, 3 roundings with
    a = 2 scale, or the constant a gout (1 rounding: exact to u).
    Measured: worst error / bound 0.06 (forward), 0.49 (backward)."""
    from gan_lab_amd import ops
    gen = np.random.default_rng(n)
    x0 = (1.0 + 0.5 * gen.standard_normal(n)).astype(np.float32)
    x64 = x0.astype(np.float64)
    terms, _ = _sum_terms(n)
    scale, go = 0.37, 1.7
    s32 = ref.f32(scale)
    for squared in (False, True):
        x = _gpu(x0).requires_grad_(True)
        out = (ops.sumsq_all if squared else ops.sum_all)(x, scale)
        mag = (x64 * x64).sum() if squared else np.abs(x64).sum()
        _check(f'sum n={n} squared={squared}', out, s32 * ((x64 * x64).sum() if squared else x64.sum()),
               (terms + 16) * U * mag * s32)
        out.backward(torch.tensor(ref.f32(go), device='cuda'))
        if squared:
            k = ref.f32(2.0 * scale) * ref.f32(go)
            _check('  d sumsq', x.grad, k * x64, 3 * U * np.abs(k * x64))
        else:
            k = s32 * ref.f32(go)
            _check('  d sum', x.grad, np.full(n, k), U * abs(k))


def _logits(n, seed):
    gen = np.random.default_rng(seed)
    x = (3.0 * gen.standard_normal(n)).astype(np.float32)
    edge = np.array([0.0, 20.0, -20.0, 100.0, -100.0], dtype=np.float32)[:n]
    x[:edge.size] = edge
    return x


@pytest.mark.parametrize('target', [0.0, 1.0])
@pytest.mark.parametrize('n', [1, 8, 300])
def test_bce_logits_mean_against_float64(n, target):
    """Terms max(x, 0) - x t + log1p(exp(-|x|)): expf and log1pf a few ulps each, two sums - 8 u per term on
    |x| + log 2 >= its parts; a thread chains ceil(n / 256) terms, the block reduce adds 8 levels and the division one:
    (8 + ceil(n / 256) + 9) u mean(|x| + log 2).  Backward gout (sigmoid(x) - t) / n: sigmoid to 4 u of 1 (expf, sum,
    quotient), the difference exact or one rounding, product and quotient: 8 u |gout| / n absolute.
    Measured: worst error / bound 0.03 (forward), 0.24 (backward)."""
    from gan_lab_amd import ops
    x0 = _logits(n, 5 + n)
    x = _gpu(x0).requires_grad_(True)
    xr = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    want = ref.bce_logits_mean(xr, target)
    out = ops.bce_logits_mean(x, target)
    _check(f'bce n={n} t={target}', out, want.item(), (17 + -(-n // 256)) * U * (np.abs(x0.astype(np.float64)) + math.log(2)).mean())
    go = 1.3
    out.backward(torch.tensor(ref.f32(go), device='cuda'))
    want.backward(torch.tensor(ref.f32(go), dtype=torch.float64))
    _check('  d bce', x.grad, xr.grad.numpy(), 8 * U * ref.f32(go) / n)


@pytest.mark.parametrize('a,b', [(1.0, -1.0), (1.0, 1.0), (0.0, -1.0)])
@pytest.mark.parametrize('n', [1, 8, 300])
def test_hinge_mean_against_float64(n, a, b):
    """mean(relu(a + b x)) with entries exactly on the kink (gradient 0, as torch.relu).  Forward: one rounding per term
    (FMA), a chain of ceil(n / 256), 8 levels of block reduce, the division: (ceil(n / 256) + 10) u mean|a + b x|.  Backward
    gout b / n where a + b x > 0: two roundings.  Double backward towards gout: sum_i gg_i [a + b x_i > 0] b / n through
    mul and sum_all - 3 u per term and (chain + 16) u on the sum of magnitudes; towards x it is exactly 0.
    Measured: worst error / bound 0.08 (forward), 0.16 (backward), 0.02 (double backward)."""
    from gan_lab_amd import ops
    gen = np.random.default_rng(17 + n)
    x0 = (1.5 * gen.standard_normal(n)).astype(np.float32)
    kink = np.float32(-a / b)
    x0[::3] = kink                                    # n = 1: the only entry sits on the kink
    if n > 1:
        x0[1] = np.nextafter(kink, np.float32(10.0))  # one ulp to either side of it
    if n > 2:
        x0[2] = np.nextafter(kink, np.float32(-10.0))
    x = _gpu(x0).requires_grad_(True)
    xr = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    chain = -(-n // 256)
    want = ref.hinge_mean(xr, a, b)
    out = ops.hinge_mean(x, a, b)
    _check(f'hinge n={n} a={a} b={b}', out, want.item(), (chain + 10) * U * np.abs(a + b * x0.astype(np.float64)).mean())
    go = torch.tensor(ref.f32(0.7), device='cuda', requires_grad=True)
    gor = torch.tensor(ref.f32(0.7), dtype=torch.float64, requires_grad=True)
    gx, = torch.autograd.grad(out, x, go, create_graph=True)
    gxr, = torch.autograd.grad(want, xr, gor, create_graph=True)
    _check('  d hinge', gx, gxr.detach().numpy(), 2 * U * np.abs(gxr.detach().numpy()))
    assert (_f64(gx)[::3] == 0.0).all()
    w0 = gen.standard_normal(n).astype(np.float32)
    ggo, ggx = torch.autograd.grad((gx * _gpu(w0)).sum(), (go, x), allow_unused=True)
    ggor, = torch.autograd.grad((gxr * torch.tensor(w0, dtype=torch.float64)).sum(), gor)
    mag = np.abs(w0.astype(np.float64) * (gxr.detach().numpy() / ref.f32(0.7))).sum()
    _check('  dd hinge / d gout', ggo, ggor.item(), (3 + _sum_terms(n)[0] + 16) * U * mag)
    assert ggx is None or float(ggx.abs().max()) == 0.0


@pytest.mark.parametrize('shape', [(4, 3, 16, 16), (3, 5, 7, 9), (2, 1, 4, 4), (2, 3, 128, 128)])
def test_chnorm_penalty_against_float64(shape):
    """scale sum (||g||_2 - gamma)^2 over pixels, one of them an exactly zero vector (gradient 0).  Per pixel: q = sum of C
    squares (C u q), s = sqrt q (u more: e_s = (C / 2 + 1) u s), d = s - gamma (u |d| + e_s), d^2 (2 |d| e_d + u d^2); the
    pixel sums chain ceil(pixels / threads) terms plus 16 levels: + (chain + 16) u sum d^2.  Backward
    k g_c with k = 2 scale gout (s - gamma) / s: |g_c| (|2 scale gout| (e_s (1 + gamma / s) / s) + 6 u |k|).
    Measured: worst error / bound 0.04 (forward), 0.37 (backward)."""
    from gan_lab_amd import ops
    N, C, H, W = shape
    gen = np.random.default_rng(C * H + W)
    g0 = gen.standard_normal(shape).astype(np.float32)
    g0[N - 1, :, H // 2, W // 3] = 0.0
    gamma, scale, go = 1.0, 10.0 / 2 / (N * H * W), 0.9
    sc = ref.f32(scale)
    g = _gpu(g0).requires_grad_(True)
    gr = torch.tensor(g0, dtype=torch.float64, requires_grad=True)
    want = ref.chnorm_penalty(gr, gamma, sc)
    out = ops.chnorm_penalty(g, gamma, scale)
    g64 = g0.astype(np.float64)
    s = np.sqrt((g64 * g64).sum(axis=1))
    d = s - gamma
    e_s = (C / 2 + 1) * U * s
    e_d = U * np.abs(d) + e_s
    chain = _sum_terms(N * H * W)[0]
    tol = sc * ((2 * np.abs(d) * e_d + U * d * d + e_d * e_d).sum() + (chain + 16) * U * (d * d).sum())
    _check(f'chnorm {shape}', out, want.item(), tol)
    out.backward(torch.tensor(ref.f32(go), device='cuda'))
    want.backward(torch.tensor(ref.f32(go), dtype=torch.float64))
    k0 = 2 * sc * ref.f32(go)
    safe = np.where(s > 0, s, 1.0)
    kerr = np.where(s > 0, abs(k0) * e_s * (1 + gamma / safe) / safe + 6 * U * np.abs(k0 * d / safe), 0.0)
    _check('  d chnorm', g.grad, gr.grad.numpy(), np.abs(g64) * kerr[:, None])
    assert float(g.grad[N - 1, :, H // 2, W // 3].abs().max()) == 0.0


def _mbstd_bounds(x0, gs, eps, gstat, ggx):
    """fp32 error bounds of mbstd_fwd / mbstd_bwd / mbstd_bwdbwd from float64 quantities.  Per feature (group g, column f):
        mu: gs terms and a division, d_i = x_i - mu:          e_d = (gs + 2) u max_i |x_i|
        v = sum d_i^2 (to 2 sum |d_i| e_d + gs e_d^2), s = sqrt(v / (gs - 1) + eps), relative:
                                                               r_s = (sum |d_i| e_d + gs e_d^2 / 2) / ((gs - 1) s^2) + (gs + 4) u
        stat = mean_f s:                                       mean_f (r_s s) + (ceil(F / 256) + 12) u stat
        gx_i = k d_i, k = gstat / (F (gs - 1) s):              |k| e_d + |k d_i| (r_s + 4 u)
        dot = sum ggx_i d_i:                                   e_dot = sum |ggx_i| e_d + (gs + 1) u sum |ggx_i d_i|
        g_gstat = c sum_f dot / s, c = 1 / (F (gs - 1)):       c sum_f (e_dot / s + |dot| / s (r_s + 3 u)) + (ceil(F / 256) + 12) u c sum_f |dot| / s
        g_x_i = c gstat ((ggx_i - mg) / s - d_i k2), k2 = dot / (s^3 (gs - 1)):
            c |gstat| ((|ggx_i| + |mg|) / s (r_s + (gs + 4) u) + |d_i k2| (3 r_s + 6 u) + e_d |k2| + |d_i| e_dot / (s^3 (gs - 1)))
            + 3 u |g_x_i|."""
    B = x0.shape[0]
    G, F = B // gs, x0[0].size
    x = x0.astype(np.float64).reshape(G, gs, F)
    gg = ggx.astype(np.float64).reshape(G, gs, F)
    G_ = gstat.astype(np.float64).reshape(G, 1)
    d = x - x.mean(axis=1, keepdims=True)
    e_d = (gs + 2) * U * np.abs(x).max(axis=1)                                    # (G, F)
    s = np.sqrt((d * d).sum(axis=1) / (gs - 1) + eps)
    r_s = (np.abs(d).sum(axis=1) * e_d + gs * e_d * e_d / 2) / ((gs - 1) * s * s) + (gs + 4) * U
    chain = -(-F // 256) + 12
    t_stat = (r_s * s).mean(axis=1) + chain * U * s.mean(axis=1)
    k = G_ / (F * (gs - 1) * s)
    t_gx = np.abs(k)[:, None] * e_d[:, None] + np.abs(k[:, None] * d) * (r_s + 4 * U)[:, None]
    dot = (gg * d).sum(axis=1)
    e_dot = np.abs(gg).sum(axis=1) * e_d + (gs + 1) * U * np.abs(gg * d).sum(axis=1)
    c = 1.0 / (F * (gs - 1))
    t_ggstat = c * ((e_dot / s + np.abs(dot) / s * (r_s + 3 * U)).sum(axis=1) + chain * U * (np.abs(dot) / s).sum(axis=1))
    mg = gg.mean(axis=1, keepdims=True)
    k2 = dot / (s ** 3 * (gs - 1))
    val = c * G_[:, None] * ((gg - mg) / s[:, None] - d * k2[:, None])
    t_g_x = c * np.abs(G_)[:, None] * ((np.abs(gg) + np.abs(mg)) / s[:, None] * (r_s + (gs + 4) * U)[:, None] +
                                       np.abs(d * k2[:, None]) * (3 * r_s + 6 * U)[:, None] + (e_d * np.abs(k2))[:, None] +
                                       np.abs(d) * (e_dot / (s ** 3 * (gs - 1)))[:, None]) + 3 * U * np.abs(val)
    return t_stat, t_gx.reshape(x0.shape), t_ggstat, t_g_x.reshape(x0.shape)


@pytest.mark.parametrize('B,C,H,W,gs', [(8, 5, 4, 4, 4), (6, 3, 7, 9, 2), (6, 3, 7, 9, 3), (4, 16, 32, 32, 4)])
def test_mbstd_stat_first_and_second_order_against_float64(B, C, H, W, gs):
    """F = C H W below 256 (80), no multiple of 256 (189) and far above it (16384).  Where there is more than one group the
    last one is one sample repeated: s = sqrt(eps) there and every gradient is finite.  Forward, backward and the backward
    of the backward (towards x and towards the cotangent) against float64 autograd of ``pointwise_reference.mbstd_stat``,
    within ``_mbstd_bounds``.
    Measured: worst error / bound 0.05 (stat), 0.29 (gx), 0.01 (g_gstat), 0.17 (g_x)."""
    from gan_lab_amd import ops
    eps = 1e-8
    G = B // gs
    gen = np.random.default_rng(B * C + gs)
    x0 = gen.standard_normal((B, C, H, W)).astype(np.float32)
    if G > 1:
        x0[B - gs:] = x0[B - gs]
    gstat0 = (0.5 + gen.random(G)).astype(np.float32)
    ggx0 = gen.standard_normal((B, C, H, W)).astype(np.float32)
    t_stat, t_gx, t_ggstat, t_g_x = _mbstd_bounds(x0, gs, ref.f32(eps), gstat0, ggx0)

    x, gstat = _gpu(x0).requires_grad_(True), _gpu(gstat0).requires_grad_(True)
    xr = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    gstat_r = torch.tensor(gstat0, dtype=torch.float64, requires_grad=True)
    stat, stat_r = ops.mbstd_stat(x, gs, eps), ref.mbstd_stat(xr, gs, ref.f32(eps))
    _check(f'mbstd stat {(B, C, H, W, gs)}', stat, stat_r.detach().numpy(), t_stat)
    assert G == 1 or abs(stat_r[-1].item() - math.sqrt(ref.f32(eps))) < 1e-12
    gx, = torch.autograd.grad(stat, x, gstat, create_graph=True)
    gxr, = torch.autograd.grad(stat_r, xr, gstat_r, create_graph=True)
    _check('  gx', gx, gxr.detach().numpy(), t_gx)
    g_x, g_gstat = torch.autograd.grad(gx, (x, gstat), _gpu(ggx0))
    g_xr, g_gstat_r = torch.autograd.grad(gxr, (xr, gstat_r), torch.tensor(ggx0, dtype=torch.float64))
    _check('  g_gstat', g_gstat, g_gstat_r.numpy(), t_ggstat)
    _check('  g_x', g_x, g_xr.numpy(), t_g_x)


# =============================================================================================================================== #
# elementwise
# =============================================================================================================================== #
def _pair(n, seed):
    gen = np.random.default_rng(seed)
    return gen.standard_normal(n).astype(np.float32), (2 * gen.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 6, 7, 1024, 1025, 1026, 1027, 4 * GRID_CAP + 7])
def test_axpby_through_lerp_and_add(n):
    """out = a x + b y with the float32 scalars the kernel receives: two products and a sum, or a product and an FMA -
    2^-23 (|a x| + |b y|).  n < 4 and n % 4 in {1, 2, 3} run the scalar tail, the largest size a second grid-stride trip.
    The backward is the same kernel with y absent.  Measured: worst error / bound 0.93 (forward and backward), 0.50 (add)."""
    from gan_lab_amd import ops
    x0, y0 = _pair(n, n)
    x64, y64 = x0.astype(np.float64), y0.astype(np.float64)
    for alpha in (0.3, 1.0):
        a, b = ref.f32(float(1.0 - alpha)), ref.f32(float(alpha))
        x, y = _gpu(x0).requires_grad_(True), _gpu(y0).requires_grad_(True)
        out = ops.lerp(x, y, alpha)
        _check(f'lerp n={n} alpha={alpha}', out, a * x64 + b * y64, 2 * U * (np.abs(a * x64) + np.abs(b * y64)))
        out.backward(y.detach())
        _check('  d lerp / dx', x.grad, a * y64, U * np.abs(a * y64))
        _check('  d lerp / dy', y.grad, b * y64, U * np.abs(b * y64))
    _check(f'add n={n}', ops.add(_gpu(x0), _gpu(y0)), x64 + y64, 2 * U * (np.abs(x64) + np.abs(y64)))


@pytest.mark.parametrize('N,M', [(1, 1), (1, 7), (1, 4096), (3, 7), (5, 4096)])
def test_lerp_rows_against_float64(N, M):
    """out[n, m] = t[n] a + (1 - t[n]) b: the weight 1 - t is one rounding (exact for t >= 1/2), each product one, the sum
    one - u (2 |t a| + 3 |(1 - t) b|).  Measured: worst error / bound 0.90."""
    from gan_lab_amd import ops
    a0, b0 = _pair(N * M, N + M)
    t0 = np.random.default_rng(M).random(N).astype(np.float32)
    a64, b64, t64 = a0.astype(np.float64).reshape(N, M), b0.astype(np.float64).reshape(N, M), t0.astype(np.float64)[:, None]
    out = ops.lerp_rows(_gpu(a0).view(N, M), _gpu(b0).view(N, M), _gpu(t0))
    A, B = t64 * a64, (1.0 - t64) * b64
    _check(f'lerp_rows {(N, M)}', out, A + B, U * (2 * np.abs(A) + 3 * np.abs(B)))
    want = ref.lerp_rows(torch.tensor(a64), torch.tensor(b64), torch.tensor(t0, dtype=torch.float64)).numpy()
    assert np.array_equal(want, A + B)


@pytest.mark.parametrize('mode', ['scale', 'shift', 'both'])
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (2, 3, 4, 8), (1, 2, 1, 1), (3, 5, 64, 64)])
def test_chan_affine_against_float64(shape, mode):
    """y = x scale[c] + shift[c], H W % 4 != 0 (scalar kernel) and == 0 (float4 kernel): 2^-23 (|x scale| + |shift|).
    Measured: worst error / bound 0.50."""
    from gan_lab_amd import ops
    C = shape[1]
    gen = np.random.default_rng(sum(shape))
    x0 = gen.standard_normal(shape).astype(np.float32)
    sc0 = (1.0 + gen.standard_normal(C)).astype(np.float32) if mode != 'shift' else None
    sh0 = gen.standard_normal(C).astype(np.float32) if mode != 'scale' else None
    out = ops.chan_affine(_gpu(x0), _gpu(sc0) if sc0 is not None else None, _gpu(sh0) if sh0 is not None else None)
    t = lambda v: torch.tensor(v, dtype=torch.float64) if v is not None else None       # noqa: E731
    want = ref.chan_affine(t(x0), t(sc0), t(sh0)).numpy()
    xs = np.abs(x0.astype(np.float64) * (sc0.astype(np.float64).reshape(1, C, 1, 1) if sc0 is not None else 1.0))
    sh = np.abs(sh0.astype(np.float64)).reshape(1, C, 1, 1) if sh0 is not None else 0.0
    _check(f'chan_affine {shape} {mode}', out, want, 2 * U * (xs + sh))


@pytest.mark.parametrize('n', [1, 5, 4099, GRID_CAP + 3])
def test_mul_and_tanh_against_float64(n):
    """mul: one rounding, u |a b|.  tanh with +-20 (saturated: exactly +-1) and 0: tanhf to 4 u |tanh x|.  Its backward is
    g (1 - y^2) of the SAVED fp32 y: against the float64 1 - tanh^2 that is the error of y through d(1 - y^2) = 2 |y| dy,
    dy <= 4 u |y|, plus three roundings - |g| u (8 y^2 + 3 (1 - y^2)) + the floor |g| u for the saturated entries, where
    1 - y^2 is 0 in fp32 and 1.7e-17 in float64.
    Measured: worst error / bound 1.00 (mul: one rounding, 0.998), 0.59 (tanh), 0.41 (backward)."""
    from gan_lab_amd import ops
    a0, b0 = _pair(n, 3 * n)
    edge = np.array([20.0, -20.0, 0.0, 9.0, -9.0], dtype=np.float32)[:n]
    a0[:edge.size] = edge
    a64, b64 = a0.astype(np.float64), b0.astype(np.float64)
    _check(f'mul n={n}', ops.mul(_gpu(a0), _gpu(b0)), a64 * b64, U * np.abs(a64 * b64))
    x = _gpu(a0).requires_grad_(True)
    y = ops.tanh(x)
    _check(f'tanh n={n}', y, np.tanh(a64), 4 * U * np.abs(np.tanh(a64)))
    assert _f64(y)[:min(n, 2)].tolist() == [1.0, -1.0][:min(n, 2)]
    y.backward(_gpu(b0))
    y64 = np.tanh(a64)
    _check('  d tanh', x.grad, b64 * (1.0 - y64 * y64), np.abs(b64) * U * (8 * y64 * y64 + 3 * (1.0 - y64 * y64) + 1.0))
