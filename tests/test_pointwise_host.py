"""CPU tests of tests/pointwise_reference.py: the restatements that tests/test_gpu_pointwise.py holds the kernels to are
themselves tied to a published vector (Philox), to sampling theory (the normal draw), to the reference project's optimiser
(oracle.step.adam_update), to finite differences (the losses) and to integer arithmetic (the stream ledger's counts) - and the
perturbed forms a kernel could silently be are shown to differ from the right one by far more than the GPU tests allow."""
import math

import numpy as np
import pytest
import torch

import pointwise_reference as ref
from sample_reference import philox4x32_10

RANDN_BOUND = 8e-6                   # test_gpu_pointwise.RANDN_BOUND
RANDN_SIZES = (1, 3, 4, 5, 1023, 4099)
RANDN_GRID_TRIP = 4 * 256 * 8 * 256 + 5       # test_gpu_pointwise.RANDN_SIZES[-1]: a second grid-stride trip


def test_philox_known_answer_vectors():
    """Random123's known-answer vector for philox4x32 with 10 rounds, counter 0 and key 0 (the project's counters keep
    c[2] = c[3] = 0, so of the published vectors only this one is reachable through the 64-bit interface); the vectorised form
    over a uint64 array must agree with the scalar form word for word, across the 32- and 64-bit wraps."""
    assert philox4x32_10(0, 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ctrs = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 0x0123456789ABCDEF]
    for seed in (0, 0x5EED, 0xFEDCBA9876543210):
        for c in ctrs:
            w = ref.stream_words(seed, c, 3)
            for j in range(3):
                assert [int(x) for x in w[j]] == philox4x32_10((c + j) & ref.M64, seed), (seed, c, j)


def test_randn_reference_moments():
    """n = 2^16 draws of N(0, 1): the sample mean has standard deviation 1 / sqrt n, the sample variance sqrt(2 / n), the
    sample fourth moment sqrt((105 - 9) / n); 5 standard deviations each (the draw is deterministic: a bar, not a flake
    budget).  Both halves of the Box-Muller pair are checked on their own, and they are uncorrelated."""
    n = 1 << 16
    z = ref.randn_reference(0x5A17ED0123456789, 12345, n)
    assert z.shape == (n,) and np.isfinite(z).all()
    for name, x in (('all', z), ('cos', z[0::2]), ('sin', z[1::2])):
        k = x.size
        mean, var, m4 = x.mean(), x.var(), (x ** 4).mean()
        print(f'{name}: mean {mean:+.4e} (5 sd {5 / math.sqrt(k):.4e}), var {var:.5f} (5 sd {5 * math.sqrt(2 / k):.5f}), '
              f'm4 {m4:.4f} (5 sd {5 * math.sqrt(96 / k):.4f})')
        assert abs(mean) <= 5 / math.sqrt(k)
        assert abs(var - 1.0) <= 5 * math.sqrt(2 / k)
        assert abs(m4 - 3.0) <= 5 * math.sqrt(96 / k)
    assert abs((z[0::2] * z[1::2]).mean()) <= 5 / math.sqrt(n / 2)
    assert np.abs(z).max() <= math.sqrt(64 * math.log(2)) + 1e-12


@pytest.mark.parametrize('variant', ['swap', 'drop_high', 'floor4'])
def test_randn_perturbations_are_far_outside_the_bound(variant):
    """A swapped sin / cos, a counter whose high word is dropped and n4 = n >> 2 against the right form at the GPU test's
    sizes, seeds and offsets: wherever the perturbation can show at all (a dropped high word needs a counter above 2^32; a
    floored group count needs n % 4 != 0) it shows as an error of order 1, or as missing elements."""
    seen = 0
    for seed in (0x5EED, 0x5A17ED0123456789):
        for offset in (0, 12345, 2 ** 32 - 2, 2 ** 64 - 2):
            for n in RANDN_SIZES:
                good, bad = ref.randn_reference(seed, offset, n), ref.randn_reference(seed, offset, n, variant)
                differs = not np.array_equal(good, bad, equal_nan=True)
                if variant == 'swap':
                    expect = True
                elif variant == 'drop_high':
                    expect = any(((offset + j) & ref.M64) >> 32 for j in range((n + 3) // 4))
                else:
                    expect = n % 4 != 0
                assert differs == expect, (variant, hex(seed), offset, n)
                if differs:
                    seen += 1
                    d = np.abs(good - bad)
                    assert np.isnan(d).any() or np.nanmax(d) > 1e3 * RANDN_BOUND, (variant, hex(seed), offset, n, np.nanmax(d))
    assert seen >= 8
    n = RANDN_GRID_TRIP                                # the GPU test's largest size, once: n % 4 == 1, counters pass 2^32
    good, bad = ref.randn_reference(0x5A17ED0123456789, 2 ** 32 - 2, n), ref.randn_reference(0x5A17ED0123456789, 2 ** 32 - 2, n, variant)
    d = np.abs(good - bad)
    assert np.isnan(d).any() or np.nanmax(d) > 1e3 * RANDN_BOUND


def test_integer_draws_stay_in_range_and_use_their_counters():
    seed = 0x0123456789ABCDEF
    for high in (1, 3, 1000, 2 ** 24):
        v = ref.randint_reference(seed, 2 ** 32 - 2, 1027, high)
        assert v.min() >= 0 and v.max() < high and (high == 1 or len(set(v.tolist())) > 1)
    for (N, n, S) in ((3, 5, 1024), (7, 128, 16), (1, 1, 8)):
        v = ref.swd_positions_reference(seed, 2 ** 64 - 2, N, n, S)
        assert v.shape == (N, n, 2) and v.min() >= 3 and v.max() <= S - 4
    d = ref.swd_directions_reference(seed, 7, 3)
    assert d.shape == (3, 147) and np.allclose((d * d).sum(axis=1), 1.0, atol=1e-14)


def test_ledger_identities():
    """The integer facts ``gan_lab_amd/rng.py`` rests on, for n in 1 .. 64: a draw of n elements, four per counter, reads
    ceil(n / 4) = (n + 3) // 4 counters; n patch centres are 2n words, (2n + 3) // 4 = (n + 1) // 2 counters per image; the
    counters a draw of ``count`` counters reads end right below ``offset + count`` - also across the 32- and 64-bit wraps."""
    for n in range(1, 65):
        assert (n + 3) // 4 == -(-n // 4) == ref.randn_counters(n) == ref.randint_counters(n)
        assert (2 * n + 3) // 4 == (n + 1) // 2 == -(-2 * n // 4) == ref.swd_positions_counters(1, n)
        assert ref.swd_positions_counters(5, n) == 5 * ((n + 1) // 2)
        assert 4 * ((n + 3) // 4) >= n > 4 * ((n + 3) // 4 - 1)              # the last counter is used, none beyond it
        assert ref.swd_directions_counters(n) == 147 * n
        for offset in (0, 2 ** 32 - 2, 2 ** 64 - 2):
            count = (n + 3) // 4
            here, there = ref.counter_range(offset, count), ref.counter_range(offset + count, count)
            assert len(here) == count and not (here & there)


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
ADAM_CONFIGS = [(0.0, 0.99, 0.0), (0.5, 0.999, 0.0), (0.9, 0.999, 1e-2)]


@pytest.mark.parametrize('b1,b2,wd', ADAM_CONFIGS)
def test_adam_reference_agrees_with_the_oracle(b1, b2, wd):
    """oracle.step.adam_update is the reference project's single-tensor torch.optim.Adam; on float64 tensors the two are the
    same recurrence up to the order of float64 operations."""
    from oracle import step as S
    p0, grads = ref.adam_inputs(1000)
    lr, eps = 1e-3, 1e-8
    p, m, v = p0.astype(np.float64), np.zeros(1000), np.zeros(1000)
    pt = torch.tensor(p0, dtype=torch.float64)
    st = S.new_adam_state(pt)
    for t, g in enumerate(grads, 1):
        p, m, v = ref.adam_reference(p, g, m, v, lr, b1, b2, eps, wd, 1 - b1 ** t, 1 - b2 ** t)
        S.adam_update(pt, torch.tensor(g, dtype=torch.float64), st, lr, b1, b2, eps, wd)
    for name, a, b in (('p', p, pt), ('m', m, st['exp_avg']), ('v', v, st['exp_avg_sq'])):
        err = np.abs(a - b.numpy()).max() / max(np.abs(a).max(), 1e-300)
        print(f'{name}: {err:.3e}')
        assert err <= 1e-13


@pytest.mark.parametrize('variant', ['swap_betas', 'swap_bc', 'wd_on_p'])
def test_adam_wrong_variants_leave_the_bound(variant):
    """At the GPU test's inputs every wrong recurrence leaves the right one's fp32 error bound: swapped betas and swapped
    bias corrections in every configuration (beta1 != beta2 in all of them), decoupled weight decay where wd != 0."""
    caught = 0
    for b1, b2, wd in ADAM_CONFIGS:
        for n in (1, 1000, 4097):
            p0, grads = ref.adam_inputs(n)
            p, m, v, err = ref.adam_run(p0, grads, 1e-3, b1, b2, 1e-8, wd)
            q, mq, vq, _ = ref.adam_run(p0, grads, 1e-3, b1, b2, 1e-8, wd, variant)
            out = bool((np.abs(q - p) > err['p']).any() or (np.abs(mq - m) > err['m']).any() or (np.abs(vq - v) > err['v']).any())
            worst = (np.abs(q - p) / np.maximum(err['p'], 1e-300)).max()
            print(f'{variant} b1={b1} b2={b2} wd={wd} n={n}: |dp| up to {worst:.3g} x the bound')
            if variant == 'wd_on_p' and wd == 0.0:
                assert not out
            else:
                assert out and worst > 10
                caught += 1
    assert caught >= 3


def test_adam_bound_is_a_few_ulps_per_step():
    """The bound the GPU test uses is not vacuous: after 5 steps its median is below 20 ulps of |p|, and its largest value
    below 1000 ulps of max(|p|, lr) - reached where |p| ~ lr and weight decay feeds p's own rounding back into its gradient
    (g' = wd p), tens of ulps elsewhere."""
    for b1, b2, wd in ADAM_CONFIGS:
        p0, grads = ref.adam_inputs(4097)
        p, m, v, err = ref.adam_run(p0, grads, 1e-3, b1, b2, 1e-8, wd)
        rel = err['p'] / np.maximum(np.abs(p), 1e-3) / 2.0 ** -24
        print(f'b1={b1} b2={b2} wd={wd}: bound on p: median {np.median(rel):.1f}, max {rel.max():.1f} ulps of max(|p|, lr)')
        assert np.median(rel) <= 20 and rel.max() <= 1000


# ---- losses: finite differences against autograd ------------------------------------------------------------------------------
def _leaf(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).requires_grad_(True)


def _fd_check(fn, x, tol=1e-7):
    auto, = torch.autograd.grad(fn(x), x)
    fd = ref.fd_gradient(fn, x)
    err = ((auto - fd).abs().max() / auto.abs().max().clamp_min(1e-30)).item()
    print(f'fd against autograd: {err:.3e}')
    assert err <= tol


def test_loss_gradients_agree_with_finite_differences():
    x = _leaf(13, seed=1, scale=3.0)
    with torch.no_grad():
        x[0] = 0.0                                                           # smooth there: sigmoid(0) - t
    for t in (0.0, 1.0):
        _fd_check(lambda z: ref.bce_logits_mean(z, t), x)
        direct = x.detach().clamp(min=0) - x.detach() * t + torch.log1p(torch.exp(-x.detach().abs()))
        assert abs(direct.mean().item() - ref.bce_logits_mean(x, t).item()) <= 1e-15
    with torch.no_grad():
        x[0] = 0.3
    for a, b in ((1.0, -1.0), (1.0, 1.0), (0.0, -1.0)):
        _fd_check(lambda z: ref.hinge_mean(z, a, b), x)                 # no draw within 1e-6 of a kink
    _fd_check(lambda z: ref.chnorm_penalty(z, 1.0, 0.37), _leaf(2, 3, 2, 3, seed=2))
    for gs in (2, 3):
        w = torch.tensor([0.7, -1.3, 0.4])[:6 // gs].double()
        _fd_check(lambda z: (ref.mbstd_stat(z, gs) * w).sum(), _leaf(6, 2, 2, 2, seed=3))
    _fd_check(lambda z: ref.sum_all(z, 0.5), x)
    _fd_check(lambda z: ref.sumsq_all(z, 0.5), x)
    y = _leaf(13, seed=4)
    _fd_check(lambda z: (ref.axpby(z, y, 0.3, 0.7) ** 2).sum(), x)
    a, b, t = _leaf(3, 5, seed=5), _leaf(3, 5, seed=6), torch.tensor([0.2, 0.5, 0.9]).double()
    _fd_check(lambda z: (ref.lerp_rows(z, b, t) ** 2).sum(), a)
    xs = _leaf(2, 3, 2, 2, seed=7)
    sc, sh = _leaf(3, seed=8), _leaf(3, seed=9)
    _fd_check(lambda z: (ref.chan_affine(z, sc, sh) ** 2).sum(), xs)
    _fd_check(lambda z: (ref.chan_affine(xs, z, sh) ** 2).sum(), sc)


def test_loss_edge_gradients():
    """On a hinge kink and at a zero channel vector the float64 references give gradient 0, as the kernels do; a group of
    identical samples has s = sqrt(eps) and a finite (zero) gradient."""
    x = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(ref.hinge_mean(x, 1.0, -1.0), x)
    assert g.tolist() == [0.0, -1.0 / 3, 0.0]
    z = _leaf(2, 3, 2, 2, seed=11)
    with torch.no_grad():
        z[1, :, 0, 1] = 0.0
    gz, = torch.autograd.grad(ref.chnorm_penalty(z, 1.0, 1.0), z)
    assert torch.isfinite(gz).all() and gz[1, :, 0, 1].abs().max() == 0.0
    s = _leaf(1, 4, seed=12).detach().expand(4, 4).clone().requires_grad_(True)
    stat = ref.mbstd_stat(s, 4)
    gs_, = torch.autograd.grad(stat.sum(), s)
    assert abs(stat.item() - 1e-4) < 1e-12 and torch.isfinite(gs_).all() and gs_.abs().max() == 0.0
