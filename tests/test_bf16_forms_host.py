"""The table of tests/bf16_forms.py itself, on the CPU: its rounding against ``tensor.to(torch.bfloat16)``, its float64
restatements against ``torch.autograd`` of the layer definitions, the edges its restated plans claim, its coverage of the kernels
csrc/conv_bf16.hip defines, the ATen yardstick on every (row, distribution) of the GPU test, and targeted mistakes that must
each leave the bound tests/test_gpu_bf16_kernels.py uses."""
import os
import re

import pytest
import torch

import bf16_forms as B
import x3_forms as X
from util import rel_err

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gan_lab_amd', 'csrc', 'conv_bf16.hip')
BF16_MAX = 3.3895313892515355e38        # 0x7f7f0000


# ---- rne_bf16 ------------------------------------------------------------------------------------------------------------------------
from_bits = B.from_bits


def same_rounding(t):
    got, want = B.rne_bf16(t), t.to(torch.bfloat16).float()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])
    assert torch.equal(got, B.rne_bf16(got)[...]) or nan.any()          # (what it returns is a bf16 number)
    return got


def test_rne_bf16_on_random_bit_patterns():
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 2 ** 32, (2 ** 21,), generator=g, dtype=torch.int64)
    t = from_bits(u)
    assert torch.isnan(t).any() and (t.abs() < 1.1754944e-38).any()        # NaNs and subnormals are among them
    same_rounding(t)


def test_rne_bf16_on_every_tie_of_a_binade():
    # binade [1, 2): kept bits 0x3f80 .. 0x3fff, low half exactly 0x8000 (a tie), one below and one above it
    kept = torch.arange(0x3F80, 0x4000, dtype=torch.int64)
    for sign in (0, 0x80000000):
        ties = from_bits(sign | (kept << 16) | 0x8000)
        got = same_rounding(ties)
        up = (kept & 1) == 1                   # an odd low kept bit rounds away, an even one stays
        assert torch.equal(B.bf16_bits(got).to(torch.int64) & 0xFFFF, ((sign >> 16) | (kept + up.to(torch.int64))) & 0xFFFF)
        assert up.any() and (~up).any()
        same_rounding(from_bits(sign | (kept << 16) | 0x7FFF))
        same_rounding(from_bits(sign | (kept << 16) | 0x8001))


def test_rne_bf16_on_zeros_subnormals_overflow_inf_and_nan():
    z = same_rounding(torch.tensor([0.0, -0.0]))
    assert z.view(torch.int32).tolist() == [0, -2 ** 31]
    sub = torch.arange(1, 2 ** 23, 997, dtype=torch.int64)
    same_rounding(torch.cat([from_bits(sub), from_bits(sub | 0x80000000), from_bits(torch.tensor([1, 0x7FFF, 0x8000, 0x8001, 0x7FFFFF]))]))
    # above bf16's maximum: from the first pattern that rounds up (0x7f7f8000) to fp32's maximum, all must become inf
    over = torch.cat([torch.arange(0x7F7F8000, 0x7F800000, 509, dtype=torch.int64), torch.tensor([0x7F7F8000, 0x7F7FFFFF])])
    for sign, inf in ((0, float('inf')), (0x80000000, float('-inf'))):
        got = same_rounding(from_bits(over | sign))
        assert (got == inf).all()
    assert B.rne_bf16(torch.tensor([B.FP32_MAX])).item() == float('inf')
    assert same_rounding(from_bits(torch.tensor([0x7F7F7FFF]))).item() == BF16_MAX          # the last one that stays finite
    same_rounding(torch.tensor([float('inf'), float('-inf')]))
    nans = same_rounding(from_bits(torch.tensor([0x7FC00000, 0x7F800001, 0xFFC00000, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF])))
    assert torch.isnan(nans).all()


# ---- restatements against the definitions ---------------------------------------------------------------------------------------------
SMALL = [(op, kind) for op in B.OPS for kind in ('plain', 'up', 'pool')]


def small_row(op, kind, shape=(2, 3, 4, 3, 4)):
    return B.Row('host_%s_%s' % (op, kind), op, kind, shape, dict(plan=[('', 0)]), None, '')


def agree(a, b, bar=1e-12):
    assert a.dtype == torch.float64 and tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    err = (a - b.detach()).abs().max().item() / b.detach().abs().max().item()
    assert err <= bar, err


@pytest.mark.parametrize('op,kind', SMALL, ids=['%s-%s' % c for c in SMALL])
def test_restatement_agrees_with_autograd_of_the_definition(op, kind):
    f = small_row(op, kind)
    T = X.to_f64(B.round_operands(f, X.draw(f, 'randn')))
    got, want = f.ref(f, T), f.define(f, T)
    assert len(got) == len(want) == len(f.outs) == 1
    agree(got[0], want[0])


@pytest.mark.parametrize('kind', ['plain', 'up', 'pool'])
def test_strip_and_segment_forms_of_the_weight_gradient_are_the_weight_gradient(kind):
    f = small_row('wgrad', kind, (2, 3, 4, 9, 32))          # taps at 9 x 32 or 18 x 64
    T = X.to_f64(B.round_operands(f, X.draw(f, 'randn')))
    want, = f.ref(f, T)
    agree(B.r_wgrad_by_strips(f, T)[0], want)
    if kind != 'plain':
        agree(B.r_wgrad_by_segments(f, T, 3)[0], want)
        agree(B.r_wgrad_by_segments(f, T, 6)[0], want)


def test_pack_layout_is_the_kernel_index_arithmetic():
    """pack_layout against the kernel's own loop over e = (((chunk * 9 + tap) * 4 + kg) * CO + co) * 8 + j, element by element"""
    cout, cin = 128, 64
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3)
    for mode in (B.PACK_FWD, B.PACK_DGRAD):
        lay = B.pack_layout(w, mode).reshape(-1)
        CO, CI = (cin, cout) if mode == B.PACK_DGRAD else (cout, cin)
        assert lay.numel() == 9 * CO * CI
        g = torch.Generator().manual_seed(mode)
        for e in torch.randint(0, lay.numel(), (500,), generator=g).tolist() + [0, lay.numel() - 1]:
            j, t = e & 7, e >> 3
            co, t = t % CO, t // CO
            kg, t = t & 3, t >> 2
            tap, chunk = t % 9, t // 9
            ci = chunk * 32 + kg * 8 + j
            want = w.reshape(cout, cin, 9)[ci, co, 8 - tap] if mode == B.PACK_DGRAD else w.reshape(cout, cin, 9)[co, ci, tap]
            assert lay[e].item() == want.item(), (mode, e)


# ---- the plans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(B.ROWS))
def test_row_reaches_its_edge(name):
    r = B.ROWS[name]
    assert r.plan and r.symbol == r.plan[0][0] and r.why
    for sym, grid in r.plan:
        assert isinstance(grid, int) and 0 < grid < 2 ** 31, (name, sym, grid)
    assert r.edge(r.facts), (name, r.why, r.facts)
    n, ci, hin, win, co, up, pool = B.geom_args(r.kind, *r.shape)
    assert B.bf16_ok(n, ci, co, hin, win, up, pool), name
    if r.role == 'wgrad' and not r.tile:
        assert B.bf16_wgrad_ok(n, ci, co, hin, win, up, pool, roll=True), name
    if r.tile:          # with the rolling kernel off the fused up / pool geometry is refused and the plain one at the taps taken
        assert B.bf16_wgrad_ok(n, ci, co, hin, win, up, pool, roll=False) == (r.kind == 'plain'), name
        assert B.bf16_wgrad_ok(n, ci, co, r.facts['H'], r.facts['W'], 0, 0, roll=False), name
    assert r.n >= 2 or 'ragged' in name or 'odd_rs' in name or 'cout_chunks' in name, name


def test_named_edges_of_the_plans():
    assert B.bf16_splitk_plan(1, 448, 64, 16, 16) == 3 and B.split_sizes(14, 3) == [5, 5, 4]
    assert B.bf16_splitk_plan(2, 256, 128, 16, 16) == 2 and B.bf16_splitk_plan(1, 512, 64, 16, 16) == 4     # cases of test_gpu_bf16.py
    assert B.bf16_splitk_plan(2, 384, 128, 16, 16) == 3 and B.split_sizes(12, 3) == [4, 4, 4]
    assert B.bf16_splitk_plan(4, 256, 128, 64, 64) == 1 and B.bf16_splitk_plan(3, 256, 128, 64, 64) == 2        # 128 / 96 tiles
    assert B.bf16_splitk_plan(1, 224, 64, 16, 16) == 1                                                        # 7 chunks
    for chunks in range(8, 65):         # no split of any plan is empty: c_first < CI / 32 in every workgroup
        for s in (2, 3, 4):
            if chunks // s >= 4:
                assert min(B.split_sizes(chunks, s)) >= 1, (chunks, s)
    # RS: the largest divisor of H of at most 32; the padding steps of the unroll by 3 take all three values
    assert [B.wr_plan(1, 64, 64, h, 32)['RS'] for h in (8, 16, 24, 40, 136, 128, 56)] == [8, 16, 24, 20, 17, 32, 28]
    assert {B.wr_plan(1, 64, 64, h, 32)['pad_steps'] for h in (8, 16, 24)} == {0, 1, 2}
    assert not B.bf16_ok(2, 32, 64, 8, 32) and not B.bf16_ok(2, 64, 64, 8, 16) and B.bf16_ok(2, 64, 64, 8, 16, up=1)
    assert not B.bf16_wgrad_ok(2, 64, 64, 16, 16) and B.bf16_wgrad_ok(2, 64, 64, 16, 16, up=1) and \
        not B.bf16_wgrad_ok(2, 64, 64, 16, 16, up=1, roll=False)
    for name, (py, px) in B.NONFINITE:
        r = B.ROWS[name]
        h, w = r.hw_out if r.role == 'dgrad' else r.hw_in
        assert r.n >= 2 and py < h and px < w, (name, py, px, h, w)
        if r.role == 'wgrad':       # off the image's first and last row (see bf16_forms.NONFINITE)
            assert 0 < py < h - 1


def kernels_defined():
    with open(SRC) as fh:
        text = fh.read()
    return set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', text)), text


def test_every_kernel_and_instantiation_has_a_row():
    names, text = kernels_defined()
    assert 'conv_fwd_bf16_kernel' in names and 'pack_bf16_kernel' in names and len(names) >= 7, sorted(names)
    have = [B.norm(sym) for r in B.ROWS.values() for sym, _ in r.plan] + ['pack_bf16_kernel']
    assert not sorted(names - {re.match(r'\w+', h).group(0) for h in have})
    assert not sorted({re.match(r'\w+', h).group(0) for h in B.INSTANTIATIONS} ^ names)
    for want in B.INSTANTIATIONS:
        assert any(B.norm(want) in h for h in have), want
    # what the launchers can instantiate, from their text: GL_LAUNCH((kernel<args>) ...
    for kern, args in re.findall(r'GL_LAUNCH\(\((\w+)<([^>]*)>\)', text):
        args = [a.strip() for a in args.split(',')]
        if kern == 'conv_fwd_bf16_kernel' and len(args) == 2:
            args += ['false', 'false']
        want = B.norm('%s<%s>' % (kern, ', '.join(args)))
        assert want in [B.norm(i) for i in B.INSTANTIATIONS], want
    # one row per instantiation runs under every distribution; the odd-RS and ragged split-K rows are among them
    dist_syms = {B.norm(r.symbol) for r in B.ROWS.values() if r.dists}
    for want in B.INSTANTIATIONS:
        if 'conv_' in want:
            assert B.norm(want) in dist_syms, want
    assert all(r.dists for n, r in B.ROWS.items() if 'odd_rs' in n or 'ragged' in n)


# ---- the ATen yardstick alone, on every (row, distribution) the GPU test runs ---------------------------------------------------------
DIST_ROWS = [n for n, r in B.ROWS.items() if r.dists]


@pytest.mark.parametrize('name', DIST_ROWS)
def test_aten_fp32_is_finite_and_within_half_the_bar_on_every_distribution(name):
    f = B.ROWS[name]
    for dist in X.DISTS:
        R = B.round_operands(f, X.draw(f, dist))
        want, = f.ref(f, X.to_f64(R))
        aten, = f.define(f, R)
        assert aten.dtype == torch.float32 and torch.isfinite(aten).all() and torch.isfinite(want).all(), (name, dist)
        if dist in ('tiny', 'huge'):
            assert 1e-20 <= want.pow(2).mean().sqrt().item() <= 1e20 and want.abs().max().item() <= 1e20, (name, dist)
        assert rel_err(aten.detach(), want) <= X.TOL / 2, (name, dist, rel_err(aten.detach(), want))


# ---- targeted mistakes must leave the bound of the GPU test ----------------------------------------------------------------------------
def leaves(f, wrong, right):
    e = rel_err(wrong, right)
    assert e > f.tol, (f.name, e, f.tol)
    return e


def rounded(f, **kw):
    return X.to_f64(B.round_operands(f, X.draw(f, 'randn'), **kw))


@pytest.mark.parametrize('name', ['fwd_8x32', 'up_dgrad_8x32', 'roll_pad2'])
def test_mistake_truncation_instead_of_rne(name):
    f = B.ROWS[name]
    leaves(f, f.ref(f, rounded(f, rne=B.trunc_bf16))[0], f.ref(f, rounded(f))[0])


@pytest.mark.parametrize('name', ['fwd_8x32', 'pool_dgrad_8x32'])
def test_mistake_weight_rounded_before_the_scale(name):
    f = B.ROWS[name]
    leaves(f, f.ref(f, rounded(f, scale_first=False))[0], f.ref(f, rounded(f))[0])


@pytest.mark.parametrize('name', ['splitk_ragged_16x16', 'splitk_ragged_up', 'splitk_ragged_pool', 'splitk_dgrad_cout_chunks'])
def test_mistake_last_split_drops_its_final_chunk(name):
    f = B.ROWS[name]
    T = rounded(f)
    leaves(f, f.ref(f, T, mistake='drop_last_chunk')[0], f.ref(f, T)[0])


@pytest.mark.parametrize('name', ['roll_plain', 'roll_up', 'roll_pool'])
def test_mistake_halo_column_from_the_wrong_side(name):
    f = B.ROWS[name]
    T = rounded(f)
    leaves(f, B.r_wgrad_by_strips(f, T, halo_wrong_side=True)[0], f.ref(f, T)[0])


@pytest.mark.parametrize('name', ['roll_up_odd_rs', 'roll_pool_odd_rs'])
def test_mistake_source_row_of_an_odd_segment_start(name):
    f = B.ROWS[name]
    T = rounded(f)
    right, = f.ref(f, T)
    agree(B.r_wgrad_by_segments(f, T, f.facts['RS'])[0], right)
    leaves(f, B.r_wgrad_by_segments(f, T, f.facts['RS'], odd_start_row_off_by_one=True)[0], right)
    # with an even RS no segment starts on an odd row and the same mistake changes nothing: the odd-RS rows are what catches it
    g = B.ROWS['roll_up' if f.kind == 'up' else 'roll_pool']
    Tg = rounded(g)
    assert rel_err(B.r_wgrad_by_segments(g, Tg, g.facts['RS'], odd_start_row_off_by_one=True)[0], g.ref(g, Tg)[0]) <= 1e-12


@pytest.mark.parametrize('name', ['pool_fwd_8x32', 'pool_dgrad_16x16', 'splitk_ragged_pool', 'roll_pool'])
def test_mistake_pooled_quarter_missing(name):
    f = B.ROWS[name]
    T = rounded(f)
    leaves(f, f.ref(f, T, mistake='no_quarter')[0], f.ref(f, T)[0])


def test_mistake_dgrad_pack_without_the_tap_flip():
    """the pack test's bound is bit equality"""
    g = torch.Generator().manual_seed(5)
    wq = B.rne_bf16(torch.randn(128, 64, 3, 3, generator=g) * 0.04)
    right, wrong = B.bf16_bits(B.pack_layout(wq, B.PACK_DGRAD)), B.bf16_bits(B.pack_layout(wq, B.PACK_DGRAD, flip=False))
    assert not torch.equal(right, wrong)
    assert tuple(right.shape) == (4, 9, 4, 64, 8)           # [chunk of Cout][tap][kg][CO = Cin][8]
    assert torch.equal(right[:, 4], wrong[:, 4]) and torch.equal(right[:, 0], wrong[:, 8])      # the centre tap stays, 0 <-> 8
    assert not torch.equal(B.bf16_bits(B.pack_layout(wq, B.PACK_FWD)).reshape(-1), right.reshape(-1))
