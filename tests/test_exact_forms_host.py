"""The table of tests/exact_forms.py itself, on the CPU: its float64 restatements against ``torch.autograd`` of the layer
definitions, its coverage of the kernels the seven source files define, and what its restated plans claim."""
import os
import re

import pytest
import torch

import exact_forms as E
import x3_forms as X

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'gan_lab_amd', 'csrc')
SOURCES = ('conv.hip', 'conv_s2.hip', 'conv_roll_blur.hip', 'conv_s2_roll.hip', 'conv_s2_roll_blur.hip', 'wgrad_roll.hip', 'mod.hip')

# one small shape per form of operation: (op, kind, (N, Cin, Cout, H, W), ks)
SMALL = [('fwd', 'plain', (2, 3, 4, 5, 6), 3), ('fwd', 'plain', (2, 3, 4, 5, 6), 1), ('fwd', 'up', (2, 3, 4, 3, 4), 3),
         ('fwd', 'pool', (2, 3, 4, 3, 4), 3), ('dgrad', 'plain', (2, 3, 4, 5, 6), 3), ('dgrad', 'plain', (2, 3, 4, 5, 6), 1),
         ('dgrad', 'up', (2, 3, 4, 3, 4), 3), ('dgrad', 'pool', (2, 3, 4, 3, 4), 3), ('dgrad_mask', 'plain', (2, 3, 4, 5, 6), 3),
         ('wgrad', 'plain', (2, 3, 4, 5, 6), 3), ('wgrad', 'plain', (2, 3, 4, 5, 6), 1), ('wgrad', 'up', (2, 3, 4, 3, 4), 3),
         ('wgrad', 'pool', (2, 3, 4, 3, 4), 3), ('wgrad_aff', 'plain', (2, 3, 4, 5, 6), 3), ('wgrad_aff', 'up', (2, 3, 4, 3, 4), 3),
         ('fwd_aff', 'plain', (2, 3, 4, 5, 6), 3), ('fwd_aff', 'up', (2, 3, 4, 3, 4), 3), ('tail', 'plain', (2, 3, 4, 5, 6), 3),
         ('mod', 'plain', (2, 3, 4, 5, 6), 3), ('blur', 'plain', (2, 3, 4, 5, 6), 3), ('up_blur_tail', 'up', (2, 3, 4, 3, 4), 3),
         ('pool_dgrad_blur', 'pool', (2, 3, 4, 3, 4), 3), ('rgb', 'plain', (2, 3, 4, 5, 6), 3)]


@pytest.mark.parametrize('op,kind,shape,ks', SMALL, ids=['%s-%s-k%d' % (c[0], c[1], c[3]) for c in SMALL])
def test_restatement_agrees_with_autograd_of_the_definition(op, kind, shape, ks):
    f = E.Row('host_%s_%s_%d' % (op, kind, ks), op, kind, shape, ks, '', [], '')
    T = X.to_f64(X.draw(f, 'randn'))
    got, want = f.ref(f, T), f.define(f, T)
    assert len(got) == len(want) == len(f.outs)
    for name, a, b in zip(f.outs, got, want):
        assert a.dtype == torch.float64 and tuple(a.shape) == tuple(b.shape), (name, a.shape, b.shape)
        err = (a - b.detach()).abs().max().item() / b.detach().abs().max().item()
        assert err <= 1e-12, (op, kind, name, err)


def test_tail_statistics_are_instance_norm():
    f = E.Row('host_tail_in', 'tail', 'plain', (2, 3, 4, 5, 6), 3, '', [], '')
    y, mean, rstd = f.ref(f, X.to_f64(X.draw(f, 'randn')))
    want = torch.nn.functional.instance_norm(y, eps=E.EPS)
    assert ((y - mean[:, :, None, None]) * rstd[:, :, None, None] - want).abs().max().item() <= 1e-12


def kernels_defined():
    names = set()
    for src in SOURCES:
        with open(os.path.join(CSRC, src)) as fh:
            text = fh.read()
        found = re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)\s*\(', text)       # (launch bounds may span lines and nest)
        assert found, src
        names.update(found)
    return names


def test_every_kernel_of_the_family_has_a_row():
    names = kernels_defined()
    assert len(names) >= 36 and 'conv_fwd_kernel' in names and 'conv_s2_wgrad_roll2_kernel' in names, sorted(names)
    launched = {re.match(r'\w+', sym).group(0) for r in E.ROWS.values() for sym, _ in r.plan}
    unreached = {re.match(r'\w+', sym).group(0) for sym, _ in E.UNREACHED}
    missing = sorted(names - launched - unreached - set(E.NOT_CONV))
    assert not missing, missing
    stale = sorted((launched | set(E.NOT_CONV)) - names)
    assert not stale, stale
    assert not launched & set(E.NOT_CONV)


# the kernel forms the table must hold, by the template arguments that select another body
FORMS_WANTED = [
    'conv_fwd_kernel<FwdCfg<3, 2, 5, 3, 0, 1>, false, false, false, false>', 'conv_fwd_kernel<FwdCfg<3, 2, 4, 4, 0, 1>, false',
    'conv_fwd_kernel<FwdCfg<3, 2, 4, 4, 0, 2>, false', 'conv_fwd_kernel<FwdCfg<3, 1, 5, 3, 0, 0>, false',
    'conv_fwd_kernel<FwdCfg<3, 1, 3, 3, 2, 0>, false', 'conv_fwd_kernel<FwdCfg<3, 1, 2, 2, 4, 0>, false',
    'conv_fwd_kernel<FwdCfg<3, 4, 4, 3, 0, 1>, false, false, false, false>', 'conv_fwd_kernel<FwdCfg<3, 2, 5, 3, 0, 1>, true',
    'conv_fwd_kernel<FwdCfg<3, 1, 3, 3, 2, 0>, false, true', 'conv_fwd_kernel<FwdCfg<3, 1, 4, 4, 0, 1>, false, true',
    'conv_fwd_kernel<FwdCfg<1, 1, 0, 0, 6, 0>, false, true', 'false, false, true, false>', 'false, false, true, true>',
    'conv_fwd_strip_kernel<FwdCfg<3, 1, 4, 4, 0, 2>>', 'conv_fwd_strip_kernel<FwdCfg<1, 1, 5, 3, 0, 1>>',
    'conv_fwd_strip2_kernel<FwdCfg<3, 1, 5, 3, 0, 1>>', 'conv_fwd_strip2_kernel<FwdCfg<3, 1, 4, 4, 0, 1>>',
    'conv_fwd_roll2_kernel', 'conv_fwd_roll_blur_kernel<1>', 'conv_fwd_roll_blur_kernel<2>', 'rb_rgb_finish_kernel',
    'conv_wgrad_kernel<WgCfg<3, 2, 1, 4, 5, 3, 0, 1>, false>', 'conv_wgrad_kernel<WgCfg<3, 1, 1, 4, 3, 3, 2, 0>, false>',
    'conv_wgrad_kernel<WgCfg<3, 2, 4, 1, 3, 3, 0, 1>, false>', 'conv_wgrad_kernel<WgCfg<3, 2, 4, 1, 3, 3, 0, 1>, true>',
    'wgrad_reduce_kernel', 'conv_wgrad_roll_kernel<false>', 'conv_wgrad_roll_kernel<true>',
    'pw_few_to_many_kernel', 'pw_many_to_few_kernel', 'pw_cross_sums_kernel', 'pw_cross_finish_kernel', 'splitk_finish_kernel',
    'conv_s2_down_kernel<SCfg<2, 5, 4>>', 'conv_s2_down_kernel<SCfg<4, 4, 2>>', 'conv_s2_up_kernel<TCfg<2, 2>, false>',
    'conv_s2_up_kernel<TCfg<1, 4>, false>', 'conv_s2_up_kernel<TCfg<2, 2>, true>', 'conv_s2_wgrad_kernel<WCfg<2>>',
    'reduce_s2_slots_kernel', 'fold_s2_kernel', 'conv_s2_down_roll_kernel', 'conv_s2_up_roll_kernel<false>',
    'conv_s2_up_roll_blur_kernel<0, true>', 'conv_s2_up_roll_blur_kernel<1, false>', 'tb_stats_finish_kernel', 'tb_sum_finish_kernel',
    'conv_s2_wgrad_roll2_kernel<1, false>', 'conv_s2_wgrad_roll2_kernel<2, false>', 'conv_s2_wgrad_roll2_kernel<2, true>',
    'conv_fwd_rollmod_kernel', 'rm_stats_finish_kernel', 'conv_tail_stats_finish_kernel',
]


def test_table_holds_every_form_the_issue_names():
    have = [E.norm(sym) for r in E.ROWS.values() for sym, _ in r.plan]
    for want in FORMS_WANTED:
        assert any(E.norm(want) in h for h in have), want


@pytest.mark.parametrize('name', list(E.ROWS))
def test_row_plan_is_positive_and_claims_hold(name):
    r = E.ROWS[name]
    assert r.plan and r.symbol == r.plan[0][0] and r.edge
    for sym, grid in r.plan:
        assert isinstance(grid, int) and 0 < grid < 2 ** 31, (name, sym, grid)
    for what, (got, want) in r.claims.items():
        assert got == want, (name, what, got, want)
    if 'two' in r.edge and 'strips' in name:
        assert 'strips' in r.claims, name


def test_named_edges_of_the_plans():
    # rb_plan: a second strip at 17 steps (blur: 32); wr_plan: two units per workgroup only beyond 768 / (tiles_ci * tiles_co)
    assert E.rb_plan(1, 56, 64, 0)[1] == 1 and E.rb_plan(1, 64, 64, 0)[1:3] == (2, 8) and E.rb_plan(1, 68, 64, 0)[1:3] == (2, 9)
    assert E.rb_plan(1, 120, 64, 1)[1] == 1 and E.rb_plan(1, 128, 64, 1)[1:3] == (2, 16) and E.rb_plan(1, 132, 64, 1)[1:3] == (2, 17)
    assert E.wr_plan(12, 24, 20, 68, 512)['units_per_wg'] == 1 and E.wr_plan(13, 24, 20, 68, 512)['units_per_wg'] == 2
    assert E.splitk_plan(4, 1040, 16, 1, 1, 1) == 7 and E.splitk_plan(4, 1024, 16, 1, 1, 1) == 8
    # the non-finite rows exist and their pixel lies inside the poisoned operand
    for name, (py, px) in E.NONFINITE:
        r = E.ROWS[name]
        h, w = r.hw_out if r.role == 'dgrad' else r.hw_in
        assert py < h and px < w, (name, py, px, h, w)
