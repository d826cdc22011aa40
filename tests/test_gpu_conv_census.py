"""Replay of the dispatch census (tests/conv_census.py) against tests/golden/conv_census.json, which was recorded from the
commit before ``ops.conv_route`` and the pack table existed: every row must launch exactly the kernels, with exactly the grids,
that the per-launcher chains launched - on its first call (weight pack included) and in the steady state - and
``ops.conv_route`` must name the family those kernels belong to."""
import pytest
import torch

import conv_census as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gan_lab_amd import ops as _ops, _lib
    _lib.lib()
    return _ops


@pytest.fixture(scope='module')
def recorded():
    return C.load()


def test_fixture_has_every_row(recorded):
    assert sorted(recorded) == sorted(r[0] for r in C.ROWS) and len(recorded) == len(C.ROWS)


@pytest.mark.parametrize('row', C.ROWS, ids=lambda r: r[0])
def test_row_launches_what_was_recorded(ops, recorded, row):
    first, second = C.run(ops, row)
    want_first, want_second = recorded[row[0]]
    assert second == want_second, (row[0], second, want_second)
    assert first == want_first, (row[0], first, want_first)
    assert ops.conv_route(C.geom_of(ops, row), row[1]) == C.family_of(row, second), (row[0], second)


def test_census_reaches_every_family_and_pack_row(ops, recorded):
    """A condition on the table: a family or a packed layout that no row reaches is not pinned by the replay."""
    families = {C.family_of(row, recorded[row[0]][1]) for row in C.ROWS}
    assert families == set(C.FAMILIES) == {ops.BF16, ops.X3, ops.X3_UP, ops.X3_DOWN, ops.S2, ops.LINEAR, ops.F32}
    packs = set().union(*(C.pack_rows_of(recorded[row[0]][0]) for row in C.ROWS))
    assert packs == set(ops._PACK_ROWS) == set(C.PACK_SYMBOL_ROW.values())
