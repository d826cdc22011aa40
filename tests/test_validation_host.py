"""The single table of the learners' set metrics (gan_lab_amd/validation.py): its names, the config fields a
reference-format checkpoint keeps per row, and the metric modules' ``wanted`` against the shared helper.  Runs without a GPU."""
import pytest

NAMES = ('swd', 'msssim', 'spectrum', 'prdc', 'fd', 'kid', 'ppl')


def test_the_table_holds_exactly_the_seven_in_report_order():
    from gan_lab_amd import validation
    assert tuple(s.name for s in validation.SCORERS) == NAMES == validation.NAMES
    assert tuple(s.name for s in validation.FEED_ORDER) == ('swd', 'spectrum', 'prdc', 'fd', 'kid', 'ppl', 'msssim')
    assert tuple(s.name for s in validation.ROW_SCORERS) == ('prdc', 'fd', 'kid')
    assert [s.name for s in validation.SCORERS if s.reals == 'required'] == ['swd', 'spectrum', 'prdc', 'fd', 'kid']
    assert validation.uses_reals(['generator loss', 'MSSSIM']) and not validation.uses_reals(['generator loss', 'ppl']) and \
        not validation.uses_reals(None)


@pytest.mark.parametrize('name', NAMES)
def test_reference_format_checkpoint_keeps_a_rows_fields_only_while_its_metric_is_on(name):
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    for model in ('stylegan', 'progan'):
        off = make_config(model, dev='cpu', pin_memory=False)
        mine = sorted(k for k in vars(off) if k.startswith(name + '_'))
        assert mine                                          # every row has config fields of its own
        assert not [k for k in checkpoint.reference_config_fields(off) if k.startswith(tuple(n + '_' for n in NAMES))]
        kept = checkpoint.reference_config_fields(make_config(model, dev='cpu', pin_memory=False, gen_metrics=['generator loss', name.upper()]))
        assert sorted(k for k in kept if k.startswith(tuple(n + '_' for n in NAMES))) == mine


@pytest.mark.parametrize('name', NAMES)
def test_each_modules_wanted_is_the_shared_helper(name):
    from gan_lab_amd import _metric_common, validation
    (scorer,) = [s for s in validation.SCORERS if s.name == name]
    other = NAMES[(NAMES.index(name) + 1) % len(NAMES)]
    for metrics in (None, [], (), [name], (name.upper(),), ['generator loss', name.capitalize()], [other], [name + 's', 3, None],
                    ['Generator Loss', other.upper()]):
        got = scorer.module.wanted(metrics)
        assert got is _metric_common.wanted(metrics, name) and got == any(isinstance(m, str) and m.casefold() == name
                                                                         for m in (metrics or ()))
