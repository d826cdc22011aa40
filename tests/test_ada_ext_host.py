"""Host-side tests of ADA's filter, noise and cutout groups (gan_lab_amd/ada.py): policy parsing, the filter bank's
properties, hand-made ext rows and the config round trip.  No GPU."""
import numpy as np
import pytest
import torch

SIX = 'blit,geom,color,filter,noise,cutout'


def test_policy_parsing_knows_the_new_groups():
    from gan_lab_amd import ada
    assert (ada.FILTER, ada.NOISE, ada.CUTOUT) == (8, 16, 32)
    assert ada.parse_policy(SIX) == 63
    assert ada.parse_policy('filter') == 8 and ada.parse_policy('noise') == 16 and ada.parse_policy('cutout') == 32
    assert ada.parse_policy('blit,filter,cutout') == 1 | 8 | 32
    assert ada.parse_policy('blit,geom,color') == 7                 # as before
    for bad in ('filter,color', 'blit,cutout,filter', 'cutout,noise', 'noise,filter', 'filter,filter',
                'blit,geom,color,filter,noise,cutout,blit', 'Filter', 'filter, noise', 'cut', '', 'filter,'):
        with pytest.raises(ValueError):
            ada.parse_policy(bad)


def test_filter_bank_properties():
    """(4, 43), every row symmetric, the rows sum to the unit impulse at tap 21 within 7e-16, row 0 sums to 1 and the others
    to 0; sum |h| over the corners of the +-3 clamp of the band draws stays below 8.21."""
    import itertools
    from gan_lab_amd import ada
    bank = ada.filter_bank()
    assert bank.dtype == torch.float64 and tuple(bank.shape) == (4, 43)
    b = bank.numpy()
    assert np.abs(b - b[:, ::-1]).max() <= 1e-16
    assert np.abs(b.sum(0) - np.eye(43)[21]).max() <= 7e-16
    assert np.abs(b.sum(1) - np.array([1.0, 0, 0, 0])).max() <= 1e-15
    e, worst = np.array([10.0, 1, 1, 1]) / 13, 0.0
    for z in itertools.product((-3.0, 0.0, 3.0), repeat=4):
        g = np.ones(4)
        for i in range(4):
            t = np.ones(4)
            t[i] = 2.0 ** z[i]
            g *= t / np.sqrt((e * t * t).sum())
        worst = max(worst, np.abs(g @ b).sum())
    assert 8.0 < worst <= 8.21


def test_ext_rows_by_hand():
    from gan_lab_amd import ada
    rows = ada.ext_rows(g=[[1, 2, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]], sigma=[0, 0.1, 0],
                        rect=[[0, 0, 0, 0], [1, 3, 2, 4], [2, 2, 0, 4]])
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (3, ada.EXT_ROW) and ada.EXT_ROW == 16
    assert rows[:, 9].tolist() == [15.0, 48.0, 0.0]
    assert rows[1, 4].item() == np.float32(0.1) and rows[1, 5:9].tolist() == [1.0, 3.0, 2.0, 4.0]
    assert rows[:, 10:].abs().max() == 0
    forced = ada.ext_rows(gates=[1, 0], n=2)
    assert forced[:, 9].tolist() == [1.0, 0.0] and torch.equal(forced[:, :4], torch.ones(2, 4))
    assert tuple(ada.ext_rows(n=5).shape) == (5, 16)


def test_config_round_trip_of_a_six_part_policy():
    from gan_lab_amd import ada, checkpoint
    from gan_lab_amd.config import make_config
    cfg = make_config('resnetgan', dev='cpu', ada=SIX, ada_p=0.5, ada_target=None)
    assert cfg.ada == SIX and ada.parse_policy(cfg.ada) == 63
    kept = checkpoint.saved_config_fields(dict(vars(cfg)))          # what a checkpoint stores of the config
    again = make_config('resnetgan', **{k: kept[k] for k in ('dev', 'ada', 'ada_p', 'ada_target')})
    assert again.ada == SIX and again.ada_p == 0.5 and again.ada_target is None


def test_ada_plus_diffaugment_still_raises():
    from gan_lab_amd import ada
    from gan_lab_amd.config import make_config
    cfg = make_config('resnetgan', dev='cpu', ada=SIX, diffaugment='color,translation,cutout')
    with pytest.raises(ValueError, match='diffaugment'):
        ada.from_config(cfg)
