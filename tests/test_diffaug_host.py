"""Host-side tests of DiffAugment (gan_lab_amd/augment.py): policy parsing, the config option and its CLI flag, and the
per-resolution translation / cutout sizes of the transform (DESIGN.md "DiffAugment")."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARTS = ('color', 'translation', 'cutout')


def _subsets():
    for k in range(1, 4):
        for combo in itertools.combinations(range(3), k):
            yield ','.join(PARTS[i] for i in combo), sum(1 << i for i in combo)


def test_every_ordered_subset_parses_to_its_bit_mask():
    from gan_lab_amd import augment
    got = {p: augment.parse_policy(p) for p, _ in _subsets()}
    assert got == dict(_subsets()) and len(got) == 7
    assert augment.parse_policy('color,translation,cutout') == augment.COLOR | augment.TRANSLATION | augment.CUTOUT


@pytest.mark.parametrize('bad', ['', 'colour', 'Color', 'color,', ',color', 'color translation', 'color, translation',
                                 'color,color', 'cutout,cutout', 'translation,color', 'cutout,translation',
                                 'color,cutout,translation', 'color,translation,cutout,color', 'none'])
def test_bad_policies_are_rejected(bad):
    from gan_lab_amd import augment
    with pytest.raises(ValueError):
        augment.parse_policy(bad)
    with pytest.raises(ValueError):
        augment.DiffAugment(bad)


def test_non_string_policy_is_rejected():
    from gan_lab_amd import augment
    for bad in (None, 3, ['color']):
        with pytest.raises(ValueError):
            augment.parse_policy(bad)
    assert augment.from_config(None) is None
    assert augment.from_config('translation,cutout').mask == augment.TRANSLATION | augment.CUTOUT


@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_default_and_override(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    assert make_config(model, **kw).diffaugment is None
    assert make_config(model, diffaugment='color,cutout', **kw).diffaugment == 'color,cutout'


def test_config_cli_flag(monkeypatch, tmp_path):
    from gan_lab_amd import config
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['stylegan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    assert config.main(args).diffaugment is None
    assert config.main(args + ['--diffaugment=color,translation,cutout']).diffaugment == 'color,translation,cutout'
    assert config.main(args + ['--diffaugment', 'translation']).diffaugment == 'translation'


def test_learner_validates_the_policy(monkeypatch):
    """A bad policy fails when the learner is built, before any step."""
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    cfg = make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                      diffaugment='cutout,color')
    with pytest.raises(ValueError):
        GANLearner(cfg)


@pytest.mark.parametrize('h', [4, 8, 16, 32, 64, 128, 256, 512, 1024])
def test_translation_and_cutout_sizes(h):
    """sh = int(0.125 H + 0.5), ch = int(0.5 H + 0.5); ox in [0, H + 1 - ch % 2) (the official DiffAugment definition)."""
    from gan_lab_amd import augment
    w = h // 2 if h >= 8 else h
    sh, sw, ch, cw = augment.sizes(h, w)
    assert (sh, sw) == (int(h * 0.125 + 0.5), int(w * 0.125 + 0.5))
    assert (ch, cw) == (int(h * 0.5 + 0.5), int(w * 0.5 + 0.5))
    assert sh == {4: 1, 8: 1, 16: 2, 32: 4, 64: 8, 128: 16, 256: 32, 512: 64, 1024: 128}[h]
    assert ch == h // 2
    # the range of ox and the rows a cut covers: every cut stays a (clipped) rectangle that meets the image
    n_ox = h + 1 - ch % 2
    for ox in range(n_ox):
        r0, r1 = ox - ch // 2, ox - ch // 2 + ch
        assert r1 > 0 and r0 < h
        assert max(r0, 0) < min(r1, h)
    assert augment.sizes(5, 12) == (1, 2, 3, 6)
