"""Host-side tests of ADA (gan_lab_amd/ada.py): policy parsing, the config options and their CLI flags, the exclusion of
DiffAugment, the controller's adjustment rule restated on the host, the accumulator reduction over two gloo ranks, and the
checkpoint's config filter (DESIGN.md "ADA")."""
import itertools
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARTS = ('blit', 'geom', 'color')


def _subsets():
    for k in range(1, 4):
        for combo in itertools.combinations(range(3), k):
            yield ','.join(PARTS[i] for i in combo), sum(1 << i for i in combo)


def test_every_ordered_subset_parses_to_its_bit_mask():
    from gan_lab_amd import ada
    got = {p: ada.parse_policy(p) for p, _ in _subsets()}
    assert got == dict(_subsets()) and len(got) == 7
    assert ada.parse_policy('blit,geom,color') == ada.BLIT | ada.GEOM | ada.COLOR
    assert (ada.BLIT, ada.GEOM, ada.COLOR) == (1, 2, 4)


@pytest.mark.parametrize('bad', ['', 'bilt', 'Blit', 'blit,', ',blit', 'blit geom', 'blit, geom', 'blit,blit', 'color,color',
                                 'geom,blit', 'color,geom', 'blit,color,geom', 'blit,geom,color,blit', 'none', 'bgc',
                                 'translation'])
def test_bad_policies_are_rejected(bad):
    from gan_lab_amd import ada
    with pytest.raises(ValueError):
        ada.parse_policy(bad)
    with pytest.raises(ValueError):
        ada.AdaptiveAugment(bad, device='cpu')


def test_non_string_policy_and_bad_numbers_are_rejected():
    from gan_lab_amd import ada
    for bad in (None, 3, ['blit']):
        with pytest.raises(ValueError):
            ada.parse_policy(bad)
    for kw in (dict(p=-0.1), dict(p=1.5), dict(interval=0), dict(kimg=0)):
        with pytest.raises(ValueError):
            ada.AdaptiveAugment('blit', device='cpu', **kw)
    a = ada.AdaptiveAugment('geom,color', p=0.25, target=None, device='cpu')
    assert a.mask == ada.GEOM | ada.COLOR and not a.adaptive and a.p == 0.25
    assert a.state.tolist() == [0.25, 0.0, 0.0, 0.0]


@pytest.mark.parametrize('model', ['stylegan', 'progan', 'resnetgan'])
def test_config_defaults_and_overrides(model):
    from gan_lab_amd.config import make_config
    kw = dict(dev='cpu', pin_memory=False)
    c = make_config(model, **kw)
    assert (c.ada, c.ada_p, c.ada_target, c.ada_interval, c.ada_kimg) == (None, 0.0, 0.6, 4, 500)
    c = make_config(model, ada='blit,color', ada_p=0.3, ada_target=None, ada_interval=2, ada_kimg=100, **kw)
    assert (c.ada, c.ada_p, c.ada_target, c.ada_interval, c.ada_kimg) == ('blit,color', 0.3, None, 2, 100)


def test_config_cli_flags(monkeypatch, tmp_path):
    from gan_lab_amd import config
    monkeypatch.setenv('HOME', str(tmp_path))
    monkeypatch.setattr(config, '_HERE', str(tmp_path))
    args = ['stylegan', '--dev=cpu', '--pin_memory=False', f'--save_samples_dir={tmp_path}/s', f'--save_model_dir={tmp_path}/m']
    c = config.main(args)
    assert (c.ada, c.ada_p, c.ada_target, c.ada_interval, c.ada_kimg) == (None, 0.0, 0.6, 4, 500)
    c = config.main(args + ['--ada=blit,geom,color', '--ada_p=0.2', '--ada_target=0.5', '--ada_interval', '8',
                            '--ada_kimg=100'])
    assert (c.ada, c.ada_p, c.ada_target, c.ada_interval, c.ada_kimg) == ('blit,geom,color', 0.2, 0.5, 8, 100)
    assert config.main(args + ['--ada', 'geom', '--ada_target=none']).ada_target is None


def _resnet_cfg(**kw):
    from gan_lab_amd.config import make_config
    return make_config('resnetgan', dev='cpu', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4, **kw)


def test_learner_validates_the_policy_and_rejects_both_augmentations(monkeypatch):
    """A bad policy, and ``ada`` together with ``diffaugment``, fail when the learner is built, before any step."""
    from gan_lab_amd import ada
    from gan_lab_amd.resnetgan.learner import GANLearner
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    with pytest.raises(ValueError):
        GANLearner(_resnet_cfg(ada='color,blit'))
    with pytest.raises(ValueError, match='diffaugment'):
        GANLearner(_resnet_cfg(ada='blit', diffaugment='color'))
    L = GANLearner(_resnet_cfg(ada='blit,geom', ada_p=0.125, ada_target=None))
    assert isinstance(L.ada, ada.AdaptiveAugment) and L.critic_aug is L.ada and L.diffaug is None
    assert L.ada.p == 0.125 and not L.ada.adaptive
    L = GANLearner(_resnet_cfg())
    assert L.ada is None and L.critic_aug is None
    L = GANLearner(_resnet_cfg(diffaugment='color'))
    assert L.ada is None and L.critic_aug is L.diffaug


def test_next_p_moves_one_step_towards_the_target_and_clamps():
    from gan_lab_amd import ada
    f = np.float32
    step = ada.step_size(32, 1, 4, 500)
    assert step == 32 * 4 / 500000
    up, down = float(f(f(0.5) + f(step))), float(f(f(0.5) - f(step)))
    assert ada.next_p(0.5, 100, 128, 0.6, step) == up          # r = 0.78 > 0.6: more augmentation
    assert ada.next_p(0.5, 10, 128, 0.6, step) == down         # r = 0.08 < 0.6: less
    assert ada.next_p(0.5, -128, 128, 0.6, step) == down
    assert ada.next_p(0.5, 64, 128, 0.5, step) == 0.5          # on target: no move
    assert ada.next_p(0.5, 0, 0, 0.6, step) == 0.5             # no samples: no move
    # clamping at both ends, also when the step overshoots
    assert ada.next_p(0.0, -5, 8, 0.6, step) == 0.0
    assert ada.next_p(1.0, 8, 8, 0.6, step) == 1.0
    assert ada.next_p(0.9, 8, 8, 0.6, 0.25) == 1.0
    assert ada.next_p(0.1, -8, 8, 0.6, 0.25) == 0.0
    # the arithmetic is fp32, as on the device: repeated steps do not drift from a float32 accumulation
    p, q = 0.0, f(0)
    for _ in range(1000):
        p = ada.next_p(p, 1, 1, 0.0, step)
        q = f(q + f(step))
    assert p == float(q)
    # the paper's step: kimg thousand images move p from 0 to 1
    assert abs(ada.step_size(64, 8, 4, 500) * (500000 / (64 * 8 * 4)) - 1) < 1e-12


def test_rows_from_matrices_carry_the_inverse():
    from gan_lab_amd import ada
    M = torch.tensor([[[1.0, 0, 0], [0, 1, 0]], [[0.5, -0.25, 3.0], [0.25, 0.5, -2.0]], [[0.0, -1, 1.0], [1, 0, 0]]])
    C = torch.arange(36, dtype=torch.float32).reshape(3, 3, 4)
    rows = ada.rows_from_matrices(M, C)
    assert rows.shape == (3, ada.ROW) and rows.dtype == torch.float32
    assert torch.equal(rows[:, :6], M.reshape(3, 6)) and torch.equal(rows[:, 10:22], C.reshape(3, 12))
    G = rows[:, 6:10].reshape(3, 2, 2).double()
    assert torch.allclose(G @ M[:, :, :2].double(), torch.eye(2, dtype=torch.float64).expand(3, 2, 2), atol=1e-6)
    assert torch.equal(rows[2, 6:10], torch.tensor([0.0, 1, -1, 0]))      # a quarter turn inverts exactly
    assert (rows[:, 22:] == 0).all()
    ident = ada.rows_from_matrices(M[:1])
    assert torch.equal(ident[0, 10:22], torch.eye(3, 4).reshape(-1))


# ------------------------------------------------------------------------------------------------------------------- #
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from gan_lab_amd import ada
        # rank 0 saw mostly positive critic outputs, rank 1 mostly negative ones: alone they would move p in opposite directions
        state = torch.tensor([0.5, 30.0, 32.0, 4.0]) if rank == 0 else torch.tensor([0.5, -20.0, 32.0, 4.0])
        alone = ada.next_p(state[0], state[1], state[2], 0.6, 0.01)
        ada.reduce_accumulators(state)
        p = ada.next_p(state[0], state[1], state[2], 0.6, 0.01)
        q.put((rank, alone, state.tolist(), p))
    finally:
        dist.destroy_process_group()


def test_accumulators_are_summed_over_two_gloo_ranks():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0, f'worker exit code {p.exitcode}'
    got = dict((r, rest) for r, *rest in (q.get(timeout=10) for _ in range(2)))
    assert got[0][0] > 0.5 > got[1][0]                       # alone, the ranks disagree
    for r in (0, 1):                                         # p and the call counter are left alone, the sums are global
        assert got[r][1] == [0.5, 10.0, 64.0, 4.0]
    f = np.float32
    assert got[0][2] == got[1][2] == float(f(f(0.5) - f(0.01)))     # 10 / 64 < 0.6: both step down


def test_reduce_is_a_no_op_in_a_single_process():
    from gan_lab_amd import ada
    s = torch.tensor([0.25, 3.0, 8.0, 1.0])
    assert ada.reduce_accumulators(s) is s and s.tolist() == [0.25, 3.0, 8.0, 1.0]


# ------------------------------------------------------------------------------------------------------------------- #
def test_saved_config_has_no_ada_key_while_ada_is_off():
    from gan_lab_amd import checkpoint
    from gan_lab_amd.config import make_config
    for model in ('stylegan', 'progan', 'resnetgan'):
        off = vars(make_config(model, dev='cpu', pin_memory=False))
        assert {'ada', 'ada_p', 'ada_target', 'ada_interval', 'ada_kimg'} <= set(off)
        kept = checkpoint.saved_config_fields(dict(off))
        assert not [k for k in kept if k.startswith('ada')]
        assert kept == {k: v for k, v in off.items() if not k.startswith('ada')}      # nothing else is touched
        on = vars(make_config(model, dev='cpu', pin_memory=False, ada='blit', ada_target=None))
        kept = checkpoint.saved_config_fields(dict(on))
        assert kept == on and kept['ada'] == 'blit' and kept['ada_target'] is None


def test_config_filter_keeps_fields_that_merely_start_alike():
    """Only ``ada`` and ``ada_*`` are this option's fields: ``adam_beta`` and the like stay."""
    from gan_lab_amd import checkpoint
    cfg = checkpoint.saved_config_fields({'ada': None, 'ada_p': 0.0, 'ada_target': 0.6, 'ada_interval': 4, 'ada_kimg': 500.0,
                                          'adam_beta': 0.9, 'lr_base': 0.001})
    assert cfg == {'adam_beta': 0.9, 'lr_base': 0.001}
