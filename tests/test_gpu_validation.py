"""The learners' set metrics evaluated together (ProGANLearner.compute_metrics): all seven in one call must give,
for every name, exactly what a call with that name alone gives - the same ``last_metrics`` entry and the same lines, in the report
order 'swd', 'msssim', 'spectrum', 'prdc', 'fd', 'kid', 'ppl'.  ProGAN draws no per-layer noise, so the images each metric scores
do not depend on what else is evaluated: equality is bitwise unless the shared per-batch loop lets one metric disturb another.

Sizes: batch 4, 12 latents and 8 reals, so the sets compared hold two whole batches and 'msssim fake' a third one; 16x16 is the
smallest resolution at which 'swd', 'msssim' and 'spectrum' have a level, 8x8 the one below it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SET_METRICS = ['swd', 'msssim', 'spectrum', 'prdc', 'fd', 'kid', 'ppl']


def _learner(monkeypatch, res, **kw):
    from gan_lab_amd import progressive as P
    from test_gpu_learner import make_learner
    monkeypatch.setattr(P, 'FMAP_BASE', 64)
    monkeypatch.setattr(P, 'FMAP_MAX', 16)
    torch.manual_seed(7)
    return make_learner('progan', res, init_res=res, batch=4, gen_metrics=['generator loss'] + SET_METRICS, disc_metrics=[],
                        random_seed=4, swd_nhoods=8, swd_dir_repeats=1, swd_dirs_per_repeat=16, prdc_k=3, prdc_res=8, fd_res=4,
                        kid_res=8, kid_block=4, ppl_samples=8, **kw)


def _same(a, b):
    """Exact equality of the nested results, a NaN equal to a NaN."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):          # 'ppl' keeps its per-sample distances on the device
        return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (a.isnan() & b.isnan())).all())
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def _parsed(lines):
    """(name, printed value) per line: the column width depends on the longest name of the call, the rest does not."""
    return [tuple(part.strip() for part in ln.split(':', 1)) for ln in lines]


def _together_and_alone(L, z_dl, x_dl):
    lines = _parsed(L.compute_metrics(['generator loss'] + SET_METRICS, 'Generator', z_dl, x_dl))
    together = dict(L.last_metrics['generator'])
    assert lines[0][0] == 'generator loss' and set(together) == {'generator loss'} | set(SET_METRICS)
    alone, alone_lines = {}, []
    for name in SET_METRICS:
        got = _parsed(L.compute_metrics([name], 'Generator', z_dl, x_dl))
        assert set(L.last_metrics['generator']) == {name}
        alone[name] = L.last_metrics['generator'][name]
        alone_lines.append(got)
        print(name, got)
    for name in SET_METRICS:
        assert _same(together[name], alone[name]), name
    assert lines[1:] == [ln for got in alone_lines for ln in got]             # the same lines, in the report order
    return together, dict(zip(SET_METRICS, alone_lines))


@pytest.mark.parametrize('use_ewma_gen', [False, True])
def test_all_metrics_together_equal_each_alone_at_16(monkeypatch, use_ewma_gen):
    from test_gpu_prdc import _fixed_loaders
    L = _learner(monkeypatch, 16, use_ewma_gen=use_ewma_gen)
    z_dl, x_dl = _fixed_loaders(4, 16, 16)
    if use_ewma_gen:                                         # the time-averaged generator, which the set metrics score, is another one
        with torch.no_grad():
            L.ewma.flat.mul_(0.75)
    got, lines = _together_and_alone(L, z_dl, x_dl)
    assert [n for n, _ in lines['swd']] == ['swd 16x16', 'swd mean'] and [n for n, _ in lines['msssim']] == ['msssim fake', 'msssim real']
    assert [n for n, _ in lines['spectrum']] == ['spectrum', 'spectrum hf']
    assert (got['msssim']['pairs'], got['msssim']['real']['pairs'], got['spectrum']['images']) == (6, 4, 8)
    assert (got['prdc']['n_fake'], got['fd']['n_real'], got['kid']['blocks']) == (8, 8, 2)
    for name, key in (('swd', 'mean'), ('msssim', 'msssim'), ('spectrum', 'spectrum'), ('fd', 'fd'), ('kid', 'kid'), ('ppl', 'ppl')):
        assert math.isfinite(got[name][key]), name
    assert L.gen_model.training and L.disc_model.training


def test_all_metrics_together_equal_each_alone_at_8(monkeypatch):
    from test_gpu_prdc import SCORES, _fixed_loaders
    L = _learner(monkeypatch, 8, use_ewma_gen=True)
    z_dl, x_dl = _fixed_loaders(4, 8, 16)
    got, lines = _together_and_alone(L, z_dl, x_dl)
    for name, key in (('swd', 'mean'), ('msssim', 'msssim'), ('spectrum', 'spectrum')):
        assert math.isnan(got[name][key])
        ((line_name, text),) = lines[name]
        assert line_name == name and text.startswith('nan (') and '16x16' in text and '8x8' in text
    assert [n for n, _ in lines['prdc']] == list(SCORES) and [lines[n][0][0] for n in ('fd', 'kid', 'ppl')] == ['fd', 'kid', 'ppl']
    for name, key in (('prdc', 'precision'), ('fd', 'fd'), ('kid', 'kid'), ('ppl', 'ppl')):
        assert math.isfinite(got[name][key]) and math.isfinite(float(lines[name][0][1])), name


def test_unequal_batches_name_the_first_metric_with_images_to_go(monkeypatch):
    from test_gpu_prdc import _fixed_loaders
    L = _learner(monkeypatch, 16, use_ewma_gen=False)
    z_dl = _fixed_loaders(4, 16, 16)[0]                      # 12 latents in batches of 4
    x_dl = _fixed_loaders(2, 16, 16, n_x_batches=4)[1]       # 8 reals in batches of 2
    with pytest.raises(ValueError, match=r"^'kid': validation latents and reals must come in equal batches \(got 4 and 2 with 8 "):
        L.compute_metrics(['kid', 'msssim'], 'Generator', z_dl, x_dl)
    with pytest.raises(ValueError, match=r"^'msssim': validation latents and reals must come in equal batches \(got 4 and 2 with 8 "):
        L.compute_metrics(['msssim'], 'Generator', z_dl, x_dl)
    assert L.gen_model.training and L.disc_model.training
