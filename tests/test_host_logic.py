"""CPU tests of the host-side logic: phase machine vs the trace of the REAL reference learner,
config / LearnerConfigCopy behaviour, C-ABI surface.  No GPU, no compute kernels."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_phase_schedule_matches_reference_trace():
    from gan_lab_amd.schedule import FINAL, GROW, STABILISE, PhaseSchedule, ewma_beta
    g = load_golden('schedule_progan_4to16.npz')
    cols = [str(c) for c in g['columns']]
    tr = g['trace']
    bs_dict = {int(k): int(v) for k, v in g['bs_dict']}
    lr_fctr = {int(k): float(v) for k, v in g['lr_fctr']}
    ps = PhaseSchedule(4, 16, bs_dict, int(g['cfg_nimg_transition']), num_disc_iters=1)
    saw = []
    for row in tr:
        r = dict(zip(cols, row))
        ev = ps.begin_iter()
        saw += ev
        ps.after_d_iter()                      # one D iteration
        # state seen by the G-step of this main iteration
        assert ps.curr_res == int(r['curr_res']), r
        assert int(ps.fade_in_phase) == int(r['fade_in']), r
        assert abs(ps.alpha - r['alpha']) < 1e-9, r
        assert ps.batch_size == int(r['batch']), r
        assert ps.curr_phase_num == int(r['phase_num']), r
        assert ps.curr_img_num == int(r['curr_img_num_after_dstep']), r
        assert abs(1e-3 * lr_fctr[ps.curr_res] - r['lr_gen']) < 1e-12
        ps.end_iter()
    assert saw == [GROW, STABILISE, GROW, FINAL]
    ref_lst = [x if x >= 0 else math.inf for x in g['nimg_transition_lst']]
    assert ps.nimg_transition_lst == ref_lst
    assert abs(ewma_beta(ps.batch_size) - float(g['final_beta'])) < 1e-15
    # the real-image stream the reference consumed: (batch, resolution) per D iteration
    assert [tuple(x) for x in g['real_batches']] == [(int(r[4]), int(r[1])) for r in tr]


def test_schedule_known_answers():
    from gan_lab_amd.schedule import delta_alpha, ewma_beta, round_nimg_transition
    assert round_nimg_transition(600000, 64) == 600000
    assert round_nimg_transition(600000, 7) == 7 * (600000 // 7 + 1)
    assert delta_alpha(64, 600000, 1) == 64 / (600000 - 64)
    assert abs(ewma_beta(32) - 0.5 ** (32 / 10000)) < 1e-15
    assert ewma_beta(32, half_life=0.) == 0.


def test_schedule_counts_global_images_under_data_parallel():
    """W ranks at per-rank batch B walk the same schedule, in images and in alpha, as one process at batch W*B
    (``nimg_transition`` counts real images; reference: progan/learner.py:646-653, :848)."""
    from gan_lab_amd.schedule import PhaseSchedule
    bs1 = {4: 8, 8: 8, 16: 4}
    bs2 = {4: 16, 8: 16, 16: 8}
    a = PhaseSchedule(4, 16, bs1, 100, num_disc_iters=1, world_size=2)
    b = PhaseSchedule(4, 16, bs2, 100, num_disc_iters=1, world_size=1)
    for _ in range(60):
        assert a.begin_iter() == b.begin_iter()
        a.after_d_iter(), b.after_d_iter()
        assert (a.curr_img_num, a.curr_res, a.curr_phase_num) == (b.curr_img_num, b.curr_res, b.curr_phase_num)
        assert a.batch_size * 2 == b.batch_size == a.global_batch
        a.end_iter(), b.end_iter()
        assert a.alpha == b.alpha and a.fade_in_phase == b.fade_in_phase
    assert a.nimg_transition_lst == b.nimg_transition_lst and a.curr_res == 16


def test_fmap_table_and_lockstep_state():
    from gan_lab_amd import progressive as P
    assert (P.FMAP_BASE, P.FMAP_MAX) == (8192, 512)
    want = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256, 128: 128, 256: 64, 512: 32, 1024: 16}
    for res, f in want.items():
        assert P._fmap(int(np.log2(res)) - 1) == f

    class A(P.StyleGAN):
        def forward(self, x):
            return x

    class B(P.StyleGAN):
        def forward(self, x):
            return x
    P.StyleGAN.reset_state()
    P.ProGAN.reset_state()
    a, b = A(64), B(64)
    a.increase_scale()
    assert b.curr_res == 8 and b.fade_in_phase and b.scale_inc_metadata_updated
    a.alpha = 0.25
    assert b.alpha == 0.25
    a.alpha = 1 - 1e-9          # snaps to 1 and leaves the fade-in phase (base.py:161-170)
    assert b.alpha == 1 and not b.fade_in_phase
    with pytest.raises(ValueError):
        a.alpha = 1.5
    assert a.cls_base.__dict__ == b.cls_base.__dict__
    assert P.ProGAN._state.curr_res == 4     # the two families do not share state
    P.StyleGAN.reset_state()


def test_learner_config_copy_guards():
    from gan_lab_amd._int import LearnerConfigCopy
    ns = argparse.Namespace(model='StyleGAN', res_samples=128, batch_size=8, lda=10.0)
    c = LearnerConfigCopy(ns, 'StyleGANLearner', ('model', 'res_samples'), ('batch_size',))
    c.lda = 5.0
    assert c.lda == 5.0 and ns.lda == 10.0
    with pytest.raises(AttributeError):
        c.res_samples = 256
    with pytest.raises(AttributeError):
        c.batch_size = 4
    with pytest.raises(ValueError):
        LearnerConfigCopy(ns, 'Nope', (), ())


def _header_functions():
    src = open(os.path.join(ROOT, 'include', 'ganlab_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(ganlab_[a-z0-9_]+)\s*\(', src)))


def test_c_abi_exports_every_declared_symbol():
    """The shared library loads on a CPU-only box and exports exactly the functions the header
    declares (no compute call is made here)."""
    from gan_lab_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    declared = _header_functions()
    assert len(declared) >= 30
    assert sorted(_lib.SIGNATURES) == declared
    handle = ctypes.CDLL(_lib.SO_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    L = _lib.lib()
    assert L.ganlab_abi_version() == 1
    # pure host-side queries are callable without a GPU
    g = _lib.ConvGeom(32, 16, 1024, 1024, 16, 3, 1, 0)
    ho, wo = ctypes.c_int(), ctypes.c_int()
    assert L.ganlab_conv_out_hw(ctypes.byref(g), ctypes.byref(ho), ctypes.byref(wo)) == 0
    assert (ho.value, wo.value) == (1024, 1024)
    assert L.ganlab_conv_pack_f32(None, None, 16, 32, 3, 0, 1.0, None) == 9 * 32 * 64
    assert L.ganlab_conv_wgrad_workspace(ctypes.byref(g)) > 0
    bad = _lib.ConvGeom(1, 1, 4, 4, 1, 5, 0, 0)
    assert L.ganlab_conv_out_hw(ctypes.byref(bad), None, None) == -1


def test_ops_fail_loudly_without_gpu_tensors():
    import torch
    from gan_lab_amd import ops
    with pytest.raises(TypeError):
        ops.conv2d(torch.zeros(1, 3, 4, 4), torch.zeros(4, 3, 3, 3), padding=1)
    with pytest.raises(TypeError):
        ops.pixelnorm(torch.zeros(2, 8))


@pytest.mark.parametrize('res', [32, 64])
def test_resnet_state_dict_layout_matches_reference(res):
    """Module tree / state_dict keys and shapes of the ResNet GAN nets against the reference's own
    (captured in tests/golden/resnet{32,64}.npz); construction only, no kernels."""
    import numpy as np
    import os
    from gan_lab_amd.resnetgan import architectures as A
    G = np.load(os.path.join(os.path.dirname(__file__), 'golden', f'resnet{res}.npz'))
    gen_cls, disc_cls = (A.Generator64PixResnet, A.Discriminator64PixResnet) if res == 64 else \
        (A.Generator32PixResnet, A.Discriminator32PixResnet)
    g = gen_cls(len_latent=int(G['len_latent']), fmap=int(G['fmap_g']))
    d = disc_cls(fmap=int(G['fmap_d']))
    for pre, m in (('g0.', g), ('d0.', d)):
        ref = [(k[3:], G[k].shape) for k in G.files if k.startswith(pre)]
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref


def test_reference_checkpoint_reads_without_the_reference():
    """A file written by the reference's own save_model (tests/golden/ref_progan_ckpt.tar, made by
    make_golden.py) unpickles with the two foreign classes mapped onto local stand-ins."""
    import os
    import sys
    import torch
    from gan_lab_amd import checkpoint as ckpt
    assert not any('reference' in p for p in sys.path)
    path = os.path.join(os.path.dirname(__file__), 'golden', 'ref_progan_ckpt.tar')
    ck = ckpt.load_checkpoint(path)
    assert ckpt.is_reference_format(ck)
    cfg = ckpt.config_dict(ck)
    assert cfg['model'] == 'ProGAN' and cfg['res_samples'] == 16 and cfg['len_latent'] == 16
    assert ck['curr_res'] == 8 and 0 < ck['alpha'] < 1
    assert isinstance(ck['lagged_params'], dict) and isinstance(ck['lagged_params'].keys(), list)
    g_names = list(ck['gen_model_state_dict'].keys())
    assert list(ck['lagged_params'].keys()) == g_names
    # the reference re-creates its optimisers right before every save (progan/learner.py:963, :992, :1018), so
    # a reference checkpoint always carries a fresh Adam: all parameters listed (fade-in), no moments yet
    m = ckpt.moments_from_torch_adam(ck['opt_gen_state_dict'], g_names)
    assert m['step'] == 0 and not m['exp_avg']
    assert isinstance(ck['nl'], torch.nn.LeakyReLU)
    with pytest.raises(ValueError):
        ckpt.moments_from_torch_adam(ck['opt_gen_state_dict'], g_names[:-2])
    # the translation itself, on a torch Adam that has stepped
    ps = {'a.weight': torch.nn.Parameter(torch.randn(3, 4)), 'b.bias': torch.nn.Parameter(torch.randn(5))}
    opt = torch.optim.Adam(ps.values(), lr=1e-3, betas=(0., .99))
    for _ in range(3):
        opt.zero_grad()
        (ps['a.weight'].sum() ** 2 + (ps['b.bias'] ** 2).sum()).backward()
        opt.step()
    m = ckpt.moments_from_torch_adam(opt.state_dict(), list(ps))
    assert m['step'] == 3
    for k, p in ps.items():
        assert torch.equal(m['exp_avg'][k], opt.state[p]['exp_avg']) and \
            torch.equal(m['exp_avg_sq'][k], opt.state[p]['exp_avg_sq'])
    ns = type('C', (), dict(cfg))()
    ckpt.check_architecture(cfg, ns)
    ns.len_latent = 512
    with pytest.raises(ValueError):
        ckpt.check_architecture(cfg, ns)


def test_phase_schedule_restore_continues_identically():
    from gan_lab_amd.schedule import PhaseSchedule
    bs = {4: 4, 8: 4, 16: 2, 32: 2}

    def run(s, n, log):
        for _ in range(n):
            ev = s.begin_iter()
            s.after_d_iter()
            s.end_iter()
            log.append((tuple(ev), s.curr_res, s.batch_size, s.fade_in_phase, round(float(s.alpha), 12), s.curr_img_num))

    full, log_full = PhaseSchedule(4, 32, bs, 22), []
    run(full, 60, log_full)
    for k in (3, 9, 14, 27, 41):
        a, la = PhaseSchedule(4, 32, bs, 22), []
        run(a, k, la)
        b = PhaseSchedule(4, 32, bs, 22).restore(a.curr_res, a.curr_img_num, a.curr_phase_num,
                                                 list(a.nimg_transition_lst), a.alpha, a.progressively_grow)
        lb = []
        run(b, 60 - k, lb)
        assert la + lb == log_full, k


def test_bf16_compute_mode_host_side():
    """Config #2 plumbing without a GPU: which geometries the bf16-compute kernels take (pure host query), the
    packed-weight size query, the config field, and that a layer's kernel choice is frozen when its Geom is built."""
    from gan_lab_amd import _lib, ops
    from gan_lab_amd.config import make_config
    L = _lib.lib()

    def ok(n, cin, h, w, cout, ks=3, pad=1, up=0, pool=0):
        return L.ganlab_conv_bf16_supported(ctypes.byref(_lib.ConvGeom(n, cin, h, w, cout, ks, pad, up, pool)))
    assert ok(8, 128, 128, 128, 128) == 1 and ok(8, 512, 32, 32, 512) == 1 and ok(8, 256, 64, 64, 128) == 1
    assert ok(8, 128, 16, 16, 128) == 1          # 16-wide maps: 16 x 16 pixel tiles (forward / input gradient) ...
    wsz = L.ganlab_conv_wgrad_bf16_workspace
    assert wsz(ctypes.byref(_lib.ConvGeom(8, 128, 16, 16, 128, 3, 1, 0, 0))) == 0   # ... but an fp32 weight gradient
    assert ok(8, 128, 8, 8, 128) == 0 and ok(8, 128, 24, 16, 128) == 0              # H % 16 for the 16-wide tiles
    assert ok(8, 16, 1024, 1024, 16) == 0        # thin layers
    assert ok(8, 96, 32, 32, 128) == 0           # Cin not a multiple of 64
    assert ok(8, 128, 32, 32, 128, ks=1, pad=0) == 0
    # the nearest upsample in front / the average pool behind fold into the forward and input-gradient kernels (not both)
    assert ok(8, 128, 32, 32, 128, up=1) == 1 and ok(8, 128, 32, 32, 128, pool=1) == 1
    assert ok(8, 128, 32, 32, 128, up=1, pool=1) == 0 and ok(8, 128, 4, 8, 128, up=1) == 0
    assert wsz(ctypes.byref(_lib.ConvGeom(8, 128, 32, 32, 128, 3, 1, 1, 0))) > 0       # weight gradient: half-resolution x in place
    assert wsz(ctypes.byref(_lib.ConvGeom(8, 128, 8, 8, 128, 3, 1, 1, 0))) == 0        # ... but not on 16-wide taps
    assert ok(8, 128, 36, 32, 128) == 0          # H % 8
    assert L.ganlab_conv_pack_bf16(None, None, 128, 256, 0, 1.0, None) == 9 * 128 * 256
    assert L.ganlab_conv_pack_bf16(None, None, 100, 256, 0, 1.0, None) == -1
    assert L.ganlab_conv_wgrad_bf16_workspace(ctypes.byref(_lib.ConvGeom(8, 128, 32, 32, 128, 3, 1, 0, 0))) > 0

    assert make_config('stylegan', dev='cuda').compute_dtype == 'f32'
    assert make_config('stylegan', dev='cuda', compute_dtype='bf16').compute_dtype == 'bf16'
    with pytest.raises(ValueError):
        ops.set_compute_dtype('fp8')
    assert ops.get_compute_dtype() == 'f32'
    with ops.compute_dtype('bf16'):
        g_bf = ops.Geom(8, 128, 32, 32, 128, 3, 1)
        g_up = ops.Geom(8, 256, 32, 32, 128, 3, 1, up=1)       # upsample materialised, then the bf16 conv at 64^2
        g_thin = ops.Geom(8, 16, 64, 64, 16, 3, 1)
        assert ops.pool_fusable(8, 128, 64, 64, 128, 3, 1)      # conv + pool as one bf16 kernel
        g_pool = ops.Geom(8, 128, 64, 64, 128, 3, 1, pool=1)
    assert g_bf.bf is not None and g_up.bf is not None and (g_up.bf.Hin, g_up.up, g_up.s2) == (64, 1, False)
    assert g_bf.bf_fused is None and g_up.bf_fused is not None and (g_up.bf_fused.Hin, g_up.bf_fused.up) == (32, 1)
    assert g_pool.bf_fused is not None and (g_pool.bf.Hin, g_pool.Ho, g_pool.s2) == (64, 32, False)
    assert g_thin.bf is None
    assert ops.get_compute_dtype() == 'f32' and ops.Geom(8, 128, 32, 32, 128, 3, 1).bf is None
    assert ops.pool_fusable(8, 128, 64, 64, 128, 3, 1)


def test_splitk_and_fusion_plans_host_side():
    """Pure host queries of the C ABI (no GPU): which layers get split-K and with how many splits, that no split is ever
    empty, and which geometries fold a LeakyReLU derivative into their gradient kernels."""
    from gan_lab_amd import _lib
    L = _lib.lib()

    def geom(n, cin, h, w, cout, ks=3, pad=1, up=0, pool=0):
        return ctypes.byref(_lib.ConvGeom(n, cin, h, w, cout, ks, pad, up, pool))

    def plan(*a, dgrad=0, **k):
        return L.ganlab_conv_splitk_plan(geom(*a, **k), dgrad)
    # the benchmark's low-resolution 512-channel layers at batch 32, forward and input gradient alike
    # (16 x 16 maps: the 64-channel tile covers 16 x 8 pixels, so batch 32 x 8 channel tiles is 512 workgroups unsplit)
    assert plan(32, 512, 4, 4, 512) == 4 and plan(32, 512, 8, 8, 512) == 2 and plan(32, 512, 16, 16, 512) <= 1
    assert plan(8, 512, 16, 16, 512) == 2
    assert plan(32, 512, 8, 8, 512, dgrad=1) == 2
    assert plan(32, 512, 32, 32, 512) <= 1 and plan(32, 16, 1024, 1024, 16) <= 1      # enough tiles: plain launch
    assert plan(32, 512, 8, 8, 512, up=1) == 0                                         # never with the folded upsample
    # linear layers (1x1 "images"): mapping network at batch 32 / 8, style affine; a short contraction is left alone
    assert plan(32, 512, 1, 1, 512, ks=1, pad=0) == 4 and plan(8, 512, 1, 1, 1024, ks=1, pad=0) == 4
    assert plan(8, 128, 1, 1, 8192, ks=1, pad=0) <= 1
    # no empty split for any channel count: (S - 1) * ceil(chunks / S) < chunks with the kernel's K-chunk
    for cin in list(range(8, 80, 7)) + [96, 200, 257, 513, 1000]:
        for (h, ks) in [(4, 3), (8, 3), (16, 3), (1, 1)]:
            for cout in (16, 40, 72, 512):
                s = plan(3, cin, h, h, cout, ks=ks, pad=ks // 2)
                if s >= 2:
                    mb = 1 if cout <= 16 else (2 if cout <= 32 else None)
                    ci_t = 32 if ks == 1 else (16 if (h >= 16 and mb is not None) else 8)
                    pad_to = 32 if ks == 1 else 16
                    cin_p = -(-cin // pad_to) * pad_to
                    for t in {ci_t, 8 if ks == 3 else 32}:            # vector-staged or scalar-staged variant
                        chunks = cin_p // t
                        assert (s - 1) * -(-chunks // s) < chunks, (cin, h, ks, cout, s, t)
    # LeakyReLU-derivative folding: fromRGB's streaming kernels from 64x64 up; the dgrad epilogue mask for plain 3x3
    # 'same' convs on rows of >= 16 4-aligned pixels
    assert L.ganlab_conv_act_bwd_fused_supported(geom(32, 3, 1024, 1024, 16, ks=1, pad=0)) == 1
    assert L.ganlab_conv_act_bwd_fused_supported(geom(32, 3, 32, 32, 16, ks=1, pad=0)) == 0
    assert L.ganlab_conv_act_bwd_fused_supported(geom(32, 16, 1024, 1024, 16)) == 0
    assert L.ganlab_conv_dgrad_mask_supported(geom(32, 32, 512, 512, 32)) == 1
    assert L.ganlab_conv_dgrad_mask_supported(geom(32, 512, 8, 8, 512)) == 0
    assert L.ganlab_conv_dgrad_mask_supported(geom(32, 32, 512, 512, 32, up=1)) == 0
    assert L.ganlab_conv_dgrad_mask_supported(geom(32, 32, 512, 512, 32, ks=1, pad=0)) == 0


def integration_snippets():
    """The ```python blocks of INTEGRATION.md §1 (load + struct + signatures) and §2 (the forward binding)."""
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    blocks = re.findall(r'```python\n(.*?)```', text, flags=re.S)
    load = next(b for b in blocks if 'class ConvGeom' in b)
    fwd = next(b for b in blocks if 'def conv2d_ex_forward' in b)
    return load, fwd


def test_integration_snippet_host_side():
    """The documented ctypes binding, executed as written (from the repo root, like a maintainer would): the library
    loads, the mirror struct has the header's size (9 ints - VERDICT r01 #10), the pack size query answers."""
    load, fwd = integration_snippets()
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec(compile(load, 'INTEGRATION.md#1', 'exec'), ns)
        exec(compile(fwd, 'INTEGRATION.md#2', 'exec'), ns)
    finally:
        os.chdir(cwd)
    hdr = open(os.path.join(ROOT, 'include', 'ganlab_hip.h')).read()
    body = re.search(r'typedef struct \{(.*?)\} ganlab_conv_geom;', hdr, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [f.strip() for part in re.findall(r'int ([^;]+);', body) for f in part.split(',')]
    assert [n for n, _ in ns['ConvGeom']._fields_] == fields
    assert ctypes.sizeof(ns['ConvGeom']) == ns['lib'].ganlab_conv_geom_size() == 4 * len(fields)
    # size query of the packing (no device work): [tap][Cin padded to 16][Cout padded to 64] floats
    n = ns['lib'].ganlab_conv_pack_f32(None, None, 16, 16, 3, 0, 1.0, None)
    assert n >= 9 * 16 * 16 and n % 4 == 0
    assert callable(ns['conv2d_ex_forward'])


def test_conditional_variants_row_is_closed_by_the_probe(monkeypatch):
    """tests/golden/probe_conditional.py ran the REAL reference with class_condition /
    use_auxiliary_classifier (ProGAN, StyleGAN, ResNet GAN; several loss / penalty settings) - every variant raises in
    the reference's own constructor or first training iteration, so there is nothing to be in parity with and the
    product learners refuse the options loudly."""
    import json
    probe = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conditional_probe.json')))
    assert len(probe['variants']) >= 9 and probe['any_variant_runs'] is False
    for v in probe['variants']:
        assert v['exception'] and v['where'], v                      # each failure is located in a reference file:line
        assert v['stage'] in ('constructor', 'train')
    models = {v['variant'].split(':')[0] for v in probe['variants']}
    assert models == {'ProGAN', 'StyleGAN', 'ResNet GAN'}
    monkeypatch.setenv('GANLAB_HOST_LOGIC_ONLY', '1')
    from gan_lab_amd.config import make_config
    from gan_lab_amd.progan.learner import ProGANLearner
    for kw in (dict(class_condition=True), dict(use_auxiliary_classifier=True)):
        cfg = make_config('progan', dev='cpu', pin_memory=False, res_samples=8, res_dataset=8, num_classes=3, **kw)
        with pytest.raises(NotImplementedError, match='conditional_probe'):
            ProGANLearner(cfg)


@pytest.mark.parametrize('mode,scale,tmode', [('bilinear_up', 2, 'bilinear'), ('bilinear_down', .5, 'bilinear'),
                                              ('nearest_down', .5, 'nearest')])
def test_resampler_tables_reproduce_interpolate(mode, scale, tmode):
    """The host-built interpolation matrices of the table-driven resampler kernel (ops.resample_matrix: ATen's
    source-index arithmetic restated) against F.interpolate itself - what the reference's nn.Upsample(mode='bilinear'),
    NearestPool2d and BilinearPool2d call (utils/custom_layers.py:59-75) - and the tap tables handed to the kernel
    (forward: <= 2 taps, adjoint: <= 6) against the matrices."""
    import torch
    import torch.nn.functional as F
    from gan_lab_amd import ops
    for align in ((False, True) if tmode == 'bilinear' else (False,)):
        for n in (4, 6, 8, 16, 64, 256):
            m = ops.resample_matrix(mode, align, n)
            x = torch.randn(2, 3, n, n, dtype=torch.float64)
            kw = {} if tmode == 'nearest' else {'align_corners': align}
            y = F.interpolate(x.float(), scale_factor=scale, mode=tmode, **kw).double()
            mm = torch.from_numpy(m)
            assert (y - mm @ x @ mm.T).abs().max().item() < 1e-6, (mode, align, n)
            for mat, tmax in ((m, 2), (m.T, 6)):
                idx, w, t = ops._taps(mat)
                assert t <= tmax
                dense = np.zeros_like(mat)
                for o in range(mat.shape[0]):
                    for a in range(t):
                        dense[o, idx[o, a]] += w[o, a]
                assert np.abs(dense - mat).max() < 1e-7


def test_post_accumulate_hook_fires_for_a_directly_written_gradient():
    """ops.direct_param_grads writes a parameter's gradient into its arena slot and returns None to the engine; the
    data-parallel bucket hooks (parallel.GradReducer) rely on AccumulateGrad still running its post-accumulate hooks for
    such a parameter.  That is undocumented torch behaviour: this pins it, so an upgrade cannot silently turn the overlap
    of the gradient exchange with the backward off."""
    class Direct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, p, x):
            ctx.p = p
            ctx.save_for_backward(x)
            return (p.detach() * x).sum()

        @staticmethod
        def backward(ctx, g):
            x, = ctx.saved_tensors
            ctx.p.grad.add_(g * x)          # the kernel's direct write
            return None, None

    p = torch.nn.Parameter(torch.arange(4.0))
    q = torch.nn.Parameter(torch.ones(4))
    p.grad, q.grad = torch.zeros(4), torch.zeros(4)
    fired = []
    p.register_post_accumulate_grad_hook(lambda t: fired.append('p'))
    q.register_post_accumulate_grad_hook(lambda t: fired.append('q'))
    x = torch.tensor([1.0, 2.0, 3.0, 4.0])
    (Direct.apply(p, x) + (q * x).sum()).backward()
    assert sorted(fired) == ['p', 'q'], fired
    assert torch.equal(p.grad, x) and torch.equal(q.grad, x)


def test_fused_adam_refuses_device_scalars_with_several_groups():
    """One (lr, step count) triple lives on the device for a replayed step: a second parameter group would
    silently train with the first one's."""
    from gan_lab_amd.optim import FusedAdam
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    a.grad, b.grad = torch.ones(4), torch.ones(4)
    opt = FusedAdam([{'params': [a]}, {'params': [b], 'lr': 1e-4}])
    opt.dev_scalars = 1234
    with pytest.raises(RuntimeError, match='exactly one parameter group'):
        opt.step()


def test_step_graphs_own_what_they_captured(monkeypatch):
    """captured step graphs hold raw pointers into the pack cache's buffers and descriptor tables.
    Host side of the fix: (i) the graphs keep strong references to every buffer / table alive at capture, (ii) a flush
    of the cache or a table rebuild changes ``ops.pack_generation()``, which is part of the graphs' signature, (iii) the
    learner's generation counter - not ``id()`` of arenas / optimisers - identifies what was captured, (iv) the batch's
    leading size is not part of the signature (a short last batch steps eagerly, the graphs stay)."""
    from gan_lab_amd import graphs, ops

    class _Net(object):
        training, curr_res, fade_in_phase = True, 8, False

    class _L(object):
        batch_size = 4
        gen_model = disc_model = _Net()
        _graph_gen = 3

    monkeypatch.setattr(ops, '_PACK_CACHE', {})
    monkeypatch.setattr(ops, '_PACK_TABLES', {})
    e = ops._PackEntry()
    e.w, e.out = torch.zeros(3), torch.ones(5)
    ops._PACK_CACHE['k'] = e
    tab = torch.zeros(7, dtype=torch.uint8)
    ops._PACK_TABLES[(0, 1)] = (('k',), tab, 1)
    sg = graphs._StepGraphs(_L())
    sg._own_pack_state()
    held = {id(t) for t in sg.keepalive}
    assert {id(e.out), id(e.w), id(tab)} <= held
    gen0 = ops.pack_generation()
    sig0 = sg._common_signature(torch.zeros(4, 3, 8, 8))
    assert sig0 == sg._common_signature(torch.zeros(3, 3, 8, 8))        # (iv)
    ops.bump_weight_epoch()                                              # full flush (cache overflow, growth, sampling graph)
    assert ops.pack_generation() == gen0 + 1 and not ops._PACK_CACHE
    assert sg._common_signature(torch.zeros(4, 3, 8, 8)) != sig0         # (ii)
    assert sg.keepalive and sg.keepalive[0] is not None                  # (i) still referenced after the flush
    sig1 = sg._common_signature(torch.zeros(4, 3, 8, 8))
    _L._graph_gen += 1                                                   # (iii) arenas / optimisers rebuilt
    assert sg._common_signature(torch.zeros(4, 3, 8, 8)) != sig1
    ops.bump_weight_epoch([(0, 16)])                                     # an optimiser step: nothing dropped
    assert ops.pack_generation() == gen0 + 1


def test_deferred_exposes_the_shape_of_its_tensor():
    """``Deferred.shape`` had slipped out of the class (an edit left it as dead code under a function)."""
    import torch
    from gan_lab_amd import ops
    a = torch.zeros(2, 3, 4, 5)
    d = ops.Deferred(a, None, None, None, None, None)
    assert d.shape == a.shape and d.read() is d


def test_custom_layers_define_tanh_once():
    import inspect
    from gan_lab_amd.utils import custom_layers
    src = inspect.getsource(custom_layers)
    assert src.count('class Tanh(') == 1


def test_mark_packs_stale_keeps_the_pack_generation():
    """With no rewritten range on record the whole cache goes stale through one catch-all range; nothing is dropped and the
    generation (part of a step graph's signature) does not move - and an empty cache has nothing to go stale."""
    from gan_lab_amd import ops
    saved = (dict(ops._PACK_CACHE), dict(ops._PACK_TABLES), dict(ops._PACK_RANGES))
    try:
        ops._PACK_CACHE.clear(); ops._PACK_TABLES.clear(); ops._PACK_RANGES.clear()
        gen = ops.pack_generation()
        ops.mark_packs_stale()
        assert ops.pack_generation() == gen and not ops._PACK_RANGES
        e = ops._PackEntry()
        e.w, e.out, e.serial, e.ptr, e.desc = None, None, ops._PACK_SERIAL[0], 4096, None
        ops._PACK_CACHE['k'] = e
        ops.mark_packs_stale()
        assert ops.pack_generation() == gen and 'k' in ops._PACK_CACHE
        assert ops._stale_range(e) == ops._ALL_ADDRESSES
        ops.mark_packs_stale()          # with a range on record: the same range again, newer serial
        assert ops.pack_generation() == gen and list(ops._PACK_RANGES) == [ops._ALL_ADDRESSES]
    finally:
        ops._PACK_CACHE.clear(); ops._PACK_TABLES.clear(); ops._PACK_RANGES.clear()
        ops._PACK_CACHE.update(saved[0]); ops._PACK_TABLES.update(saved[1]); ops._PACK_RANGES.update(saved[2])


# ---- the split-product kernels' support predicates agree with their launchers' limits -----------------------------------------
# Each launcher refuses (GANLAB_EINVAL) a geometry past one of its byte / index limits: 32-bit buffer ranges and offsets, the tile
# count.  The predicate (ops.x3_ok and kin) must refuse it first, so the layer falls back to the exact kernels instead of failing.
# Restated here in the kernels' GEMM roles (CI contracted, CO written; H, W: conv_x3 plane, Hl, Wl: the low resolution).
_I31, _U32 = 0x7fffffff, 0xffffffff


def _x3_launch_ok(n, ci, co, h, w):           # x3_launch (conv_x3.hip): 64 x 16 x 16 tiles, 9 stages of 24 KB per 64 channels
    return (n * (w // 16) * (h // 16) * (co // 64) <= _I31 and (co // 64) * (ci // 64 * 9) * 24576 <= _U32 and
            ci * h * w * 4 <= _I31 and n * ci * 4 <= _I31)


def _xu_launch_ok(n, ci, co, hl, wl):         # xu_launch (conv_x3_up.hip): co / 32 images of ci / 8 k-steps of 24 KB
    return (n * (wl // 16) * (hl // 8) * (co // 32) <= _I31 and (co // 32) * (ci // 8) * 24576 <= _U32 and
            ci * hl * wl * 4 <= _I31 and n * ci * 4 <= _I31)


def _xd_launch_ok(n, ci, co, hl, wl):         # xd_launch (conv_x3_down.hip): co / 128 tiles of ci / 2 k-steps of 24 KB
    return (n * (wl // 16) * (hl // 8) * (co // 128) <= _I31 and (co // 128) * (ci // 2) * 24576 <= _U32 and
            ci * hl * wl * 16 <= _I31)


def _x3_geoms(n, ci, co, h, w):
    return {'fwd': (0, (n, ci, h, w, co, 3, 1, 0, 0)), 'dgrad': (1, (n, co, h, w, ci, 3, 1, 0, 0))}


def _xu_geoms(n, ci, co, hl, wl):     # an up layer's forward; a pooled layer's input gradient
    return {'fwd': (0, (n, ci, hl, wl, co, 3, 1, 1, 0)), 'dgrad': (1, (n, co, 2 * hl, 2 * wl, ci, 3, 1, 0, 1))}


def _xd_geoms(n, ci, co, hl, wl):     # a pooled layer's forward; an up layer's input gradient
    return {'fwd': (0, (n, ci, 2 * hl, 2 * wl, co, 3, 1, 0, 1)), 'dgrad': (1, (n, co, hl, wl, ci, 3, 1, 1, 0))}


# kernel, limit, (N, CI, CO, H, W) just under the limit, the same just over it
_X3_LIMIT_CASES = [
    ('x3', 'plane bytes', (1, 64, 64, 2048, 4080), (1, 64, 64, 2048, 4096)),
    ('x3', 'affine table bytes', (2 ** 23 - 1, 64, 64, 16, 16), (2 ** 23, 64, 64, 16, 16)),
    ('x3', 'weight image bytes', (1, 64, 1242752, 16, 16), (1, 64, 1242816, 16, 16)),
    ('x3', 'tile count', (2 ** 22, 64, 32704, 16, 16), (2 ** 22, 64, 32768, 16, 16)),
    ('xu', 'plane bytes', (1, 64, 64, 2048, 4080), (1, 64, 64, 2048, 4096)),
    ('xu', 'affine table bytes', (2 ** 23 - 1, 64, 64, 8, 16), (2 ** 23, 64, 64, 8, 16)),
    ('xu', 'weight image bytes', (1, 64, 699040, 8, 16), (1, 64, 699072, 8, 16)),
    ('xu', 'tile count', (2 ** 22, 64, 32 * 511, 8, 16), (2 ** 22, 64, 32 * 512, 8, 16)),
    ('xd', 'plane bytes', (1, 16, 128, 2048, 4080), (1, 16, 128, 2048, 4096)),
    ('xd', 'weight image bytes', (1, 16, 2796160, 8, 16), (1, 16, 2796288, 8, 16)),
    ('xd', 'tile count', (2 ** 24, 16, 128 * 127, 8, 16), (2 ** 24, 16, 128 * 128, 8, 16)),
]


@pytest.mark.parametrize('case', _X3_LIMIT_CASES, ids=lambda c: f'{c[0]}-{c[1].replace(" ", "_")}')
def test_x3_support_predicates_refuse_what_the_launchers_refuse(case):
    """Only the predicates run (pure host code): no allocation, no launch."""
    from gan_lab_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    L = _lib.lib()
    kernel, limit, under, over = case
    pred = {'x3': L.ganlab_conv_x3_supported, 'xu': L.ganlab_conv_s2_x3_supported,
            'xd': L.ganlab_conv_s2_down_x3_supported}[kernel]
    launch_ok = {'x3': _x3_launch_ok, 'xu': _xu_launch_ok, 'xd': _xd_launch_ok}[kernel]
    geoms = {'x3': _x3_geoms, 'xu': _xu_geoms, 'xd': _xd_geoms}[kernel]
    assert launch_ok(*under) and not launch_ok(*over)
    for shape, want in ((under, 1), (over, 0)):
        for role, (dgrad, fields) in geoms(*shape).items():
            g = _lib.ConvGeom(*fields)
            assert pred(ctypes.byref(g), dgrad) == want, (kernel, limit, role, shape)


def test_conv_route_names_the_recorded_families():
    """``ops.conv_route`` on every row of the dispatch census (tests/conv_census.py), against the kernels the commit before it
    launched for that row (tests/golden/conv_census.json): only predicates run, so the routing order is pinned without a GPU.  The
    table must reach every family and every packed layout."""
    import conv_census as C
    from gan_lab_amd import _lib, ops
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    recorded = C.load()
    assert sorted(recorded) == sorted(r[0] for r in C.ROWS)
    assert ops.x3_enabled() and ops._X3_MIN_TILES == 128 and ops.get_compute_dtype() == 'f32'
    families, packs = set(), set()
    for row in C.ROWS:
        first, second = recorded[row[0]]
        g = C.geom_of(ops, row)
        assert C.admitted(ops, row, g), row[0]
        want = C.family_of(row, second)
        assert ops.conv_route(g, row[1]) == want, (row[0], want)
        families.add(want)
        packs |= C.pack_rows_of(first)
        if want in ops._PACK_ROWS and row[1] != 'wgrad':        # the family packs into the row of its name
            assert C.pack_rows_of(first) == {want}, (row[0], first)
    assert families == set(C.FAMILIES) == {ops.BF16, ops.X3, ops.X3_UP, ops.X3_DOWN, ops.S2, ops.LINEAR, ops.F32}
    assert packs == set(ops._PACK_ROWS)
