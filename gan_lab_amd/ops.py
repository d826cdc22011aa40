"""Autograd ops over the HIP C-ABI (include/ganlab_hip.h): convolution dispatch with its fused tails, and the facade of the op
families.

This file holds one subject, the tightly coupled conv core - the packed-weight cache, the split-product gates, the ``k_conv_*``
launchers, the mask-bits and fused-blur launchers, the mutually recursive conv Functions, handoffs, InstanceNorm, deferred tails
and modulated convs - and the module state that tests, bench.py and tools rebind (DESIGN.md 4.4a lists the names).  The leaf
families, each a launcher layer over one or two ``csrc/*.hip`` files, live in ``gan_lab_amd/_ops/`` and are imported below by
name, so ``ops.<name>`` is the one way in for callers:
  _ops/core.py       plumbing (``_p``, ``_st``, ``_c``, ...) and the three autograd switches
  _ops/geom.py       compute-dtype switch, ``Geom``, launch observer
  _ops/pointwise.py  blur, up / pool / resample, bias_act and act_bwd launchers, channel sums, axpby, tanh, mul, per-channel affine
  _ops/norm.py       BatchNorm (training), LayerNorm, their composed cross-checks
  _ops/loss.py       minibatch stddev, scalar reductions, BCE / hinge / channel-norm penalty
  _ops/attention.py  attention, 2x2 max pool, gated residual
  _ops/metrics.py    SWD, PRDC, Frechet moments / KID, path length, MS-SSIM, radial spectrum and its regulariser
  _ops/optim.py      spectral norm, orthogonal regularisation, Adam / RMSprop / SGD / optimistic Adam, EWMA
  _ops/augment.py    random draws, DiffAugment, ADA
  _ops/cond.py       labels, conditional BatchNorm
  _ops/hier.py       hierarchical latents, modulated BatchNorm, class projection
  _ops/cr.py         consistency regularisation
  _ops/cond_loss.py  class cross-entropy, contrastive losses
  _ops/project.py    latent-space projection
A function that reads a name which is rebound on this module stays in this file: a rebinding reaches only functions whose
globals are this module's.  A new family goes into a new ``_ops/`` module, not at the tail of this file.

Layering:
  k_*        thin launchers: torch tensors in (device memory + current stream), kernel call, tensor out.
  _Fn        torch.autograd.Function subclasses.  Every backward is itself written with other
             Functions of this module, so `torch.autograd.grad(..., create_graph=True)` (the R1 /
             WGAN-GP penalty, reference resnetgan/learner.py:811-815) differentiates straight
             through the hand-written kernels:
                conv is bilinear -> {fwd, dgrad, wgrad} is closed under differentiation;
                LeakyReLU'' = 0 -> act_bwd is linear in the cotangent, None towards the activation;
                blur is self-adjoint; pool2/up2 are an adjoint pair; mbstd has an explicit bwd-of-bwd.
  functional wrappers (conv2d, linear, bias_act, ...) used by custom_layers.py / the architectures.

All ops require contiguous fp32 CUDA(HIP) tensors and raise otherwise - there is no CPU path.
"""
import collections
import ctypes
import os

import numpy as np  # noqa: F401  (part of the module's surface: tests/golden/ops_surface.txt)

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, PACK_DGRAD, PACK_FWD, ConvGeom, check
from ._ops.core import (  # noqa: F401
    _p, _RAW_STREAM, _GET_DEVICE, _st, _c, _inplace, _same_numel, _gpu_device, _new, _ct, _aligned16, _nchw, _row_workspace,
    _INPUT_GRAD_ONLY, input_grad_only, _want_param_grads, _NO_GRAD_TOWARDS, no_grad_towards, _wants_input_grad, _DIRECT, _SINK,
    _TAKEN, _TAKE_HITS, direct_grads_enabled, direct_param_grads, _sink, _take, arena_takes, _sunk)
from ._ops.geom import (  # noqa: F401
    _COMPUTE, set_compute_dtype, get_compute_dtype, compute_dtype, Geom, pool_fusable, _OBSERVER, set_launch_observer, conv_flops,
    _note)
from ._ops.pointwise import (  # noqa: F401
    k_blur, decode_u8, k_up2, k_pool2, RESAMPLE_MODES, _RESAMPLE_TABLES, resample_matrix, _taps, _resample_tables, k_resample,
    k_bias_act, k_act_bwd, k_act_bwd_bias, k_channel_sum, k_axpby, k_scale_dev, k_sum, _ActBwd, _ActBwdBias, _ChanSum,
    _GroupBroadcast, _Blur, _Pool2, _Up2, _Resample, _Scale, _Axpby, _PixelNorm, _ChanAffine, _Mul, _Tanh, _TanhBwd, chan_affine,
    mul, tanh, channel_sum, blur, avg_pool2, upsample2, resample, lerp, scale, add, global_avg_pool, pixelnorm, group_broadcast)
from ._ops.norm import (  # noqa: F401
    _BatchNormTrain, batch_norm_composed, _ln_rowsums, _ln_project, _LayerNorm, _LayerNormBwd, layer_norm, layer_norm_composed)
from ._ops.loss import (  # noqa: F401
    _MbstdStat, _MbstdBwd, _Sum, _BceMean, _HingeMean, _HingeBwd, _ChNormPenalty, mbstd_stat, sum_all, sumsq_all, bce_logits_mean,
    hinge_mean, chnorm_penalty)
from ._ops.attention import (  # noqa: F401
    _ATTN_SECOND_ORDER, _attn_dims, attention_ok, k_attn_fwd, k_attn_bwd, _Attention, _AttentionBwd, _pool_dims, k_maxpool2x2,
    k_maxpool2x2_bwd, _MaxPool2x2, _MaxPool2x2Bwd, k_gated_residual, k_dot, _GatedResidual, _GatedResidualBwd, attention,
    max_pool2x2, gated_residual)
from ._ops.metrics import (  # noqa: F401
    SWD_DESC, _swd_planes, swd_down, swd_band, swd_gather, swd_stats, swd_project, _SWD_WS, _swd_workspace, swd_sort, swd_distance,
    swd_positions, swd_directions, PRDC_MAX_K, _prdc_rows, _prdc_vector, prdc_norms, prdc_knn, prdc_cross, MOMENTS_MAX_DIM,
    _accumulator, moments_accum, kid_rowsums, PPL_MAX_DIM, PPL_MODES, PPL_SAMPLINGS, PPL_RECORD, check_ppl_epsilon, ppl_endpoints,
    row_sqdist, trimmed_mean, MSSSIM_LEVELS, _msssim_images, msssim_workspace, msssim_level, msssim_finish,
    SPECTRUM_MIN_RES, SPECTRUM_MAX_RES, SPECTRUM_WINDOWS, _spectrum_size, spectrum_scratch_bytes, _spectrum_alloc,
    spectrum_workspace, spectrum_scratch, spectrum_feed, spectrum_finish, SPECTRUM_BANDS, _spectrum_batch, _spectrum_chunk,
    _spectrum_window, _spectrum_profiles, spectrum_profile_mean, spectrum_target_update, _SpectrumLossBwd, _SpectrumLoss,
    spectrum_loss)
from ._ops.optim import (  # noqa: F401
    SN_EPS, SnTable, sn_refresh, sn_backward, ortho_plan, OrthoTable, ortho_apply, lerp_rows, _adam_operands, adam_step,
    adam_step_dev, _optim_operands, rmsprop_step, rmsprop_step_dev, sgd_step, sgd_step_dev, oadam_step, oadam_step_dev,
    set_step_scalars, ewma_step, EwmaTable, ewma_many)
from ._ops.augment import (  # noqa: F401
    randn, check_truncation, trunc_randn, randn_dev, diffaug_params, diffaug_params_dev, k_diffaug, ADA_ROW, ADA_COUNTERS,
    ada_params, ada_params_dev, k_ada, ADA_EXT_ROW, ADA_EXT_COUNTERS, ADA_FILTER_TAPS, ADA_FILTER, ADA_NOISE, ADA_CUTOUT,
    ADA_NEW_GROUPS, AdaDraw, ada_filter_bank, ada_ext_params, ada_ext_params_dev, k_ada_ext, ada_update, _DiffAugment,
    _DiffAugmentAdjoint, _AdaAugment, _AdaAugmentAdjoint, diff_augment, ada_augment)
from ._ops.cond import _labels, randint, _bn_batch_stats, _CondBatchNorm, cond_batch_norm  # noqa: F401
from ._ops.hier import (  # noqa: F401
    _slot_open, HierTable, _HierModulate, hier_modulate, _ModBatchNorm, _mod_rows, _mod_stats, mod_batch_norm, mod_batch_norm_cols,
    _proj_dims, _ClassProj, _ClassProjDfeat, _ClassProjDweight, class_projection)
from ._ops.cr import (  # noqa: F401
    _cr_table, cr_params, cr_transform, _FirstOrderOnly, _first_order, _CrMsd, _cr_imsd_fwd, _CrImsd, _CrImsdHalves, cr_msd, cr_imsd)
from ._ops.cond_loss import (  # noqa: F401
    CL_MODES, CL_MAX_N, CL_MAX_E, CL_MAX_K, _cl_range, _ClassCrossEntropy, _ClassContrastive, class_cross_entropy, class_contrastive)
from ._ops.project import (  # noqa: F401
    PYRAMID_MAX_LEVELS, PROJECT_SCHEDULE, pyramid_max_levels, check_pyramid_weights, _PyramidMse, pyramid_mse, w_moments,
    check_project_schedule, project_step)


# ---- packed-weight cache ------------------------------------------------------------------------
# Packing (OIHW -> [tap][ci][co], eq-LR scale folded in) costs one tiny kernel; D weights are used by 3 forward + several
# dgrad passes per step, so the result is cached until the weights change.  The entry keeps an alias of the weight alive so
# its address cannot be recycled under the key.
# Who changes weights: (i) in-place torch ops - seen through ``w._version`` in the key; (ii) the fused optimiser, which
# rewrites a whole parameter arena through raw pointers - it reports the byte ranges it touched
# (``bump_weight_epoch(ranges)``), every cached entry inside such a range is stale, and the FIRST request for one of them
# re-packs ALL of them in ONE launch from a device-resident descriptor table (csrc/pack.hip: 60-190 pack launches per
# training step before).  Entries outside the range (the other network) stay valid.  ``bump_weight_epoch()`` without
# ranges drops everything (growth events, graph capture).
class _PackEntry(object):
    __slots__ = ('w', 'out', 'serial', 'ptr', 'row', 'desc')      # row: of _PACK_ROWS; desc: the PackDesc fields kind ... total


_PACK_CACHE = {}
_PACK_SERIAL = [0]
_PACK_GEN = [0]          # bumped when buffers a captured graph may point at are dropped: full flush, table rebuild
_PACK_RANGES = {}        # (lo, hi) byte range -> serial of its last rewrite
_PACK_TABLES = {}        # (lo, hi) -> (entry keys, device descriptor table, total blocks)
_KIND_PLAIN, _KIND_S2, _KIND_BF16, _KIND_X3 = (_lib.DEFINES['GANLAB_PACKKIND_' + n] for n in ('PLAIN', 'S2', 'BF16', 'X3'))
# The kernel families a conv can run on (``conv_route``): bf16 compute; split products plain, transposed (an up layer's forward, a
# pooled layer's input gradient) and strided (the other two); exact stride-2; the long-contraction linear run as a weight gradient;
# exact fp32.  A family that packs weights has the row of its name below.
BF16, X3, X3_UP, X3_DOWN, S2, LINEAR, F32 = 'bf16', 'x3', 'x3_up', 'x3_down', 's2', 'linear', 'f32'

# The packed layouts, one row each; a new kernel family's layout is a new row (and its branch in csrc/pack.hip).
#   fn, dtype   library entry point ``ganlab_<fn>(w, out, Cout, Cin, *args, scale, stream)`` (``out`` NULL: size query), buffer dtype
#   args        what the entry point takes between Cin and scale, in its order: the weight's ``ks``, the request's ``mode``
#               (PACK_FWD / PACK_DGRAD; ``transpose`` to the stride-2 f32 entry point) and ``up``
#   kind, ks    of ``_lib.PackDesc`` in the batched re-pack (ks None: the weight's own; 4 / 5: the stride-2 split-product layouts);
#               its ``mode`` / ``up`` are the request's where ``args`` names them, else 0
#   per_thread  packed elements per thread of pack_many_kernel, all taps of one weight position (None: ks * ks) - the kernel
#               returns past ``total / per_thread`` threads of a descriptor, so the block count here must agree with csrc/pack.hip
_PackRow = collections.namedtuple('_PackRow', 'fn dtype args kind ks per_thread')
_PACK_ROWS = {
    F32: _PackRow('conv_pack_f32', torch.float32, ('ks', 'mode'), _KIND_PLAIN, None, None),
    S2: _PackRow('conv_s2_pack_f32', torch.float32, ('up', 'mode'), _KIND_S2, 3, 16),
    BF16: _PackRow('conv_pack_bf16', torch.bfloat16, ('mode',), _KIND_BF16, 3, 9),
    X3: _PackRow('conv_x3_pack', torch.bfloat16, ('mode',), _KIND_X3, 3, 27),
    X3_UP: _PackRow('conv_s2_x3_pack', torch.bfloat16, ('up',), _KIND_X3, 4, 48),
    X3_DOWN: _PackRow('conv_s2_down_x3_pack', torch.bfloat16, ('up',), _KIND_X3, 5, 48),
}


def bump_weight_epoch(ranges=None):
    """Called by the fused optimiser after it rewrites parameters through raw pointers (``ranges``: [(lo, hi)] device
    address ranges), or without arguments to drop every packed weight."""
    _PACK_SERIAL[0] += 1
    if ranges is None:
        if _PACK_CACHE or _PACK_TABLES:      # (a flush that drops nothing leaves the generation - a step graph's signature - alone)
            _PACK_GEN[0] += 1
        _PACK_CACHE.clear()
        _PACK_TABLES.clear()
        _PACK_RANGES.clear()
        return
    for r in ranges:
        _PACK_RANGES[(int(r[0]), int(r[1]))] = _PACK_SERIAL[0]


def pack_generation():
    """Changes whenever the cache dropped buffers that an earlier reader may still hold raw pointers to (graphs.py)."""
    return _PACK_GEN[0]


_ALL_ADDRESSES = (0, 1 << 62)


def mark_packs_stale():
    """Every cached packed weight is re-packed at its next use, but the cache entries, their buffers and the descriptor
    tables of the batched re-pack stay (``bump_weight_epoch()`` without arguments drops them).  graphs.GraphedStep: a step
    graph must pack what it uses itself - with the ONE launch per parameter range of the steady state, whose table is
    already on the device - and a replay rewrites the parameters behind the host's back."""
    if _PACK_RANGES:
        bump_weight_epoch(list(_PACK_RANGES.keys()))
    elif _PACK_CACHE:
        # no range recorded yet (no optimiser step since the last flush): one catch-all range - nothing is dropped, so the
        # generation, which is part of a step graph's signature, stays: a capture or replay must not invalidate its own graphs
        bump_weight_epoch([_ALL_ADDRESSES])


def _pack_call(row, w, out, desc, stream):
    """The row's entry point on one weight: the size query (``w``, ``out`` and ``stream`` None) or the pack kernel."""
    _, cout, cin, ks, mode, up, scale, _ = desc
    args = {'ks': ks, 'mode': mode, 'up': up}
    return getattr(_lib.lib(), 'ganlab_' + row.fn)(_p(w), _p(out), cout, cin, *[args[a] for a in row.args], scale, stream)


def _pack_one(e):
    """Re-pack one cache entry with its own kernel (the batched launch's table cannot be uploaded while a capture runs)."""
    rc = _pack_call(e.row, e.w, e.out, e.desc, _st())
    if rc != e.desc[7]:
        raise _lib.GanlabLibraryError(f're-pack failed ({rc} != {e.desc[7]})')


def _stale_range(e):
    for r, ser in _PACK_RANGES.items():
        if ser > e.serial and r[0] <= e.ptr < r[1]:
            return r
    return None


def _repack_range(r):
    """Re-pack every cached entry whose weight lives in the rewritten range ``r`` with ONE launch."""
    L = _lib.lib()
    ser = _PACK_RANGES[r]
    items = [(k, e) for k, e in _PACK_CACHE.items() if r[0] <= e.ptr < r[1] and e.serial < ser]
    keys = tuple(k for k, _ in items)
    tab = _PACK_TABLES.get(r)
    if (tab is None or tab[0] != keys) and torch.cuda.is_current_stream_capturing():
        for _, e in items:          # no host-to-device copy inside a capture: one kernel per entry
            _pack_one(e)
            e.serial = _PACK_SERIAL[0]
        return
    if tab is None or tab[0] != keys:
        arr = (_lib.PackDesc * len(items))()
        blocks = 0
        for i, (_, e) in enumerate(items):
            kind, cout, cin, ks, mode, up, scale, total = e.desc
            d = arr[i]
            d.src, d.dst = e.w.data_ptr(), e.out.data_ptr()
            d.kind, d.Cout, d.Cin, d.ks, d.mode, d.up, d.scale, d.total, d.block0 = kind, cout, cin, ks, mode, up, scale, \
                total, blocks
            # one thread per weight position, all of its taps (csrc/pack.hip pack_many_kernel)
            blocks += (total // (e.row.per_thread or ks * ks) + 255) // 256
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        if tab is not None:
            _PACK_GEN[0] += 1       # the old table's memory goes back to the allocator
        tab = (keys, host.to(items[0][1].w.device), blocks)
        _PACK_TABLES[r] = tab
    check(L.ganlab_pack_many(tab[1].data_ptr(), len(items), tab[2], _st()), 'pack_many')
    now = _PACK_SERIAL[0]
    for _, e in items:
        e.serial = now


def _pack_lookup(key):
    e = _PACK_CACHE.get(key)
    if e is None:
        return None
    r = _stale_range(e)
    if r is not None:
        _repack_range(r)
    return e.out


def _pack_store(key, w, out, row, desc):
    if len(_PACK_CACHE) > 1024:
        bump_weight_epoch()
    e = _PackEntry()
    e.w, e.out, e.serial, e.ptr, e.row, e.desc = w.detach(), out, _PACK_SERIAL[0], w.data_ptr(), row, desc
    _PACK_CACHE[key] = e
    # a new entry changes the entry set of its range: the table is rebuilt at the next re-pack (keys differ)
    return out


def _packed_as(layout, w, mode, up, scale):
    """Weight ``w`` in the layout of row ``layout`` of ``_PACK_ROWS``, from the cache or packed now.  ``mode`` / ``up``: what the
    row's entry point takes of them, 0 for the one it does not take."""
    key = (w.data_ptr(), w._version, tuple(w.shape), mode, up, float(scale), layout)
    hit = _pack_lookup(key)
    if hit is not None:
        return hit
    row = _PACK_ROWS[layout]
    desc = (row.kind, w.shape[0], w.shape[1], row.ks or w.shape[2], mode, up, float(scale))
    n = _pack_call(row, None, None, desc + (0,), None)
    if n <= 0:
        raise _lib.GanlabLibraryError(f'{row.fn} size query failed ({n}) for weight {tuple(w.shape)}')
    out = torch.empty((n,), dtype=row.dtype, device=w.device)
    rc = _pack_call(row, w, out, desc + (0,), _st())
    if rc != n:
        raise _lib.GanlabLibraryError(f'{row.fn} failed ({rc})')
    return _pack_store(key, w, out, row, desc + (int(n),))


def _packed(w, mode, scale, s2_up=None):
    """mode: PACK_FWD / PACK_DGRAD.  s2_up: None -> plain [tap][ci][co] packing; 0 / 1 -> K4 packing of the
    stride-2 kernels for a down (pool) / up layer."""
    if s2_up is not None:
        return _packed_as(S2, w, 1 if mode == PACK_DGRAD else 0, int(s2_up), scale)
    return _packed_as(F32, w, mode, 0, scale)


def _packed_bf16(w, mode, scale):
    return _packed_as(BF16, w, mode, 0, scale)


# ---- fp32 convolutions as split products on the bf16 matrix cores (csrc/conv_x3.hip) --------------------------------
# Three bf16 planes per operand, six products per fp32 product, fp32 chains of one 32-channel chunk: as close to float64 as
# the exact-fp32 MFMA kernels (tools/x3_bench.py: 0.45-0.51 of ATen's rms error against 0.82-1.00) at 1.6-1.9x their speed.
# On by default for the thick plain 3x3 layers; GANLAB_X3=0 (or set_x3(False)) restores the exact-fp32 kernels everywhere.
_X3 = [os.environ.get('GANLAB_X3', '1') != '0']
_X3_MIN_TILES = 128       # (16 x 16 pixels x 64 channels) tiles below which the launch leaves most of the 256 CUs idle


def set_x3(enabled):
    """Switch the split-product kernels on / off (returns the previous setting)."""
    old = _X3[0]
    _X3[0] = bool(enabled)
    return old


def x3_enabled():
    return _X3[0]


# The three tile gates: pixel rows, pixel columns and output channels of one tile, the flag the layer must carry for its FORWARD to
# take the form (its input gradient: the other flag; None: a plain layer) and the library's predicate.  The resolution counted in
# tiles is the layer's low one.
_X3_GATES = {
    X3: (16, 16, 64, None, 'conv_x3_supported'),
    X3_UP: (8, 16, 32, 'up', 'conv_s2_x3_supported'),        # (32 output channels: both row parities in one workgroup)
    X3_DOWN: (8, 16, 128, 'pool', 'conv_s2_down_x3_supported'),
}


def _x3_gate(form, g, dgrad):
    """The Python conditions, then the minimum tile count, then the library's predicate (byte limits, divisibility)."""
    if not _X3[0]:
        return False
    rows, cols, chans, flag, supported = _X3_GATES[form]
    if flag is None:
        if g.bf is not None or g.s2 or g.up or g.pool or g.ks != 3 or g.pad != 1:
            return False
        hl, wl = g.Hin, g.Win
    else:
        if dgrad:
            flag = 'pool' if flag == 'up' else 'up'
        if not g.s2 or getattr(g, flag) != 1:
            return False
        hl, wl = (g.Hin // 2, g.Win // 2) if flag == 'pool' else (g.Hin, g.Win)
    co = g.Cin if dgrad else g.Cout
    if g.N * (hl // rows) * (wl // cols) * (co // chans) < _X3_MIN_TILES:
        return False
    return bool(getattr(_lib.lib(), 'ganlab_' + supported)(g.ref(), 1 if dgrad else 0))


def x3_ok(g, dgrad=False):
    """Does this conv (forward, or its input gradient) run on the split-product kernels?"""
    return _x3_gate(X3, g, dgrad)


def x3_s2_ok(g, dgrad=False):
    """Does this stride-2 fused layer run on the split-product kernel's transposed form?  (An up layer's forward, a pooled
    layer's input gradient.)"""
    return _x3_gate(X3_UP, g, dgrad)


def x3_s2_down_ok(g, dgrad=False):
    """The strided stride-2 form on the split-product kernel: a pooled layer's forward, an up layer's input gradient."""
    return _x3_gate(X3_DOWN, g, dgrad)


def x3_wgrad_ok(g):
    """Does this plain 3x3 layer's weight gradient run on the split-product kernel?"""
    if not _X3[0] or g.bf is not None or g.s2 or g.up or g.pool or g.ks != 3 or g.pad != 1 or g.Cin < 64 or g.Cout < 64:
        return False
    return bool(_lib.lib().ganlab_conv_wgrad_x3_supported(g.ref()))


def x3_s2_wgrad_ok(g):
    """Does this stride-2 layer's weight gradient run on the split-product box-sum kernel?"""
    if not _X3[0] or g.bf is not None or not g.s2 or g.ks != 3 or g.pad != 1:
        return False
    return bool(_lib.lib().ganlab_conv_s2_wgrad_x3_supported(g.ref()))


def _wgrad_x3(gy, x, s_, t_, gw, g, scale):
    """The split-product weight gradient of a plain layer or (``g.s2``) of a stride-2 one, the box-sum kernel."""
    L = _lib.lib()
    name = 'conv_s2_wgrad_x3' if g.s2 else 'conv_wgrad_x3'
    ws = torch.empty((getattr(L, f'ganlab_{name}_workspace')(g.ref()) + 3) // 4, dtype=torch.float32, device=x.device)
    check(getattr(L, 'ganlab_' + name)(_p(gy), _p(x), _p(s_), _p(t_), _p(gw), g.ref(), scale, _p(ws), ws.numel() * 4, _st()), name)
    return gw


def _packed_x3_s2_down(w, up, scale):
    """``up``: 0 = a pooled layer's forward weights, 1 = an up layer's input-gradient weights."""
    return _packed_as(X3_DOWN, w, 0, int(up), scale)


def _packed_x3_s2(w, up, scale):
    """``up``: 1 = an up layer's forward weights, 0 = a pooled layer's input-gradient weights."""
    return _packed_as(X3_UP, w, 0, int(up), scale)


def _packed_x3(w, mode, scale):
    return _packed_as(X3, w, mode, 0, scale)


_packed_x3_any, _wgrad_x3_s2 = _packed_as, _wgrad_x3      # the names these two had before they took every layout / both forms


# ---- which kernel family a conv runs on -------------------------------------------------------------------------------------------
def conv_route(g, op):
    """The kernel family the launcher of ``op`` ('fwd', 'dgrad', 'wgrad') uses for geometry ``g``.  The order of the questions
    below is the specification and this is its only statement (of a stride-2 layer: the strided split-product gate before the transposed
    one, both before the exact kernels); a new family is a line here, in front of the first family that would otherwise take its geometries.  The
    stride-2 split-product weight gradient is one kernel for both layer kinds and goes by the form of its layer's forward.
    Sub-choices that need a plan from the library (split-K, the rolling and 16-wide bf16 weight gradients) are made inside the
    family's launcher body."""
    if g.bf is not None:
        return BF16
    if op == 'wgrad':
        if g.s2:
            return (X3_UP if g.up else X3_DOWN) if x3_s2_wgrad_ok(g) else S2
        return X3 if x3_wgrad_ok(g) else F32
    dgrad = op == 'dgrad'
    assert dgrad or op == 'fwd', op
    if g.s2:
        if x3_s2_down_ok(g, dgrad):
            return X3_DOWN
        return X3_UP if x3_s2_ok(g, dgrad) else S2
    if not dgrad and g.ks == 1 and g.Hin == 1 and g.Win == 1 and g.N <= 64 and g.Cin >= 2048 and g.Cin % 128 == 0:
        return LINEAR
    return X3 if x3_ok(g, dgrad) else F32


def _route_among(g, op, admitted):
    """For a launcher whose form exists in some families only (masked, affine-on-load, one-pass layer tail): the routed family
    where it is one of ``admitted``, else exact fp32 - whose entry point refuses a geometry it does not take."""
    fam = conv_route(g, op)
    return fam if fam in admitted else F32


_AFF_FAMILIES = ((X3,), (X3_UP, S2))      # what the affine-on-load forms admit, by ``g.up``: they exist for plain and up layers


def _packed_for(fam, w, g, scale, dgrad=False):
    """``w`` as family ``fam``'s forward (``dgrad``: input-gradient) kernels read it."""
    if fam == X3_UP:            # these two entry points take the layer kind: an up layer's forward, a pooled layer's input gradient
        return _packed_as(fam, w, 0, 0 if dgrad else 1, scale)
    if fam == X3_DOWN:          # a pooled layer's forward, an up layer's input gradient
        return _packed_as(fam, w, 0, 1 if dgrad else 0, scale)
    return _packed_as(fam, w, PACK_DGRAD if dgrad else PACK_FWD, g.up if fam == S2 else 0, scale)


# family: its forward and its input-gradient entry point, for the families whose two launches are one call each with the
# signatures (x, wp, bias, y, geom, bias_scale, act, slope, stream) and (gy, wp, gx, geom, stream)
_CONV_ENTRY = {
    X3_DOWN: ('conv_s2_down_fwd_x3', 'conv_s2_down_dgrad_x3'),
    X3_UP: ('conv_s2_fwd_x3', 'conv_s2_dgrad_x3'),
    S2: ('conv_s2_fwd_f32', 'conv_s2_dgrad_f32'),       # conv + average pool (S kernel) or upsample + conv (T kernel)
    X3: ('conv_fwd_x3', 'conv_dgrad_x3'),
}


# ---------------------------------------------------------------------------------------------- #
# kernel launchers
# ---------------------------------------------------------------------------------------------- #
def k_conv_fwd(x, w, bias, g, scale, bias_scale=1.0, act=ACT_NONE, slope=0.2):
    x, w = _c(x, 'conv input'), _c(w, 'conv weight')
    assert tuple(x.shape) == g.in_shape, (tuple(x.shape), g.in_shape)
    assert tuple(w.shape) == (g.Cout, g.Cin, g.ks, g.ks), (tuple(w.shape), g.Cout, g.Cin, g.ks)
    _note('fwd', g)
    if bias is not None:
        bias = _c(bias, 'bias')
        assert bias.numel() == g.Cout
    y = _new(g.out_shape, x)
    fam = conv_route(g, 'fwd')
    L = _lib.lib()
    if fam == BF16:   # bf16-compute layer; a nearest upsample in front / average pool behind folds into the kernel
        geom = g.bf_fused if g.bf_fused is not None else g.bf
        xin = k_up2(x, 1.0) if (g.up and g.bf_fused is None) else x
        wp = _packed_for(BF16, w, g, scale)
        split = L.ganlab_conv_bf16_splitk_plan(ctypes.byref(geom), 0)
        if split >= 2:     # few output tiles, long contraction (512-channel 16x16 layers at small batch)
            m = 2 if geom.up else 1
            ws = torch.empty((split * geom.N * geom.Cout * geom.Hin * m * geom.Win * m,), dtype=torch.float32, device=x.device)
            check(L.ganlab_conv_fwd_bf16_splitk(_p(xin), _p(wp), _p(bias), _p(y), ctypes.byref(geom), bias_scale, act,
                                                slope, _p(ws), ws.numel() * 4, _st()), 'conv_fwd_bf16_splitk')
            return y
        check(L.ganlab_conv_fwd_bf16(_p(xin), _p(wp), _p(bias), _p(y), ctypes.byref(geom), bias_scale,
                                     act, slope, _st()), 'conv_fwd_bf16')
        return y
    if fam == LINEAR:
        # A linear layer with a long contraction and few rows (the critic's 4x4 "valid" conv: 8192 -> 512 on `batch`
        # rows): the forward kernel would walk all of K in 32 workgroups.  y[n][co] = sum_k x[n][k] w[co][k] is the
        # weight-gradient contraction with k as the pixel axis, x as a (1, N, k) "output gradient" and w as a
        # (1, Cout, k) "input" - no copies - and that kernel splits the pixel axis over ~1024 workgroups.
        g2 = Geom(1, g.Cout, g.Cin // 128, 128, g.N, 1, 0)
        obs = set_launch_observer(None)          # already reported as this forward
        try:
            y = k_conv_wgrad(x.view(g2.out_shape), w.view(g2.in_shape), g2, scale).view(g.out_shape)
        finally:
            set_launch_observer(obs)
        if bias is not None or act != ACT_NONE:
            y = k_bias_act(y, bias, None, None, bias_scale, act, slope)
        return y
    wp = _packed_for(fam, w, g, scale)
    if fam != F32:
        name = _CONV_ENTRY[fam][0]
        check(getattr(L, 'ganlab_' + name)(_p(x), _p(wp), _p(bias), _p(y), g.ref(), bias_scale, act, slope, _st()), name)
        return y
    split = 0 if g.up else L.ganlab_conv_splitk_plan(g.ref(), 0)
    if split >= 2:     # few output tiles, long contraction (512-channel 4x4 / 8x8 maps, small-batch linears)
        ws = torch.empty((split,) + tuple(y.shape), dtype=torch.float32, device=x.device)
        check(L.ganlab_conv_fwd_splitk_f32(_p(x), _p(wp), _p(bias), _p(y), g.ref(), bias_scale, act, slope, _p(ws),
                                           ws.numel() * 4, _st()), 'conv_fwd_splitk')
        return y
    check(L.ganlab_conv_fwd_f32(_p(x), _p(wp), _p(bias), _p(y), g.ref(), bias_scale, act, slope, _st()), 'conv_fwd')
    return y


def k_conv_dgrad(gy, w, g, scale):
    gy, w = _c(gy, 'conv grad_out'), _c(w, 'conv weight')
    assert tuple(gy.shape) == g.out_shape, (tuple(gy.shape), g.out_shape)
    _note('dgrad', g)
    fam = conv_route(g, 'dgrad')
    L = _lib.lib()
    wp = _packed_for(fam, w, g, scale, dgrad=True)
    if fam == BF16:
        def run(geom, out):
            split = L.ganlab_conv_bf16_splitk_plan(ctypes.byref(geom), 1)
            if split >= 2:
                m = 2 if geom.up else 1
                ws = torch.empty((split * geom.N * geom.Cin * geom.Hin * m * geom.Win * m,), dtype=torch.float32,
                                 device=gy.device)
                check(L.ganlab_conv_dgrad_bf16_splitk(_p(gy), _p(wp), _p(out), ctypes.byref(geom), _p(ws),
                                                      ws.numel() * 4, _st()), 'conv_dgrad_bf16_splitk')
            else:
                check(L.ganlab_conv_dgrad_bf16(_p(gy), _p(wp), _p(out), ctypes.byref(geom), _st()), 'conv_dgrad_bf16')
            return out
        if g.bf_fused is not None:     # the adjoint of the upsample (2 x 2 sum) / of the pool (upsample / 4) is in the kernel
            return run(g.bf_fused, _new(g.in_shape, gy))
        gxv = run(g.bf, _new((g.N, g.Cin, g.bf.Hin, g.bf.Win), gy))
        return k_pool2(gxv, 1.0) if g.up else gxv
    if fam != F32:
        gx = _new(g.in_shape, gy)
        name = _CONV_ENTRY[fam][1]
        check(getattr(L, 'ganlab_' + name)(_p(gy), _p(wp), _p(gx), g.ref(), _st()), name)
        return gx
    hv, wv = (2 * g.Hin, 2 * g.Win) if g.up else (g.Hin, g.Win)
    gxv = _new((g.N, g.Cin, hv, wv), gy)
    split = 0 if g.up else L.ganlab_conv_splitk_plan(g.ref(), 1)
    if split >= 2:
        ws = torch.empty((split,) + tuple(gxv.shape), dtype=torch.float32, device=gy.device)
        check(L.ganlab_conv_dgrad_splitk_f32(_p(gy), _p(wp), _p(gxv), g.ref(), _p(ws), ws.numel() * 4, _st()),
              'conv_dgrad_splitk')
        return gxv
    check(L.ganlab_conv_dgrad_f32(_p(gy), _p(wp), _p(gxv), g.ref(), _st()), 'conv_dgrad')
    if g.up:
        return k_pool2(gxv, 1.0)   # adjoint of the nearest upsample
    return gxv


def conv_dgrad_mask_ok(g):
    """The conv's input gradient can come out multiplied by lrelu'(x) (x: its input, a LeakyReLU output)."""
    return g.bf is None and not g.s2 and not g.up and bool(_lib.lib().ganlab_conv_dgrad_mask_supported(g.ref()))


def k_conv_dgrad_mask(gy, w, x, g, scale, slope):
    gy, w, x = _c(gy, 'conv grad_out'), _c(w, 'conv weight'), _c(x, 'conv input')
    assert tuple(gy.shape) == g.out_shape and tuple(x.shape) == g.in_shape
    _note('dgrad', g)
    gx = torch.empty_like(x)
    fam = _route_among(g, 'dgrad', (X3,))
    name = 'conv_dgrad_mask_x3' if fam == X3 else 'conv_dgrad_mask_f32'
    check(getattr(_lib.lib(), 'ganlab_' + name)(_p(gy), _p(_packed_for(fam, w, g, scale, dgrad=True)), _p(x), _p(gx), g.ref(),
                                                slope, _st()), name)
    return gx


def conv_act_bwd_fusable(g):
    """The conv's LeakyReLU backward folds into its own gradient kernels (fromRGB at >= 64x64, fp32)."""
    return g.bf is None and not g.s2 and bool(_lib.lib().ganlab_conv_act_bwd_fused_supported(g.ref()))


def k_conv_dgrad_act(gy, y, w, g, scale, slope):
    """``y``: the conv's activated output, or its sign bits (``k_conv_fwd_bits``)."""
    gy, w = _c(gy, 'conv grad_out'), _c(w, 'conv weight')
    assert tuple(gy.shape) == g.out_shape
    _note('dgrad', g)
    gx = _new(g.in_shape, gy)
    if _is_bits(y):
        check(_lib.lib().ganlab_conv_dgrad_act_bits_f32(_p(gy), y.data_ptr(), _p(_packed(w, PACK_DGRAD, scale)), _p(gx),
                                                        g.ref(), slope, _st()), 'conv_dgrad_act_bits')
        return gx
    y = _c(y, 'conv output')
    assert tuple(y.shape) == g.out_shape
    check(_lib.lib().ganlab_conv_dgrad_act_f32(_p(gy), _p(y), _p(_packed(w, PACK_DGRAD, scale)), _p(gx), g.ref(), slope,
                                               _st()), 'conv_dgrad_act')
    return gx


def k_conv_fwd_mask(x, w, y, g, scale, slope):
    x, w = _c(x, 'conv input'), _c(w, 'conv weight')
    assert tuple(x.shape) == g.in_shape
    _note('fwd', g)
    out = _new(g.out_shape, x)
    if _is_bits(y):
        check(_lib.lib().ganlab_conv_fwd_mask_bits_f32(_p(x), _p(_packed(w, PACK_FWD, scale)), y.data_ptr(), _p(out), g.ref(),
                                                       slope, _st()), 'conv_fwd_mask_bits')
        return out
    y = _c(y, 'conv output')
    assert tuple(y.shape) == g.out_shape
    check(_lib.lib().ganlab_conv_fwd_mask_f32(_p(x), _p(_packed(w, PACK_FWD, scale)), _p(y), _p(out), g.ref(), slope,
                                              _st()), 'conv_fwd_mask')
    return out


def k_conv_wgrad_act(gy, y, x, g, scale, slope, bias_scale, want_gb):
    gy, x = _c(gy, 'conv grad_out'), _c(x, 'conv input')
    assert tuple(gy.shape) == g.out_shape and tuple(x.shape) == g.in_shape
    _note('wgrad', g)
    L = _lib.lib()
    gw = _take('gw', (g.Cout, g.Cin, g.ks, g.ks), x)
    gb = _take('gb', (g.Cout,), x) if want_gb else None
    ws = torch.empty((max(L.ganlab_conv_wgrad_workspace(g.ref()), 4) + 3) // 4, dtype=torch.float32, device=x.device)
    if _is_bits(y):
        check(L.ganlab_conv_wgrad_act_bits_f32(_p(gy), y.data_ptr(), _p(x), _p(gw), _p(gb), g.ref(), scale, bias_scale, slope,
                                               _p(ws), ws.numel() * 4, _st()), 'conv_wgrad_act_bits')
        return gw, gb
    y = _c(y, 'conv output')
    assert tuple(y.shape) == g.out_shape
    check(L.ganlab_conv_wgrad_act_f32(_p(gy), _p(y), _p(x), _p(gw), _p(gb), g.ref(), scale, bias_scale, slope, _p(ws),
                                      ws.numel() * 4, _st()), 'conv_wgrad_act')
    return gw, gb


def k_conv_fwd_bits(x, w, bias, g, scale, bias_scale, act, slope):
    """fromRGB forward that also writes the sign bits of its activated output (the mask of its own backward)."""
    x, w = _c(x, 'conv input'), _c(w, 'conv weight')
    assert tuple(x.shape) == g.in_shape
    _note('fwd', g)
    y = _new(g.out_shape, x)
    bits = torch.empty((y.numel() // 32,), dtype=torch.int32, device=x.device)
    check(_lib.lib().ganlab_conv_fwd_bits_f32(_p(x), _p(_packed(w, PACK_FWD, scale)), _p(_c(bias, 'bias')) if bias is not None
                                              else None, _p(y), bits.data_ptr(), g.ref(), bias_scale, act, slope, _st()),
          'conv_fwd_bits')
    return y, bits


def k_conv_fwd_blur_bits(x, w, bias, g, scale, bias_scale, slope):
    """blur(lrelu(conv3x3(x, w) * scale + bias)) and the sign bits of the un-blurred activation in ONE rolling-window kernel
    (csrc/conv_roll_blur.hip) - or None where the geometry is not the thin one it takes."""
    if g.ks != 3 or g.up or g.pool or g.bf is not None or get_compute_dtype() != 'f32' or not mask_bits_ok_plane():
        return None
    if os.environ.get('GANLAB_ROLL_BLUR') == '0':      # A/B switch: conv kernel + blur pass
        return None
    x, w = _c(x, 'conv input'), _c(w, 'conv weight')
    L = _lib.lib()
    y = _new(g.out_shape, x)
    if not L.ganlab_conv_fwd_blur_supported(g.ref(), _p(x), _p(y)):
        return None
    assert tuple(x.shape) == g.in_shape
    _note('fwd', g)
    bits = torch.empty((y.numel() // 32,), dtype=torch.int32, device=x.device)
    check(L.ganlab_conv_fwd_blur_bits_f32(_p(x), _p(_packed(w, PACK_FWD, scale)), _p(_c(bias, 'bias')) if bias is not None
                                          else None, _p(y), bits.data_ptr(), g.ref(), bias_scale, slope, _st()),
          'conv_fwd_blur_bits')
    return y, bits


def conv_s2_blur_ok(g):
    """Does the thin transposed stride-2 kernel with the blur folded in (csrc/conv_s2_roll_blur.hip) take geometry ``g`` - an
    up layer for the generator's forward tail, a pooled layer for the critic's backward?"""
    if get_compute_dtype() != 'f32' or g.bf is not None or not g.s2 or os.environ.get('GANLAB_S2_ROLL_BLUR') == '0':
        return False
    key = ('s2blur', g.N, g.Cin, g.Hin, g.Win, g.Cout, g.up, g.pool)
    hit = _AFF_OK.get(key)
    if hit is None:
        hit = bool(_lib.lib().ganlab_conv_s2_blur_supported(g.ref()))
        _AFF_OK[key] = hit
    return hit


def k_conv_s2_fwd_blur_tail(a, s_, t_, w, bias, noise, noise_w, g, scale, bias_scale, act, slope, eps):
    """(y, mean, rstd): y = act(blur(conv(up2(a * s + t), w) * scale) + noise_w * noise + bias * bias_scale) and the
    InstanceNorm statistics of y, one kernel + the statistics' finish (``s_`` / ``t_`` None: plain input)."""
    a, w = _c(a, 'conv input'), _c(w, 'conv weight')
    assert g.up and tuple(a.shape) == g.in_shape
    _note('fwd', g)
    L = _lib.lib()
    y = _new(g.out_shape, a)
    mean, rstd = _new((g.N, g.Cout), a), _new((g.N, g.Cout), a)
    ws = torch.empty((L.ganlab_conv_s2_blur_workspace(g.ref()) + 7) // 8, dtype=torch.float64, device=a.device)
    wp = _packed(w, PACK_FWD, scale, s2_up=1)
    noise = _c(noise) if noise is not None else None
    if noise is not None:
        assert noise.numel() == g.N * g.Ho * g.Wo, (tuple(noise.shape), g.out_shape)
    check(L.ganlab_conv_s2_fwd_blur_tail_f32(_p(a), _p(wp), _p(s_), _p(t_), _p(bias), _p(noise), _p(noise_w), _p(y), _p(mean),
                                             _p(rstd), g.ref(), bias_scale, act, slope, eps, ctypes.c_void_p(ws.data_ptr()),
                                             ws.numel() * 8, _st()), 'conv_s2_fwd_blur_tail')
    return y, mean, rstd


def k_conv_s2_dgrad_blur_act(gy, w, bits, g, scale, slope, bias_scale, want_gb):
    """(gz, gb) = (lrelu'(bits) * blur(dgrad(gy, w) * scale), bias_scale * sum gz): the pooled conv g's input gradient fused
    with the backward of the LeakyReLU -> blur in front of it."""
    gy, w = _c(gy, 'conv grad_out'), _c(w, 'conv weight')
    assert g.pool and tuple(gy.shape) == g.out_shape and bits.numel() * 32 == g.N * g.Cin * g.Hin * g.Win
    _note('dgrad', g)
    L = _lib.lib()
    gz = _new(g.in_shape, gy)
    gb = _new((g.Cin,), gy) if want_gb else None
    ws = torch.empty((L.ganlab_conv_s2_blur_workspace(g.ref()) + 7) // 8, dtype=torch.float64, device=gy.device) \
        if want_gb else None
    wp = _packed(w, PACK_DGRAD, scale, s2_up=0)
    check(L.ganlab_conv_s2_dgrad_blur_act_bits_f32(_p(gy), _p(wp), bits.data_ptr(), _p(gz), _p(gb), g.ref(), slope, bias_scale,
                                                   ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                                   ws.numel() * 8 if ws is not None else 0, _st()),
          'conv_s2_dgrad_blur_act_bits')
    return gz, gb


def k_conv_wgrad(gy, x, g, scale):
    gy, x = _c(gy, 'conv grad_out'), _c(x, 'conv input')
    assert tuple(gy.shape) == g.out_shape and tuple(x.shape) == g.in_shape
    _note('wgrad', g)
    L = _lib.lib()
    gw = _take('gw', (g.Cout, g.Cin, g.ks, g.ks), x)
    fam = conv_route(g, 'wgrad')
    if fam in (X3, X3_UP, X3_DOWN):
        return _wgrad_x3(gy, x, None, None, gw, g, scale)
    if fam == BF16:
        if g.bf_fused is not None:
            # the rolling-row kernel reads the half-resolution operand (x of conv(up2 x), gy of pool2(conv x)) in place
            nbytes = L.ganlab_conv_wgrad_bf16_workspace(ctypes.byref(g.bf_fused))
            if nbytes > 0:
                ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
                check(L.ganlab_conv_wgrad_bf16(_p(gy), _p(x), _p(gw), ctypes.byref(g.bf_fused), scale, _p(ws),
                                               ws.numel() * 4, _st()), 'conv_wgrad_bf16')
                return gw
        # otherwise (16-wide taps) the weight gradient takes the materialised upsample of x (up) or of the pooled layer's
        # output gradient (pool: up2(gy) / 4, the adjoint of the average)
        xin = k_up2(x, 1.0) if g.up else x
        if g.pool:
            gy = k_up2(gy, 0.25)
        nbytes = L.ganlab_conv_wgrad_bf16_workspace(ctypes.byref(g.bf))
        if nbytes == 0:
            # 16-pixel-wide maps: bf16 forward / input gradient, but the bf16 weight-gradient kernels walk 32-pixel
            # strips - the (exact) fp32 kernel takes the materialised input
            nbytes = L.ganlab_conv_wgrad_workspace(ctypes.byref(g.bf))
            ws = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
            check(L.ganlab_conv_wgrad_f32(_p(gy), _p(xin), _p(gw), ctypes.byref(g.bf), scale, _p(ws), ws.numel() * 4,
                                          _st()), 'conv_wgrad')
            return gw
        ws = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
        check(L.ganlab_conv_wgrad_bf16(_p(gy), _p(xin), _p(gw), ctypes.byref(g.bf), scale, _p(ws), ws.numel() * 4,
                                       _st()), 'conv_wgrad_bf16')
        return gw
    name = 'conv_s2_wgrad' if fam == S2 else 'conv_wgrad'
    nbytes = getattr(L, f'ganlab_{name}_workspace')(g.ref())
    ws = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
    check(getattr(L, f'ganlab_{name}_f32')(_p(gy), _p(x), _p(gw), g.ref(), scale, _p(ws), ws.numel() * 4, _st()), name)
    return gw


_MASK_BITS = [None]


def mask_bits_ok(x):
    """The LeakyReLU backward of this (N,C,H,W) activation can run from its sign BITS (rows of whole 32-bit words):
    GANLAB_MASK_BITS=0 keeps the float tensor (A/B knob)."""
    if _MASK_BITS[0] is None:
        _MASK_BITS[0] = os.environ.get('GANLAB_MASK_BITS') != '0'
    return _MASK_BITS[0] and x.dim() == 4 and bool(_lib.lib().ganlab_mask_bits_supported(int(x.shape[2]), int(x.shape[3])))


def mask_bits_ok_plane():
    """The A/B knob alone (GANLAB_MASK_BITS): callers check the plane size themselves."""
    if _MASK_BITS[0] is None:
        _MASK_BITS[0] = os.environ.get('GANLAB_MASK_BITS') != '0'
    return _MASK_BITS[0]


def k_blur_bits(x):
    """(blur(x), sign bits of x): the bits are all the LeakyReLU backward of x's producer needs (int32 words, bit e of the
    NCHW-linear element index e set iff x[e] > 0)."""
    x = _aligned16(_c(x))         # (these kernels only have float4 forms: a view that starts off a 16-byte boundary is copied)
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    bits = torch.empty((x.numel() // 32,), dtype=torch.int32, device=x.device)
    check(_lib.lib().ganlab_blur3x3_bits_f32(_p(x), _p(y), bits.data_ptr(), n * c, h, w, _st()), 'blur3x3_bits')
    return y, bits


def _is_bits(y):
    return y.dtype == torch.int32


def blur_fusable(x):
    """Whether the fused blur kernels take this (N,C,H,W) map (H even, W a multiple of 4)."""
    return x.dim() == 4 and bool(_lib.lib().ganlab_blur_fused_supported(int(x.shape[2]), int(x.shape[3])))


def _blur_ws(x):
    n, c, h, w = x.shape
    nbytes = _lib.lib().ganlab_blur_fused_workspace(n, c, h, w)
    return torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)


def k_blur_bias_act(x, bias, noise, noise_w, bias_scale, act, slope):
    x = _aligned16(_c(x))
    n, c, h, w = x.shape
    bias = _c(bias) if bias is not None else None
    if noise is not None:
        noise, noise_w = _aligned16(_c(noise)), _c(noise_w)
        assert noise.numel() == n * h * w and noise_w.numel() == c
    y = torch.empty_like(x)
    check(_lib.lib().ganlab_blur_bias_act_f32(_p(x), _p(bias), _p(noise), _p(noise_w), _p(y), n, c, h, w, bias_scale,
                                              act, slope, _st()), 'blur_bias_act')
    return y


def _stats_out(x, n, c, hw):
    L = _lib.lib()
    ws = torch.empty((max(L.ganlab_act_stats_workspace(n, c, hw), 8) + 7) // 8, dtype=torch.float64, device=x.device)
    return _new((n * c,), x), _new((n * c,), x), ws


def k_blur_bias_act_stats(x, bias, noise, noise_w, bias_scale, act, slope, eps):
    """k_blur_bias_act that also returns the InstanceNorm statistics (mean, rstd) of its output."""
    x = _aligned16(_c(x))
    n, c, h, w = x.shape
    bias = _c(bias) if bias is not None else None
    if noise is not None:
        noise, noise_w = _aligned16(_c(noise)), _c(noise_w)
        assert noise.numel() == n * h * w and noise_w.numel() == c
    y = torch.empty_like(x)
    mean, rstd, ws = _stats_out(x, n, c, h * w)
    check(_lib.lib().ganlab_blur_bias_act_stats_f32(_p(x), _p(bias), _p(noise), _p(noise_w), _p(y), _p(mean), _p(rstd),
                                                    n, c, h, w, bias_scale, act, slope, eps, _p(ws), ws.numel() * 8,
                                                    _st()), 'blur_bias_act_stats')
    return y, mean, rstd


def k_bias_act_stats(x, bias, noise, noise_w, bias_scale, act, slope, eps):
    x = _aligned16(_c(x))
    n, c, hw = _nchw(x)
    y = torch.empty_like(x)
    bias = _c(bias) if bias is not None else None
    noise = _aligned16(_c(noise)) if noise is not None else None
    noise_w = _c(noise_w) if noise_w is not None else None
    if noise is not None:
        assert noise.numel() == n * hw and noise_w.numel() == c
    mean, rstd, ws = _stats_out(x, n, c, hw)
    check(_lib.lib().ganlab_bias_act_stats_f32(_p(x), _p(bias), _p(noise), _p(noise_w), _p(y), _p(mean), _p(rstd), n, c,
                                               hw, bias_scale, act, slope, eps, _p(ws), ws.numel() * 8, _st()),
          'bias_act_stats')
    return y, mean, rstd


def k_blur_act_bwd(g, y, slope, bias_scale, want_gb):
    """``y``: the LeakyReLU output, or its sign bits (``k_blur_bits``)."""
    g = _aligned16(_c(g))
    n, c, h, w = g.shape
    out = torch.empty_like(g)
    gb = _take('gb', (c,), g) if want_gb else None
    ws = _blur_ws(g) if want_gb else None
    if _is_bits(y):
        assert y.numel() * 32 == g.numel()
        check(_lib.lib().ganlab_blur_act_bwd_bits_f32(_p(g), y.data_ptr(), _p(out), _p(gb), n, c, h, w, slope, bias_scale,
                                                      _p(ws), ws.numel() * 4 if ws is not None else 0, _st()),
              'blur_act_bwd_bits')
        return out, gb
    y = _aligned16(_c(y))
    assert g.shape == y.shape
    check(_lib.lib().ganlab_blur_act_bwd_f32(_p(g), _p(y), _p(out), _p(gb), n, c, h, w, slope, bias_scale, _p(ws),
                                             ws.numel() * 4 if ws is not None else 0, _st()), 'blur_act_bwd')
    return out, gb


def k_act_bwd_blur(g, y, noise, slope, bias_scale, want_gb, want_gnw):
    g = _aligned16(_c(g))
    noise = _aligned16(_c(noise)) if want_gnw else None
    n, c, h, w = g.shape
    out = torch.empty_like(g)
    gb = _take('gb', (c,), g) if want_gb else None
    gnw = _take('gnw', (c,), g) if want_gnw else None
    ws = _blur_ws(g) if (want_gb or want_gnw) else None
    if _is_bits(y):
        assert y.numel() * 32 == g.numel()
        check(_lib.lib().ganlab_act_bwd_blur_bits_f32(_p(g), y.data_ptr(), _p(noise), _p(out),
                                                      _p(gb), _p(gnw), n, c, h, w, slope, bias_scale, _p(ws),
                                                      ws.numel() * 4 if ws is not None else 0, _st()), 'act_bwd_blur_bits')
        return out, gb, gnw
    y = _aligned16(_c(y))
    assert g.shape == y.shape
    check(_lib.lib().ganlab_act_bwd_blur_f32(_p(g), _p(y), _p(noise), _p(out), _p(gb),
                                             _p(gnw), n, c, h, w, slope, bias_scale, _p(ws),
                                             ws.numel() * 4 if ws is not None else 0, _st()), 'act_bwd_blur')
    return out, gb, gnw


# ---------------------------------------------------------------------------------------------- #
# convolution: three mutually-recursive Functions (bilinear form  C(x, w) = s * conv(up?(x), w))
# ---------------------------------------------------------------------------------------------- #
class _ConvFwd(Function):
    @staticmethod
    def forward(ctx, x, w, g, s):
        ctx.save_for_backward(x, w)
        ctx.g, ctx.s = g, s
        return k_conv_fwd(x, w, None, g, s)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = _ConvDgrad.apply(gy, w, ctx.g, ctx.s) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1] and _want_param_grads():
            _sink('gw', w)
            gw = _ConvWgrad.apply(gy, x, ctx.g, ctx.s)
            if _sunk('gw'):
                gw = None
        return gx, gw, None, None


class _ConvDgrad(Function):
    @staticmethod
    def forward(ctx, gy, w, g, s):
        ctx.save_for_backward(gy, w)
        ctx.g, ctx.s = g, s
        return k_conv_dgrad(gy, w, g, s)

    @staticmethod
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        d_gy = _ConvFwd.apply(ggx, w, ctx.g, ctx.s) if ctx.needs_input_grad[0] else None
        d_w = _ConvWgrad.apply(gy, ggx, ctx.g, ctx.s) if ctx.needs_input_grad[1] else None
        return d_gy, d_w, None, None


class _ConvDgradMask(Function):
    """gx = dgrad(gy, w) * lrelu'(x) in the dgrad kernel's epilogue: x, the conv's input, is the LeakyReLU output of the
    layer in front, whose backward then receives the gradient of its PRE-activation (see ``conv2d(defer_act_grad=)``)."""

    @staticmethod
    def forward(ctx, gy, w, x, g, s, slope):
        ctx.save_for_backward(gy, w, x)
        ctx.g, ctx.s, ctx.slope = g, s, slope
        return k_conv_dgrad_mask(gy, w, x, g, s, slope)

    @staticmethod
    def backward(ctx, ggx):
        gy, w, x = ctx.saved_tensors
        t = _ActBwd.apply(ggx, x, ctx.slope)
        d_gy = _ConvFwd.apply(t, w, ctx.g, ctx.s) if ctx.needs_input_grad[0] else None
        d_w = _ConvWgrad.apply(gy, t, ctx.g, ctx.s) if ctx.needs_input_grad[1] else None
        return d_gy, d_w, None, None, None, None


class _DeferredActGrad(Function):
    """Identity whose backward applies lrelu'(x): the explicit form of what _ConvDgradMask folds into the dgrad kernel,
    for consumers of a ``defer_act_grad`` tensor that cannot fold it in."""

    @staticmethod
    def forward(ctx, x, slope):
        ctx.save_for_backward(x)
        ctx.slope = slope
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return _ActBwd.apply(g, x, ctx.slope), None


class _ConvWgrad(Function):
    @staticmethod
    def forward(ctx, gy, x, g, s):
        ctx.save_for_backward(gy, x)
        ctx.g, ctx.s = g, s
        return k_conv_wgrad(gy, x, g, s)

    @staticmethod
    def backward(ctx, ggw):
        gy, x = ctx.saved_tensors
        d_gy = _ConvFwd.apply(x, ggw, ctx.g, ctx.s) if ctx.needs_input_grad[0] else None
        d_x = _ConvDgrad.apply(gy, ggw, ctx.g, ctx.s) if ctx.needs_input_grad[1] else None
        return d_gy, d_x, None, None


# The three maps below fold m = lrelu'(y) (y: the conv's activated output, a constant of all of them) into the conv
# gradient kernels; they are each other's derivatives, so R1 / WGAN-GP second-order sweeps stay on fused kernels.
class _ConvDgradAct(Function):
    """gx = dgrad(gy * m, w)."""

    @staticmethod
    def forward(ctx, gy, y, w, g, s, slope):
        ctx.save_for_backward(gy, y, w)
        ctx.g, ctx.s, ctx.slope = g, s, slope
        return k_conv_dgrad_act(gy, y, w, g, s, slope)

    @staticmethod
    def backward(ctx, ggx):
        gy, y, w = ctx.saved_tensors
        d_gy = _ConvFwdMask.apply(ggx, w, y, ctx.g, ctx.s, ctx.slope) if ctx.needs_input_grad[0] else None
        d_w = _ConvWgradAct.apply(gy, y, ggx, ctx.g, ctx.s, ctx.slope, 1.0, False)[0] if ctx.needs_input_grad[2] \
            else None
        return d_gy, None, d_w, None, None, None


class _ConvFwdMask(Function):
    """out = conv(x, w) * m."""

    @staticmethod
    def forward(ctx, x, w, y, g, s, slope):
        ctx.save_for_backward(x, w, y)
        ctx.g, ctx.s, ctx.slope = g, s, slope
        return k_conv_fwd_mask(x, w, y, g, s, slope)

    @staticmethod
    def backward(ctx, go):
        x, w, y = ctx.saved_tensors
        d_x = _ConvDgradAct.apply(go, y, w, ctx.g, ctx.s, ctx.slope) if ctx.needs_input_grad[0] else None
        d_w = _ConvWgradAct.apply(go, y, x, ctx.g, ctx.s, ctx.slope, 1.0, False)[0] if ctx.needs_input_grad[1] else None
        return d_x, d_w, None, None, None, None


class _ConvWgradAct(Function):
    """(gw, gb) = (wgrad(gy * m, x), bias_scale * sum(gy * m))."""

    @staticmethod
    def forward(ctx, gy, y, x, g, s, slope, bias_scale, want_gb):
        ctx.save_for_backward(gy, y, x)
        ctx.g, ctx.s, ctx.slope = g, s, slope
        gw, gb = k_conv_wgrad_act(gy, y, x, g, s, slope, bias_scale, want_gb)
        if gb is None:
            gb = gw.new_zeros(())
            ctx.mark_non_differentiable(gb)
        return gw, gb

    @staticmethod
    def backward(ctx, ggw, ggb):
        if ggb is not None and ggb.numel() > 1 and bool(ggb.ne(0).any()):
            raise NotImplementedError('second derivative through the fused fromRGB bias gradient')
        gy, y, x = ctx.saved_tensors
        d_gy = _ConvFwdMask.apply(x, ggw, y, ctx.g, ctx.s, ctx.slope) if ctx.needs_input_grad[0] else None
        d_x = _ConvDgradAct.apply(gy, y, ggw, ctx.g, ctx.s, ctx.slope) if ctx.needs_input_grad[2] else None
        return d_gy, None, d_x, None, None, None, None, None


BLUR_HANDOFF = '_ganlab_blur_handoff'


class BlurHandoff(object):
    """Link between the critic's  conv -> LeakyReLU -> blur  layer (A) and the pooled conv (B) that is its only reader
    (progan/architectures.py:254-284): B's input-gradient kernel can apply A's blur^T and LeakyReLU derivative and sum A's bias
    gradient on the way (csrc/conv_s2_roll_blur.hip).  A fills in what that takes at forward time; B's backward sets ``done``
    and ``gb``, A's backward - which always runs after it - then takes the incoming gradient as that of its pre-activation."""
    __slots__ = ('bits', 'slope', 'bias_scale', 'want_gb', 'gb', 'done')

    def __init__(self):
        self.bits, self.slope, self.bias_scale, self.want_gb, self.gb, self.done = None, 0.2, 1.0, False, None, False


RGB_HANDOFF = '_ganlab_rgb_handoff'


class RgbHandoff(object):
    """Link between the critic's fromRGB layer (1x1 conv of the image + LeakyReLU, progan/architectures.py:232-237) and the 3x3
    conv that is its only reader: where nobody needs fromRGB's input gradient (the critic steps on detached fakes, and on the
    real batch under ``no_grad_towards``), the reader's input-gradient kernel can finish fromRGB's backward itself - mask by
    the sign bits, weight / bias gradient sums against the image - and never write the 2 GiB gradient tensor between them
    (csrc/conv_roll_blur.hip, RB_RGB).  Only inside ``direct_param_grads`` (the sums go straight into the arena slots)."""
    __slots__ = ('bits', 'slope', 'img', 'w', 'bias', 'scale', 'bias_scale')

    def __init__(self):
        self.bits = None


def _rgb_fold_ok(h, g):
    """May the input gradient of the conv with geometry ``g`` swallow the backward of the fromRGB layer ``h`` describes?"""
    if h is None or h.bits is None or torch.is_grad_enabled() or not _DIRECT[0] or not _want_param_grads() or \
            os.environ.get('GANLAB_RGB_FOLD') == '0' or get_compute_dtype() != 'f32':
        return False
    x = h.img
    if x.requires_grad and not (_NO_GRAD_TOWARDS[0] is not None and x.grad_fn is None and x.data_ptr() == _NO_GRAD_TOWARDS[0]):
        return False            # somebody wants d / d image: the gradient tensor has to exist
    for p_ in (h.w, h.bias):
        if p_ is None:
            continue
        base = p_._base if p_._base is not None else p_
        if not base.requires_grad or getattr(base, '_ganlab_arena', None) is None or base.grad is None or \
                base.numel() != p_.numel():
            return False
    return bool(_lib.lib().ganlab_conv_dgrad_rgb_sums_supported(g.ref(), int(x.shape[1])))


def k_conv_dgrad_rgb_sums(gz, w, h, g, scale):
    """Input gradient of the 3x3 conv ``g`` on ``gz`` folded with fromRGB's backward: fromRGB's weight / bias gradients are
    added into their arena slots; nothing else is written."""
    gz, w = _c(gz, 'conv grad_out'), _c(w, 'conv weight')
    assert tuple(gz.shape) == g.out_shape
    _note('dgrad', g)
    L = _lib.lib()

    def slot(p_):
        base = p_._base if p_._base is not None else p_
        arena = base._ganlab_arena
        acc = getattr(base, '_ganlab_written', -1) == arena.serial
        base._ganlab_written = arena.serial
        return base.grad, int(acc)
    gw, acc_w = slot(h.w)
    gb, acc_b = slot(h.bias) if h.bias is not None else (None, 0)
    img = _c(h.img, 'image')
    ws = torch.empty((L.ganlab_conv_dgrad_rgb_sums_workspace(g.ref()) + 7) // 8, dtype=torch.float64, device=gz.device)
    check(L.ganlab_conv_dgrad_rgb_sums_f32(_p(gz), _p(_packed(w, PACK_DGRAD, scale)), h.bits.data_ptr(), _p(img), _p(gw), _p(gb),
                                           g.ref(), int(img.shape[1]), h.scale, h.bias_scale, h.slope, acc_w, acc_b,
                                           ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _st()), 'conv_dgrad_rgb_sums')


class _ConvDgradBlurAct(Function):
    """(gzA, gbA) = (lrelu'(bits) * blur(dgrad_B(gy, w)), bias_scale * sum gzA) in one kernel; linear in gy and in w.  Its
    derivative is the composition the separate passes have: the adjoint of blur^T o mask (``_ActBwdBlur``), then the pooled
    conv's forward / weight gradient."""

    @staticmethod
    def forward(ctx, gy, w, bits, g, s, slope, bias_scale, want_gb):
        ctx.save_for_backward(gy, w, bits)
        ctx.set_materialize_grads(False)
        ctx.g, ctx.s, ctx.slope = g, s, slope
        gz, gb = k_conv_s2_dgrad_blur_act(gy, w, bits, g, s, slope, bias_scale, want_gb)
        if gb is None:
            gb = gz.new_zeros(())
            ctx.mark_non_differentiable(gb)
        return gz, gb

    @staticmethod
    def backward(ctx, gg, ggb):
        if ggb is not None:
            raise NotImplementedError('second derivative through the fused bias gradient of the blurred layer')
        gy, w, bits = ctx.saved_tensors
        if gg is None:
            return (None,) * 8
        t = _ActBwdBlur.apply(gg, bits, None, ctx.slope, 1.0, False, False)[0]
        d_gy = _ConvFwd.apply(t, w, ctx.g, ctx.s) if ctx.needs_input_grad[0] else None
        d_w = _ConvWgrad.apply(gy, t, ctx.g, ctx.s) if ctx.needs_input_grad[1] else None
        return d_gy, d_w, None, None, None, None, None, None


class _BlurActBwd(Function):
    """(out, gb) = (lrelu'(y) * blur(g), bias_scale * sum_{n,hw} out): the backward of  conv+bias+LeakyReLU
    -> blur  in one pass.  Linear in g; its adjoint is _ActBwdBlur."""

    @staticmethod
    def forward(ctx, g, y, slope, bias_scale, want_gb):
        ctx.save_for_backward(y)          # the LeakyReLU output, or its sign bits (k_blur_bits)
        ctx.set_materialize_grads(False)
        ctx.slope, ctx.bias_scale, ctx.gshape = slope, bias_scale, g.shape
        return k_blur_act_bwd(g, y, slope, bias_scale, want_gb)

    @staticmethod
    def backward(ctx, gout, ggb):
        y, = ctx.saved_tensors
        g = gout
        if ggb is not None:
            shape = ctx.gshape
            b = _Scale.apply(ggb.view(1, shape[1], 1, 1).expand(shape), ctx.bias_scale)
            g = b if g is None else _Axpby.apply(g, b, 1.0, 1.0)
        if g is None:
            return None, None, None, None, None
        return _ActBwdBlur.apply(g, y, None, ctx.slope, 1.0, False, False)[0], None, None, None, None


class _ActBwdBlur(Function):
    """(out, gb, gnw) = (blur(z), bias_scale*sum z, sum z*noise) with z = lrelu'(y) * g: the backward of
    blur -> noise/bias/LeakyReLU in one pass.  Linear in g; its adjoint is _BlurActBwd."""

    @staticmethod
    def forward(ctx, g, y, noise, slope, bias_scale, want_gb, want_gnw):
        ctx.save_for_backward(y)
        ctx.set_materialize_grads(False)
        ctx.slope = slope
        return k_act_bwd_blur(g, y, noise, slope, bias_scale, want_gb, want_gnw)

    @staticmethod
    def backward(ctx, gout, ggb, ggnw):
        if ggb is not None or ggnw is not None:
            raise NotImplementedError('double backward through the bias / noise-weight gradients of the fused blur')
        y, = ctx.saved_tensors
        if gout is None:
            return (None,) * 7
        return (_BlurActBwd.apply(gout, y, ctx.slope, 1.0, False)[0],) + (None,) * 6


class _BlurBiasAct(Function):
    """y = act(blur(x) + noise_w*noise + bias*bias_scale): the blur after a generator up-conv fused with
    StyleAddNoise / Conv2dBias / LeakyReLU (stylegan/architectures.py:331-360 + :105-119)."""

    @staticmethod
    def forward(ctx, x, bias, noise, noise_w, bias_scale, act, slope, stats_eps=None):
        stats = None
        if stats_eps is None:
            y = k_blur_bias_act(x, bias, noise, noise_w, bias_scale, act, slope)
        else:    # + the InstanceNorm statistics of y in the same pass (handed to instnorm_style as constants)
            y, mean, rstd = k_blur_bias_act_stats(x, bias, noise, noise_w, bias_scale, act, slope, stats_eps)
            ctx.mark_non_differentiable(mean, rstd)
            stats = (mean, rstd)
        ctx.save_for_backward(y if act != ACT_NONE else None, noise)
        ctx.bias_scale, ctx.act, ctx.slope = bias_scale, act, slope
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.nw_shape = noise_w.shape if noise_w is not None else None
        ctx.bias_ref, ctx.nw_ref = bias, noise_w
        return y if stats is None else (y,) + stats

    @staticmethod
    def backward(ctx, gy, *_):
        y, noise = ctx.saved_tensors
        params = _want_param_grads()
        want_b = ctx.bias_shape is not None and ctx.needs_input_grad[1] and params
        want_nw = ctx.nw_shape is not None and ctx.needs_input_grad[3] and params
        act = ctx.act != ACT_NONE
        _sink('gb', ctx.bias_ref if want_b else None)
        _sink('gnw', ctx.nw_ref if want_nw else None)
        gx, gb, gnw = _ActBwdBlur.apply(gy, y if act else gy, noise if want_nw else None,
                                        ctx.slope if act else 1.0, ctx.bias_scale, bool(want_b), bool(want_nw))
        if _sunk('gb'):
            want_b = False
        if _sunk('gnw'):
            want_nw = False
        return (gx if ctx.needs_input_grad[0] else None), (gb.view(ctx.bias_shape) if want_b else None), None, \
            (gnw.view(ctx.nw_shape) if want_nw else None), None, None, None, None


class _ConvBiasAct(Function):
    """y = act(s*conv(up?(x), w) + bias*bias_scale) in ONE kernel (bias/LeakyReLU in the MFMA
    epilogue).  Reference: Conv2dEx.forward (+ nn.LeakyReLU) custom_layers.py:202-211."""

    @staticmethod
    def forward(ctx, x, w, bias, g, s, bias_scale, act, slope, blur=False, defer=False, in_slope=None, handoff_out=None,
                handoff_in=None, rgb_out=None, rgb_in=None):
        # defer: the (single) consumer of y applies this layer's lrelu'(y) to the gradient it sends back (its dgrad
        # epilogue), so backward takes gy as the pre-activation gradient.  in_slope: this conv IS such a consumer.
        ctx.g, ctx.s, ctx.bias_scale, ctx.act, ctx.slope, ctx.blur = g, s, bias_scale, act, slope, blur
        ctx.bias_ref = bias
        # an undefined incoming gradient stays undefined (RgbHandoff: the reader of a fromRGB layer may have finished this
        # layer's backward itself and sends nothing; materialised, that would be a 2 GiB tensor of zeros and two passes over it)
        ctx.set_materialize_grads(False)
        # handoff_out: this is layer A of a BlurHandoff pair (filled in below when the sign bits exist); handoff_in: layer B
        ctx.handoff_out, ctx.handoff_in = None, handoff_in
        ctx.rgb_in = rgb_in         # this conv reads a fromRGB layer's output (RgbHandoff)
        if act != ACT_NONE and not blur and not defer and in_slope is None and conv_act_bwd_fusable(g) and \
                (g.Ho * g.Wo) % 32 == 0 and mask_bits_ok_plane():
            # fromRGB: the gradient kernels take (gy, mask of y); the forward writes that mask as bits next to y
            y, bits = k_conv_fwd_bits(x, w, bias, g, s, bias_scale, act, slope)
            ctx.defer, ctx.in_slope = False, None
            ctx.bias_shape = bias.shape if bias is not None else None
            ctx.save_for_backward(x, w, bits)
            if rgb_out is not None and g.ks == 1:       # fromRGB: its only reader may finish this layer's backward
                rgb_out.bits, rgb_out.slope, rgb_out.img, rgb_out.w, rgb_out.bias = bits, slope, x, w, bias
                rgb_out.scale, rgb_out.bias_scale = s, bias_scale
            return y
        ctx.defer, ctx.in_slope = bool(defer), in_slope
        assert not (defer and blur)
        ctx.bias_shape = bias.shape if bias is not None else None
        if blur and act == ACT_LRELU:
            # thin layer: conv + bias + LeakyReLU + blur + the sign bits in one rolling-window kernel
            fused = k_conv_fwd_blur_bits(x, w, bias, g, s, bias_scale, slope)
            if fused is not None:
                ctx.save_for_backward(x, w, fused[1])
                ctx.handoff_out = _fill_handoff(handoff_out, fused[1], slope, bias_scale, bias)
                return fused[0]
        y = k_conv_fwd(x, w, bias, g, s, bias_scale, act, slope)
        # blur=True: the D block's  conv -> bias -> LeakyReLU -> blur  (progan/architectures.py:280-293);
        # forward is conv kernel + blur kernel, backward is ONE pass (blur^T, LeakyReLU', bias gradient)
        if blur and act != ACT_NONE and mask_bits_ok(y):
            # the backward only ever needs sign(y): the blur pass emits it as bits and y itself is not kept (a 2 GiB
            # tensor per pass at the top of the critic; the backward passes read 1/32 of its bytes)
            out, bits = k_blur_bits(y)
            ctx.save_for_backward(x, w, bits)
            ctx.handoff_out = _fill_handoff(handoff_out, bits, slope, bias_scale, bias)
            return out
        ctx.save_for_backward(x, w, y if (act != ACT_NONE and not defer) else None)
        return k_blur(y) if blur else y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return (None,) * 15
        x, w, y = ctx.saved_tensors
        params = _want_param_grads()
        want_b = ctx.bias_shape is not None and ctx.needs_input_grad[2] and params
        gb = None
        act = ACT_NONE if ctx.defer else ctx.act
        if act != ACT_NONE and not ctx.blur and ctx.in_slope is None and conv_act_bwd_fusable(ctx.g):
            # fromRGB: no separate  gz = gy * lrelu'(y)  pass - its gradient kernels take (gy, y)
            gx = _ConvDgradAct.apply(gy, y, w, ctx.g, ctx.s, ctx.slope) if _wants_input_grad(ctx, x) else None
            gw = None
            if params and (ctx.needs_input_grad[1] or want_b):
                _sink('gw', w if ctx.needs_input_grad[1] else None)
                _sink('gb', ctx.bias_ref if want_b else None)
                gw, gb = _ConvWgradAct.apply(gy, y, x, ctx.g, ctx.s, ctx.slope, ctx.bias_scale, bool(want_b))
                if _sunk('gw'):
                    gw = None
                if _sunk('gb'):
                    want_b = False
            return gx, (gw if ctx.needs_input_grad[1] else None), (gb.view(ctx.bias_shape) if want_b else None), \
                None, None, None, None, None, None, None, None, None, None, None, None
        h = ctx.handoff_out
        if h is not None and h.done:
            # the pooled conv behind the blur already applied blur^T and this layer's LeakyReLU derivative in its input-
            # gradient kernel (and summed the bias gradient): gy IS the pre-activation gradient
            gz, gb = gy, (h.gb if want_b else None)
            h.done, h.gb = False, None
        elif ctx.blur and act != ACT_NONE:
            _sink('gb', ctx.bias_ref if want_b else None)
            gz, gb = _BlurActBwd.apply(gy, y, ctx.slope, ctx.bias_scale, bool(want_b))
        else:
            _sink('gb', ctx.bias_ref if want_b else None)
            if ctx.blur:
                gy = _Blur.apply(gy)
            if act != ACT_NONE and want_b:
                gz, gb = _ActBwdBias.apply(gy, y, ctx.slope, ctx.bias_scale)
            else:
                gz = _ActBwd.apply(gy, y, ctx.slope) if act != ACT_NONE else gy
                if want_b:
                    gb = _ChanSum.apply(gz, None, ctx.bias_scale, 'gb')
        if _sunk('gb'):
            gb = None
        gx = None
        if _wants_input_grad(ctx, x) and ctx.in_slope is None and ctx.handoff_in is None and _rgb_fold_ok(ctx.rgb_in, ctx.g):
            # x is fromRGB's output and nobody needs fromRGB's input gradient: this conv's input-gradient kernel sums
            # fromRGB's weight / bias gradients into their arena slots; the gradient tensor in between is never written
            k_conv_dgrad_rgb_sums(gz, w, ctx.rgb_in, ctx.g, ctx.s)
        elif _wants_input_grad(ctx, x):
            hin = ctx.handoff_in
            if hin is not None:      # layer B of the pair: input gradient + layer A's blur^T, LeakyReLU', bias gradient
                gx, gba = _ConvDgradBlurAct.apply(gz, w, hin.bits, ctx.g, ctx.s, hin.slope, hin.bias_scale,
                                                  bool(hin.want_gb and params))
                hin.gb, hin.done = (gba if (hin.want_gb and params) else None), True
            else:
                gx = _ConvDgrad.apply(gz, w, ctx.g, ctx.s) if ctx.in_slope is None else \
                    _ConvDgradMask.apply(gz, w, x, ctx.g, ctx.s, ctx.in_slope)
        gw = None
        if ctx.needs_input_grad[1] and params:
            _sink('gw', w)
            gw = _ConvWgrad.apply(gz, x, ctx.g, ctx.s)
            if _sunk('gw'):
                gw = None
        return gx, gw, (gb.view(ctx.bias_shape) if want_b and gb is not None else None), None, None, None, None, \
            None, None, None, None, None, None, None, None


def _fill_handoff(h, bits, slope, bias_scale, bias):
    if h is not None:
        h.bits, h.slope, h.bias_scale = bits, slope, bias_scale
        h.want_gb = bias is not None and bias.requires_grad
        h.gb, h.done = None, False
    return h


class _BiasAct(Function):
    """y = act(x + noise_w*noise + bias*bias_scale)  (Conv2dBias + StyleAddNoise + LeakyReLU:
    custom_layers.py:213-226, stylegan/architectures.py:105-119)."""

    @staticmethod
    def forward(ctx, x, bias, noise, noise_w, bias_scale, act, slope, stats_eps=None):
        stats = None
        if stats_eps is None:
            y = k_bias_act(x, bias, noise, noise_w, bias_scale, act, slope)
        else:
            y, mean, rstd = k_bias_act_stats(x, bias, noise, noise_w, bias_scale, act, slope, stats_eps)
            ctx.mark_non_differentiable(mean, rstd)
            stats = (mean, rstd)
        ctx.save_for_backward(y if act != ACT_NONE else None, noise)
        ctx.bias_scale, ctx.act, ctx.slope = bias_scale, act, slope
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.nw_shape = noise_w.shape if noise_w is not None else None
        ctx.bias_ref, ctx.nw_ref = bias, noise_w
        return y if stats is None else (y,) + stats

    @staticmethod
    def backward(ctx, gy, *_):
        y, noise = ctx.saved_tensors
        params = _want_param_grads()
        want_b = ctx.bias_shape is not None and ctx.needs_input_grad[1] and params
        gb = gnw = None
        _sink('gb', ctx.bias_ref if want_b else None)
        if ctx.act != ACT_NONE and want_b:
            gz, gb = _ActBwdBias.apply(gy, y, ctx.slope, ctx.bias_scale)
        else:
            gz = _ActBwd.apply(gy, y, ctx.slope) if ctx.act != ACT_NONE else gy
            if want_b:
                gb = _ChanSum.apply(gz, None, ctx.bias_scale, 'gb')
        if _sunk('gb'):
            gb = None
        if ctx.nw_shape is not None and ctx.needs_input_grad[3] and params:
            _sink('gnw', ctx.nw_ref)
            gnw = _ChanSum.apply(gz, noise, 1.0, 'gnw').view(ctx.nw_shape)
            if _sunk('gnw'):
                gnw = None
        return (gz if ctx.needs_input_grad[0] else None), (gb.view(ctx.bias_shape) if gb is not None else None), \
            None, gnw, None, None, None, None


# ---------------------------------------------------------------------------------------------- #
# normalisation (generator side: first-order only)
# ---------------------------------------------------------------------------------------------- #
class _InstNormStyle(Function):
    """y = InstanceNorm(x; eps, biased var) * (ys + 1) + yb  with style (N, 2C) = [ys | yb]
    (custom_layers.py:98-99 + stylegan/architectures.py:524-526); style=None -> plain IN."""

    @staticmethod
    def forward(ctx, x, style, eps, mean=None, rstd=None):
        x = _c(x)
        n, c, hw = _nchw(x)
        L = _lib.lib()
        if mean is None:     # otherwise: produced by the kernel that wrote x (bias_act(..., stats_eps=eps))
            mean, rstd = _new((n * c,), x), _new((n * c,), x)
            check(L.ganlab_instnorm_stats_f32(_p(x), _p(mean), _p(rstd), n * c, hw, eps, _st()), 'instnorm_stats')
        assert mean.numel() == n * c and rstd.numel() == n * c
        style_c = _c(style) if style is not None else None
        if style_c is not None:
            assert style_c.numel() == n * 2 * c
        y = torch.empty_like(x)
        check(L.ganlab_instnorm_style_fwd_f32(_p(x), _p(mean), _p(rstd), _p(style_c), _p(y), n, c, hw, _st()),
              'instnorm_style_fwd')
        ctx.save_for_backward(x, mean, rstd, style_c)
        ctx.style_shape = style.shape if style is not None else None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, mean, rstd, style = ctx.saved_tensors
        gy = _c(gy)
        n, c, hw = _nchw(x)
        L = _lib.lib()
        s1, s2 = _new((n, c), x), _new((n, c), x)
        check(L.ganlab_instnorm_style_bwd_reduce_f32(_p(gy), _p(x), _p(mean), _p(rstd), _p(s1), _p(s2), n * c, hw,
                                                     _st()), 'instnorm_bwd_reduce')
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            check(L.ganlab_instnorm_style_bwd_apply_f32(_p(gy), _p(x), _p(mean), _p(rstd), _p(style), _p(s1), _p(s2),
                                                        _p(gx), n, c, hw, _st()), 'instnorm_bwd_apply')
        gstyle = None
        if style is not None and ctx.needs_input_grad[1]:
            gstyle = torch.stack((s2, s1), dim=1).reshape(ctx.style_shape)  # d/dys = sum gy*xhat ; d/dyb = sum gy
        return gx, gstyle, None, None, None


class _LayerTail(Function):
    """out = InstanceNorm(act(blur?(x) + noise_w*noise + bias*bias_scale)) * (ys+1) + yb: everything of a generator
    layer after its convolution (stylegan/architectures.py:497-526) as two forward passes (the first one also accumulates
    the InstanceNorm statistics) and, backward, the reduce pass + ONE apply pass that also undoes the LeakyReLU and sums
    the bias / noise-weight gradients (+ blur^T when ``blur``).  First order only, like _InstNormStyle."""

    @staticmethod
    def forward(ctx, x, bias, noise, noise_w, style, bias_scale, act, slope, blur, eps):
        kern = k_blur_bias_act_stats if blur else k_bias_act_stats
        noise = _aligned16(_c(noise)) if noise is not None else None
        y, mean, rstd = kern(x, bias, noise, noise_w, bias_scale, act, slope, eps)
        n, c, hw = _nchw(y)
        style_c = _c(style) if style is not None else None
        if style_c is not None:
            assert style_c.numel() == n * 2 * c
        out = torch.empty_like(y)
        check(_lib.lib().ganlab_instnorm_style_fwd_f32(_p(y), _p(mean), _p(rstd), _p(style_c), _p(out), n, c, hw, _st()),
              'instnorm_style_fwd')
        ctx.save_for_backward(y, mean, rstd, style_c, noise)
        ctx.bias_scale, ctx.act, ctx.slope, ctx.blur = bias_scale, act, slope, blur
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.nw_shape = noise_w.shape if noise_w is not None else None
        ctx.bias_ref, ctx.nw_ref = bias, noise_w
        ctx.style_shape = style.shape if style is not None else None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        ctx.want_x_grad, ctx.want_bias_grad = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.want_nw_grad, ctx.want_style_grad = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        gz, gb, gnw, gstyle = _layer_tail_backward(ctx, ctx.saved_tensors, gout, blur=ctx.blur)
        return (gz if ctx.want_x_grad else None), gb, None, gnw, gstyle, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- #
# deferred InstanceNorm ("modulated" consumers; csrc/mod.hip)
# ---------------------------------------------------------------------------------------------- #
class Deferred(object):
    """The output ``a * s[n,c] + t[n,c]`` of a generator layer (InstanceNorm + AdaIN of the activated tensor ``a``) that
    has NOT been written to memory: its consumer applies it (per-sample weights / border-class bias, csrc/mod.hip).
    Gradient contract: whoever consumes ``a`` sends back d loss / d (a*s + t) - the gradient with respect to the
    NORMALISED tensor - as the gradient of ``a``; ``_LayerTailDeferred.backward`` is the InstanceNorm backward of that
    (exactly what the materialised path feeds it), so ``s`` / ``t`` carry no gradient of their own."""
    __slots__ = ('a', 's', 't', 'mean', 'rstd', 'style', 'link')

    def __init__(self, a, s, t, mean, rstd, style, link=None):
        self.a, self.s, self.t, self.mean, self.rstd, self.style, self.link = a, s, t, mean, rstd, style, link

    def read(self):
        """Called by every consumer of ``a`` (see ``RgbGradLink``); returns self."""
        if self.link is not None:
            self.link.readers += 1
        return self

    @property
    def shape(self):
        return self.a.shape


class RgbGradLink(object):
    """Link between a generator layer's tail (the producer of a ``Deferred``) and toRGB where toRGB is its ONLY reader (the
    last layer outside the fade-in, stylegan/architectures.py:398-402): toRGB's input gradient is a 1x1 conv of the <= 4-plane
    image gradient, cheaper to recompute inside the tail's two InstanceNorm backward passes than to write as C planes and
    read back twice (csrc/pointwise.hip, RgbSrc).  toRGB's backward fills ``grgb`` / ``wp`` / ``crgb`` and returns a
    placeholder for the gradient of ``a``; the tail's backward - which always runs after it - reads them instead."""
    __slots__ = ('readers', 'grgb', 'wp', 'crgb')

    def __init__(self):
        self.readers, self.grgb, self.wp, self.crgb = 0, None, None, 0


def _rgb_link_ok(link, n, c, crgb, hw):
    return link is not None and link.readers == 1 and get_compute_dtype() == 'f32' and \
        os.environ.get('GANLAB_TORGB_FOLD') != '0' and \
        bool(_lib.lib().ganlab_instnorm_bwd_rgb_supported(n, c, crgb, hw))


def _affine_from_stats(mean, rstd, style, n, c):
    """s = rstd * (ys + 1), t = yb - mean * s  as (N, C) tensors (style: (N, 2C) = [ys | yb] or None)."""
    s_, t_ = _new((n, c), mean), _new((n, c), mean)
    check(_lib.lib().ganlab_in_affine_f32(_p(mean), _p(rstd), _p(style), _p(s_), _p(t_), n, c, _st()), 'in_affine')
    return s_, t_


def _layer_tail_backward(ctx, saved_tail, gout, blur=False):
    """Shared by _LayerTail / _LayerTailDeferred / _ConvModTail: InstanceNorm + style backward of ``gout`` (the gradient
    with respect to the normalised tensor), LeakyReLU undone, bias / noise-weight / style gradients from the same pass.
    ``blur``: the tail sits behind a blur - the (self-adjoint) blur of gz runs in the SAME pass and gz is never written.
    Returns (gz or blur(gz), gb, gnw, gstyle)."""
    y, mean, rstd, style, noise = saved_tail
    noise = _aligned16(noise) if noise is not None else None
    n, c, hw = _nchw(y)
    L = _lib.lib()
    rgb = getattr(ctx, 'link', None)
    if rgb is not None and rgb.grgb is None:
        rgb = None
    params = _want_param_grads()
    want_b = ctx.bias_shape is not None and ctx.want_bias_grad and params
    want_nw = ctx.nw_shape is not None and ctx.want_nw_grad and params
    s1, s2 = _new((n, c), y), _new((n, c), y)
    if rgb is not None:            # ``gout`` is toRGB's placeholder: the gradient is recomputed from the image gradient
        assert not blur
        grgb, wp_rgb, crgb = _aligned16(rgb.grgb), rgb.wp, rgb.crgb
        rgb.grgb = rgb.wp = None
        wsr = torch.empty((L.ganlab_instnorm_bwd_reduce_rgb_workspace(n, c, hw) + 3) // 4, dtype=torch.float32,
                          device=y.device)
        check(L.ganlab_instnorm_style_bwd_reduce_rgb_f32(_p(grgb), _p(wp_rgb), crgb, _p(y), _p(mean), _p(rstd), _p(s1),
                                                         _p(s2), n, c, hw, _p(wsr), wsr.numel() * 4, _st()),
              'instnorm_bwd_reduce_rgb')
    else:
        gout = _aligned16(_c(gout))     # (the apply passes below only have float4 forms)
        check(L.ganlab_instnorm_style_bwd_reduce_f32(_p(gout), _p(y), _p(mean), _p(rstd), _p(s1), _p(s2), n * c, hw,
                                                     _st()), 'instnorm_bwd_reduce')
    gz = gb = gnw = None
    if ctx.want_x_grad or want_b or want_nw:
        gz = torch.empty_like(y)
        _sink('gb', getattr(ctx, 'bias_ref', None) if want_b else None)
        _sink('gnw', getattr(ctx, 'nw_ref', None) if want_nw else None)
        gb = _take('gb', (c,), y) if want_b else None
        gnw = _take('gnw', (c,), y) if want_nw else None
        ws = torch.empty((L.ganlab_instnorm_bwd_act_workspace(n, c, hw) + 3) // 4, dtype=torch.float32,
                         device=y.device) if (want_b or want_nw) else None
        if rgb is not None:
            check(L.ganlab_instnorm_style_bwd_act_rgb_f32(_p(grgb), _p(wp_rgb), crgb, _p(y), _p(mean), _p(rstd), _p(style),
                                                          _p(s1), _p(s2), _p(noise) if want_nw else None, _p(gz), _p(gb),
                                                          _p(gnw), n, c, hw, ctx.act, ctx.slope, ctx.bias_scale, _p(ws),
                                                          ws.numel() * 4 if ws is not None else 0, _st()),
                  'instnorm_bwd_act_rgb')
        elif blur and blur_fusable(y):
            check(L.ganlab_instnorm_style_bwd_act_blur_f32(_p(gout), _p(y), _p(mean), _p(rstd), _p(style), _p(s1), _p(s2),
                                                           _p(noise) if want_nw else None, _p(gz), _p(gb), _p(gnw), n, c,
                                                           int(y.shape[2]), int(y.shape[3]), ctx.act, ctx.slope,
                                                           ctx.bias_scale, _p(ws), ws.numel() * 4 if ws is not None else 0,
                                                           _st()), 'instnorm_bwd_act_blur')
        else:
            check(L.ganlab_instnorm_style_bwd_act_f32(_p(gout), _p(y), _p(mean), _p(rstd), _p(style), _p(s1), _p(s2),
                                                      _p(noise) if want_nw else None, _p(gz), _p(gb), _p(gnw), n, c,
                                                      hw, ctx.act, ctx.slope, ctx.bias_scale, _p(ws),
                                                      ws.numel() * 4 if ws is not None else 0, _st()),
                  'instnorm_bwd_act')
            if blur and ctx.want_x_grad:
                gz = k_blur(gz)
    gstyle = None
    if style is not None and ctx.want_style_grad:
        gstyle = torch.stack((s2, s1), dim=1).reshape(ctx.style_shape)
    if _sunk('gb'):
        gb = None
    if _sunk('gnw'):
        gnw = None
    return gz, (gb.view(ctx.bias_shape) if gb is not None else None), \
        (gnw.view(ctx.nw_shape) if gnw is not None else None), gstyle


class _LayerTailDeferred(Function):
    """_LayerTail without its second pass: (a, s, t) with a = act(blur?(x) + noise_w*noise + bias*bias_scale) and the
    per-(n, c) scale / shift of InstanceNorm + style - see ``Deferred`` for the gradient contract."""

    @staticmethod
    def forward(ctx, x, bias, noise, noise_w, style, bias_scale, act, slope, blur, eps, link=None):
        kern = k_blur_bias_act_stats if blur else k_bias_act_stats
        noise = _aligned16(_c(noise)) if noise is not None else None
        ctx.link = link
        y, mean, rstd = kern(x, bias, noise, noise_w, bias_scale, act, slope, eps)
        n, c, _ = _nchw(y)
        style_c = _c(style) if style is not None else None
        s_, t_ = _affine_from_stats(mean, rstd, style_c, n, c)
        # (save_for_backward, not attributes: y is an OUTPUT of this node - holding it on ctx would be a reference
        # cycle that only Python's cyclic collector breaks, i.e. 2 GiB tensors freed late and a growing allocator)
        ctx.save_for_backward(y, mean, rstd, style_c, noise)
        ctx.bias_scale, ctx.act, ctx.slope, ctx.blur = bias_scale, act, slope, blur
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.nw_shape = noise_w.shape if noise_w is not None else None
        ctx.bias_ref, ctx.nw_ref = bias, noise_w
        ctx.style_shape = style.shape if style is not None else None
        ctx.want_x_grad, ctx.want_bias_grad = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.want_nw_grad, ctx.want_style_grad = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        ctx.mark_non_differentiable(s_, t_, mean, rstd)
        return y, s_, t_, mean, rstd

    @staticmethod
    @once_differentiable
    def backward(ctx, g_b, *_):
        gz, gb, gnw, gstyle = _layer_tail_backward(ctx, ctx.saved_tensors, g_b, blur=ctx.blur)
        gx = gz if ctx.want_x_grad else None
        return gx, gb, None, gnw, gstyle, None, None, None, None, None, None


class _Materialize(Function):
    """b = a*s + t written out (the second pass of round 1) for consumers without a modulated kernel; the gradient
    passes through unchanged (it IS d/db, which the deferred tail's backward expects)."""

    @staticmethod
    def forward(ctx, a, mean, rstd, style):
        n, c, hw = _nchw(a)
        out = torch.empty_like(a)
        check(_lib.lib().ganlab_instnorm_style_fwd_f32(_p(a), _p(mean), _p(rstd), _p(style), _p(out), n, c, hw, _st()),
              'instnorm_style_fwd')
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return g, None, None, None


def materialize(x):
    """Tensor for a plain consumer: a ``Deferred`` is normalised + styled now, a tensor is returned as is."""
    if isinstance(x, Deferred):
        x.read()
        return _Materialize.apply(x.a, x.mean, x.rstd, x.style)
    return x


_AFF_OK = {}      # (kind, shape, weight shape) -> bool: the support queries are pure functions of the geometry


def mod_conv_shape_ok(shape, weight, padding=1):
    """Can the 3x3 layer ``weight`` consume a deferred tensor of ``shape`` through the thin rolling-window kernel that also
    finishes the layer (noise, bias, LeakyReLU, statistics in its epilogue)?"""
    if get_compute_dtype() != 'f32' or padding != 1:
        return False
    key = ('mod', tuple(int(v) for v in shape), tuple(weight.shape))
    hit = _AFF_OK.get(key)
    if hit is None:
        n, cin, h, w = key[1]
        hit = False
        if tuple(weight.shape[1:]) == (cin, 3, 3):
            g = ConvGeom(n, cin, h, w, int(weight.shape[0]), 3, 1, 0, 0)
            hit = bool(_lib.lib().ganlab_mod_conv_supported(ctypes.byref(g)))
        _AFF_OK[key] = hit
    return hit


def conv_tail_shape_ok(shape, weight, padding=1):
    """The same one-pass layer on the tile kernels (thicker layers): affine on load, noise + bias + LeakyReLU + statistics in
    the conv's epilogue - where the affine-on-load forward AND weight gradient take the geometry."""
    if get_compute_dtype() != 'f32' or padding != 1:
        return False
    key = ('tail', tuple(int(v) for v in shape), tuple(weight.shape))
    hit = _AFF_OK.get(key)
    if hit is None:
        n, cin, h, w = key[1]
        hit = False
        if tuple(weight.shape[1:]) == (cin, 3, 3) and conv_aff_ok(shape, weight, False, padding):
            g = ConvGeom(n, cin, h, w, int(weight.shape[0]), 3, 1, 0, 0)
            hit = _lib.lib().ganlab_conv_fwd_aff_tail_chunks(ctypes.byref(g)) > 0
        _AFF_OK[key] = hit
    return hit


def mod_conv_ok(d, weight, padding=1):
    return isinstance(d, Deferred) and (mod_conv_shape_ok(d.a.shape, weight, padding) or
                                        conv_tail_shape_ok(d.a.shape, weight, padding))


def conv_aff_ok(shape, weight, up=False, padding=1):
    """Can the 3x3 conv ``weight`` (behind a nearest 2x upsample when ``up``) read a deferred tensor of ``shape`` through
    the affine-on-load kernels - forward AND weight gradient?"""
    if get_compute_dtype() != 'f32' or padding != 1:
        return False
    key = ('up' if up else 'plain', tuple(int(v) for v in shape), tuple(weight.shape))
    hit = _AFF_OK.get(key)
    if hit is None:
        n, cin, h, w = key[1]
        hit = False
        if tuple(weight.shape[1:]) == (cin, 3, 3):
            g = ConvGeom(n, cin, h, w, int(weight.shape[0]), 3, 1, 1 if up else 0, 0)
            L = _lib.lib()
            hit = (L.ganlab_conv_s2_aff_supported(ctypes.byref(g)) if up else L.ganlab_conv_aff_supported(ctypes.byref(g))) == 3
        _AFF_OK[key] = hit
    return hit


def deferrable(x):
    """A layer output of this shape can stay un-normalised for an affine-on-load consumer: the fused statistics pass
    takes it (plane >= 32x32, rows of whole float4s)."""
    if os.environ.get('GANLAB_DEFER') == '0':          # A/B knob: keep the two-pass layer tail of round 1
        return False
    n, c, h, w = x.shape
    return get_compute_dtype() == 'f32' and h * w >= STATS_MIN_PLANE and w % 4 == 0 and h % 2 == 0


def k_conv_fwd_aff(a, s_, t_, w, g, scale):
    """conv(up2?(a*s + t), w) * scale with the affine applied while the patch is staged (zero padding stays zero)."""
    a, w = _c(a, 'conv input'), _c(w, 'conv weight')
    assert tuple(a.shape) == g.in_shape and tuple(s_.shape) == (g.N, g.Cin) and tuple(t_.shape) == (g.N, g.Cin)
    _note('fwd', g)
    y = _new(g.out_shape, a)
    assert g.s2 or not g.up
    fam = _route_among(g, 'fwd', _AFF_FAMILIES[g.up])
    name = {X3_UP: 'conv_s2_fwd_aff_x3', S2: 'conv_s2_fwd_aff_f32', X3: 'conv_fwd_aff_x3', F32: 'conv_fwd_aff_f32'}[fam]
    check(getattr(_lib.lib(), 'ganlab_' + name)(_p(a), _p(_packed_for(fam, w, g, scale)), _p(s_), _p(t_), None, _p(y), g.ref(),
                                                1.0, ACT_NONE, 0.2, _st()), name)
    return y


def k_conv_wgrad_aff(gy, a, s_, t_, g, scale):
    """Weight gradient of conv(up2?(a*s + t), w): the x operand is normalised on the fly, like the forward's."""
    gy, a = _c(gy, 'conv grad_out'), _c(a, 'conv input')
    assert tuple(gy.shape) == g.out_shape and tuple(a.shape) == g.in_shape
    _note('wgrad', g)
    L = _lib.lib()
    gw = _take('gw', (g.Cout, g.Cin, 3, 3), a)
    fam = _route_among(g, 'wgrad', _AFF_FAMILIES[g.up])
    if fam in (X3, X3_UP):
        return _wgrad_x3(gy, a, _c(s_), _c(t_), gw, g, scale)
    name = 'conv_s2_wgrad' if g.up else 'conv_wgrad'
    ws = torch.empty((max(getattr(L, f'ganlab_{name}_workspace')(g.ref()), 4) + 3) // 4, dtype=torch.float32, device=a.device)
    check(getattr(L, f'ganlab_{name}_aff_f32')(_p(gy), _p(a), _p(s_), _p(t_), _p(gw), g.ref(), scale, _p(ws), ws.numel() * 4,
                                               _st()), name + '_aff')
    return gw


class _ConvAff(Function):
    """y = scale * conv(up2?(b), w) for the deferred tensor b = a*s + t (``Deferred``): the consumer's half of the
    deferred InstanceNorm.  Backward: d/da := d loss / d b (the contract of ``Deferred``) from the plain input-gradient
    kernel on the shared weights; the weight gradient contracts gy with the same on-the-fly b.  First order only."""

    @staticmethod
    def forward(ctx, a, s_, t_, w, g, scale):
        ctx.save_for_backward(a, s_, t_, w)
        ctx.g, ctx.scale = g, scale
        return k_conv_fwd_aff(a, s_, t_, w, g, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        a, s_, t_, w = ctx.saved_tensors
        ga = k_conv_dgrad(gy, w, ctx.g, ctx.scale) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[3] and _want_param_grads():
            _sink('gw', w)
            gw = k_conv_wgrad_aff(gy, a, s_, t_, ctx.g, ctx.scale)
            if _sunk('gw'):
                gw = None
        return ga, None, None, gw, None, None


def conv_aff(d, weight, scale, up=False):
    """3x3 'same' conv (behind a nearest 2x upsample when ``up``) of a ``Deferred`` tensor; see ``conv_aff_ok``."""
    n, cin, h, w = d.read().a.shape
    g = Geom(n, cin, h, w, weight.shape[0], 3, 1, 1 if up else 0, 0)
    return _ConvAff.apply(d.a, d.s, d.t, weight, g, float(scale))


class _ConvModTail(Function):
    """A plain thin 3x3 generator layer consuming a deferred input and producing a deferred output in ONE pass over the
    activations:  a_out = act(conv(a_in * s + t (zero padded), w) * scale + noise_w*noise + bias)  with the InstanceNorm
    statistics of a_out from the epilogue (csrc/mod.hip).  Backward: InstanceNorm backward of the incoming d/db_out (round-1
    kernels) -> gz; d/db_in = plain input-gradient kernel on the shared weights; the weight gradient is the rolling-window
    kernel with the affine on its x operand."""

    @staticmethod
    def forward(ctx, a_in, s_in, t_in, w, bias, noise, noise_w, style, scale, bias_scale, act, slope, eps, link=None):
        a_in, w = _c(a_in), _c(w)
        n, cin, h, wd = a_in.shape
        cout = w.shape[0]
        L = _lib.lib()
        ctx.link = link
        g = Geom(n, cin, h, wd, cout, 3, 1, 0)
        _note('fwd', g)
        noise = _c(noise) if noise is not None else None
        y = _new((n, cout, h, wd), a_in)
        mean, rstd = _new((n, cout), a_in), _new((n, cout), a_in)
        thin = mod_conv_shape_ok(a_in.shape, w)
        fam = F32 if thin else _route_among(g, 'fwd', (X3,))
        if fam == X3:                              # thick layer on the split-product kernel, same one-pass form
            name, chunks = 'conv_fwd_aff_tail_x3', L.ganlab_conv_fwd_aff_tail_x3_chunks(g.ref())
        elif thin:                                 # thin layer: the rolling-window kernel
            name, chunks = 'mod_conv_fwd_f32', L.ganlab_mod_conv_stat_chunks(g.ref())
        else:                                      # thicker layers: the tile kernels' TAIL epilogue
            name, chunks = 'conv_fwd_aff_tail_f32', L.ganlab_conv_fwd_aff_tail_chunks(g.ref())
        ws = torch.empty((n * cout * chunks * 2,), dtype=torch.float64, device=a_in.device)
        check(getattr(L, 'ganlab_' + name)(_p(a_in), _p(_packed_for(fam, w, g, scale)), _p(s_in), _p(t_in), _p(bias), _p(noise),
                                           _p(noise_w), _p(y), _p(mean), _p(rstd), g.ref(), bias_scale, act, slope, eps, _p(ws),
                                           ws.numel() * 8, _st()), name)
        style_c = _c(style) if style is not None else None
        s_, t_ = _affine_from_stats(mean, rstd, style_c, n, cout)
        ctx.save_for_backward(a_in, s_in, t_in, w, y, mean, rstd, style_c, noise)
        ctx.g, ctx.scale = g, scale
        ctx.bias_scale, ctx.act, ctx.slope, ctx.blur = bias_scale, act, slope, False
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.nw_shape = noise_w.shape if noise_w is not None else None
        ctx.bias_ref, ctx.nw_ref = bias, noise_w
        ctx.style_shape = style.shape if style is not None else None
        ctx.want_x_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[3]
        ctx.want_bias_grad, ctx.want_nw_grad = ctx.needs_input_grad[4], ctx.needs_input_grad[6]
        ctx.want_style_grad = ctx.needs_input_grad[7]
        ctx.mark_non_differentiable(s_, t_, mean, rstd)
        return y, s_, t_, mean, rstd

    @staticmethod
    @once_differentiable
    def backward(ctx, g_b, *_):
        a_in, s_in, t_in, w = ctx.saved_tensors[:4]
        gz, gb, gnw, gstyle = _layer_tail_backward(ctx, ctx.saved_tensors[4:], g_b)
        g = ctx.g
        ga = gw = None
        if ctx.needs_input_grad[0]:
            ga = k_conv_dgrad(gz, w, g, ctx.scale)              # d/d(a_in*s + t): shared weights, plain kernel
        if ctx.needs_input_grad[3] and _want_param_grads():
            _sink('gw', w)
            gw = k_conv_wgrad_aff(gz, a_in, s_in, t_in, g, ctx.scale)
            if _sunk('gw'):
                gw = None
        return ga, None, None, gw, gb, None, gnw, gstyle, None, None, None, None, None, None


class _UpConvBlurTail(Function):
    """A generator layer that opens a resolution,  Upsample -> conv3x3 -> blur -> +noise -> +bias -> LeakyReLU  with the
    InstanceNorm statistics of the result (stylegan/architectures.py:292-334, 497-526), in ONE pass over the activations
    (csrc/conv_s2_roll_blur.hip) - from a plain input or a deferred one (``s_in`` / ``t_in``: affine on load) to a deferred
    output (see ``Deferred``).  Backward: the layer tail's (InstanceNorm backward + LeakyReLU' + blur^T in one pass), then
    the up-conv's input gradient on the shared weights and its weight gradient with the same on-the-fly input."""

    @staticmethod
    def forward(ctx, a_in, s_in, t_in, w, bias, noise, noise_w, style, g, scale, bias_scale, act, slope, eps):
        noise = _c(noise) if noise is not None else None
        y, mean, rstd = k_conv_s2_fwd_blur_tail(a_in, s_in, t_in, w, bias, noise, noise_w, g, scale, bias_scale, act, slope,
                                                eps)
        style_c = _c(style) if style is not None else None
        s_, t_ = _affine_from_stats(mean, rstd, style_c, g.N, g.Cout)
        ctx.save_for_backward(a_in, s_in, t_in, w, y, mean, rstd, style_c, noise)
        ctx.g, ctx.scale = g, scale
        ctx.bias_scale, ctx.act, ctx.slope = bias_scale, act, slope
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.nw_shape = noise_w.shape if noise_w is not None else None
        ctx.style_shape = style.shape if style is not None else None
        ctx.bias_ref, ctx.nw_ref = bias, noise_w
        ctx.want_x_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[3]
        ctx.want_bias_grad, ctx.want_nw_grad = ctx.needs_input_grad[4], ctx.needs_input_grad[6]
        ctx.want_style_grad = ctx.needs_input_grad[7]
        ctx.mark_non_differentiable(s_, t_, mean, rstd)
        return y, s_, t_, mean, rstd

    @staticmethod
    @once_differentiable
    def backward(ctx, g_b, *_):
        a_in, s_in, t_in, w = ctx.saved_tensors[:4]
        gz, gb, gnw, gstyle = _layer_tail_backward(ctx, ctx.saved_tensors[4:], g_b, blur=True)   # d / d (conv output)
        g = ctx.g
        ga = gw = None
        if ctx.needs_input_grad[0]:
            ga = k_conv_dgrad(gz, w, g, ctx.scale)              # d/d(a_in*s + t) resp. d/d a_in: shared weights, plain kernel
        if ctx.needs_input_grad[3] and _want_param_grads():
            _sink('gw', w)
            gw = k_conv_wgrad_aff(gz, a_in, s_in, t_in, g, ctx.scale) if s_in is not None else \
                k_conv_wgrad(gz, a_in, g, ctx.scale)
            if _sunk('gw'):
                gw = None
        return ga, None, None, gw, gb, None, gnw, gstyle, None, None, None, None, None, None


def upconv_blur_tail_ok(shape, weight, deferred, padding=1):
    """Can the layer  Upsample -> conv3x3(weight) -> blur -> tail  on an input of ``shape`` run as the one-pass kernel (and,
    for a deferred input, its weight gradient with the affine on load)?"""
    if padding != 1 or tuple(weight.shape[2:]) != (3, 3) or int(weight.shape[1]) != int(shape[1]):
        return False
    n, cin, h, w = (int(v) for v in shape)
    try:
        g = Geom(n, cin, h, w, int(weight.shape[0]), 3, 1, 1, 0)
    except ValueError:
        return False
    if not conv_s2_blur_ok(g) or not _lib.lib().ganlab_blur_fused_supported(2 * h, 2 * w):
        return False
    return conv_aff_ok(shape, weight, True, padding) if deferred else True


def upconv_blur_tail(x, weight, scale, bias=None, noise=None, noise_w=None, style=None, bias_scale=1.0, act=None, slope=0.2,
                     eps=1e-8):
    """``x``: a tensor or a ``Deferred``; returns the layer's output as a ``Deferred`` (see ``upconv_blur_tail_ok``)."""
    a_in, s_in, t_in = (x.a, x.s, x.t) if isinstance(x, Deferred) else (x, None, None)
    if isinstance(x, Deferred):
        x.read()
    n, cin, h, w = a_in.shape
    g = Geom(n, cin, h, w, weight.shape[0], 3, 1, 1, 0)
    a = ACT_LRELU if act == 'lrelu' else ACT_NONE
    y, s_, t_, mean, rstd = _UpConvBlurTail.apply(a_in, s_in, t_in, weight, bias, noise, noise_w, style, g, float(scale),
                                                  float(bias_scale), a, float(slope), float(eps))
    return Deferred(y, s_, t_, mean, rstd, style)


class _ToRGBMod(Function):
    """toRGB (1x1, stylegan/architectures.py torgb) of a deferred tensor: per-sample weights w*s and bias b + w.t, built
    and folded back by two small kernels (csrc/mod.hip)."""

    @staticmethod
    def forward(ctx, a, s_, t_, w, bias, scale, bias_scale, link=None):
        a, w = _c(a), _c(w)
        n, cin, h, wd = a.shape
        cout = w.shape[0]
        L = _lib.lib()
        ctx.link = link
        weff, beff = _new((n, cin, 4), a), _new((n, 4), a)
        check(L.ganlab_mod_torgb_prep_f32(_p(w), _p(bias), _p(s_), _p(t_), _p(weff), _p(beff), n, cin, cout, scale,
                                          bias_scale, _st()), 'mod_torgb_prep')
        y = _new((n, cout, h, wd), a)
        check(L.ganlab_mod_torgb_fwd_f32(_p(a), _p(weff), _p(beff), _p(y), n, cin, cout, h * wd, _st()), 'mod_torgb_fwd')
        ctx.save_for_backward(a, s_, t_, w)
        ctx.scale, ctx.bias_scale = scale, bias_scale
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.bias_ref = bias
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        a, s_, t_, w = ctx.saved_tensors
        gy = _c(gy)
        n, cin, h, wd = a.shape
        cout = w.shape[0]
        L = _lib.lib()
        g = Geom(n, cin, h, wd, cout, 1, 0, 0)
        ga = None
        if ctx.link is not None:                         # a link left armed by a backward whose tail never ran is disarmed here
            ctx.link.grgb = ctx.link.wp = None
        if ctx.needs_input_grad[0]:                      # d/d(a*s + t)
            link = ctx.link
            if _rgb_link_ok(link, n, cin, cout, h * wd):
                # the producer's InstanceNorm backward recomputes it from gy (RgbGradLink); the engine only needs the shape
                link.grgb, link.wp, link.crgb = gy, _packed(w, PACK_DGRAD, ctx.scale), cout
                ga = torch.zeros((1,), dtype=a.dtype, device=a.device).expand(a.shape)      # (a 4-byte memset: never garbage)
            else:
                ga = k_conv_dgrad(gy, w, g, ctx.scale)
        gw = gb = None
        want_w = ctx.needs_input_grad[3]
        want_b = ctx.bias_shape is not None and ctx.needs_input_grad[4]
        if (want_w or want_b) and _want_param_grads():
            out = _new((n, 68), a)
            ws = torch.empty((L.ganlab_mod_torgb_cross_workspace(n) + 3) // 4, dtype=torch.float32, device=a.device)
            check(L.ganlab_mod_torgb_cross_f32(_p(a), _p(gy), _p(out), n, cin, cout, h * wd, _p(ws), ws.numel() * 4,
                                               _st()), 'mod_torgb_cross')
            _sink('gw', w if want_w else None)
            _sink('gb', ctx.bias_ref if want_b else None)
            gw = _take('gw', (cout, cin, 1, 1), a) if want_w else None
            gb = _take('gb', tuple(ctx.bias_shape), a) if want_b else None
            check(L.ganlab_mod_torgb_wgrad_f32(_p(out), _p(s_), _p(t_), _p(gw), _p(gb), n, cin, cout, ctx.scale,
                                               ctx.bias_scale, _st()), 'mod_torgb_wgrad')
            if _sunk('gw'):
                gw = None
            if _sunk('gb'):
                gb = None
        return ga, None, None, gw, gb, None, None, None


# ---------------------------------------------------------------------------------------------- #
# functional API
# ---------------------------------------------------------------------------------------------- #
ACT_DEFERRED = '_ganlab_act_deferred'    # attribute on a conv2d(defer_act_grad=True) result that really deferred


def conv2d(x, weight, bias=None, scale=1.0, padding=0, up=False, bias_scale=1.0, act=None, slope=0.2, pool=False,
           blur=False, defer_act_grad=False, in_act_slope=None, in_blur_handoff=None, in_rgb_handoff=None):
    """blur?(act(avgpool2?(scale*conv2d(up2?(x), weight, padding)) + bias*bias_scale)) on the matrix cores.
    ``pool``: the D down layer conv -> AvgPool2d(2) -> +bias -> LeakyReLU (progan/architectures.py:261-284)
    as one stride-2 kernel when the shape qualifies, else composed from the plain kernels.
    ``blur``: the binomial blur that follows conv+bias+LeakyReLU in a D block; its backward is fused with
    the LeakyReLU / bias backward.
    ``defer_act_grad`` / ``in_act_slope``: a pair of layers A -> B where B is a conv and the ONLY reader of A's
    LeakyReLU output (D block k's pooled conv -> block k+1's first conv).  A(defer_act_grad=True) may leave the
    multiplication by lrelu'(y_A) to B; when it does its result carries the attribute ``ACT_DEFERRED`` and the caller
    MUST run B with in_act_slope=<A's slope> - B's dgrad epilogue (or an explicit pass) then applies it."""
    n, cin, h, w = x.shape
    cout, cin_w, ks, _ = weight.shape
    if in_act_slope is not None:
        in_act_slope = float(in_act_slope)
        fold = not up and not pool and ks == 3 and (bias is not None or act == 'lrelu') and \
            conv_dgrad_mask_ok(Geom(n, cin, h, w, cout, ks, padding, 0, 0))
        if not fold:
            x, in_act_slope = _DeferredActGrad.apply(x, in_act_slope), None
    if blur:
        y = None
        if not pool and not up and ks in (1, 3) and act == 'lrelu':
            g = Geom(n, cin, h, w, cout, ks, padding, 0, 0)
            if _lib.lib().ganlab_blur_fused_supported(g.Ho, g.Wo):
                h = BlurHandoff()
                y = _ConvBiasAct.apply(x, weight, bias, g, float(scale), float(bias_scale), ACT_LRELU, float(slope),
                                       True, False, in_act_slope, h, None, None, in_rgb_handoff)
                if h.bits is not None:      # its only reader may take over this layer's blur^T / LeakyReLU' (fused_sequential)
                    setattr(y, BLUR_HANDOFF, h)
        return y if y is not None else _Blur.apply(conv2d(x, weight, bias, scale, padding, up, bias_scale, act, slope,
                                                          pool, in_act_slope=in_act_slope))
    if pool and not (not up and pool_fusable(n, cin, h, w, cout, ks, padding)):
        y = avg_pool2(conv2d(x, weight, None, scale, padding, up))
        return bias_act(y, bias, bias_scale=bias_scale, act=act, slope=slope)
    if ks == 4 and padding == 0 and h == 4 and w == 4 and not up:
        # 4x4 valid conv on a 4x4 map == linear over (ci, ky, kx)  (progan/architectures.py:227-229)
        y = linear(x.reshape(n, cin * 16), weight.reshape(cout, cin * 16), bias, scale, bias_scale, act, slope)
        return y.view(n, cout, 1, 1)
    g = Geom(n, cin, h, w, cout, ks, padding, up, pool)
    a = ACT_LRELU if act == 'lrelu' else ACT_NONE
    if bias is None and a == ACT_NONE:
        assert in_act_slope is None
        return _ConvFwd.apply(x, weight, g, float(scale))
    defer = bool(defer_act_grad) and a == ACT_LRELU and not conv_act_bwd_fusable(g)
    hin = None
    if in_blur_handoff is not None and pool and in_act_slope is None and in_blur_handoff.bits is not None and \
            conv_s2_blur_ok(g):
        hin = in_blur_handoff
    rgb = RgbHandoff() if (ks == 1 and a == ACT_LRELU and not up and not pool and cin <= 3) else None
    y = _ConvBiasAct.apply(x, weight, bias, g, float(scale), float(bias_scale), a, float(slope), False, defer,
                           in_act_slope, None, hin, rgb, in_rgb_handoff if (ks == 3 and not up and not pool) else None)
    if rgb is not None and rgb.bits is not None:
        setattr(y, RGB_HANDOFF, rgb)
    if defer:
        setattr(y, ACT_DEFERRED, True)
    return y


def linear(x, weight, bias=None, scale=1.0, bias_scale=1.0, act=None, slope=0.2):
    """act(scale * x @ weight.T + bias*bias_scale): a 1x1 conv over B 'pixels' of a 1x1 image."""
    n, cin = x.shape
    cout = weight.shape[0]
    y = conv2d(x.view(n, cin, 1, 1), weight.view(cout, cin, 1, 1), bias, scale, 0, False, bias_scale, act, slope)
    return y.view(n, cout)


STATS_MIN_PLANE = 1024   # planes below 32x32: the separate one-block-per-plane statistics kernel costs nothing


def bias_act(x, bias=None, noise=None, noise_w=None, bias_scale=1.0, act=None, slope=0.2, blur=False, stats_eps=None):
    """act(blur?(x) + noise_w*noise + bias*bias_scale); ``blur``: the binomial blur in front (one fused pass).
    ``stats_eps``: also return the InstanceNorm statistics of the result, ``(y, (mean, rstd))`` - or ``(y, None)``
    where the plane is too small / ragged for the fused accumulation - to hand to ``instnorm_style(stats=...)``."""
    a = ACT_LRELU if act == 'lrelu' else ACT_NONE
    eps = None
    if stats_eps is not None and x.dim() == 4:
        hw = x.shape[2] * x.shape[3]
        if hw >= STATS_MIN_PLANE and hw % 4 == 0:
            eps = float(stats_eps)
    if blur:
        if blur_fusable(x):
            out = _BlurBiasAct.apply(x, bias, noise, noise_w, float(bias_scale), a, float(slope), eps)
            return _with_stats(out, stats_eps, eps)
        x = _Blur.apply(x)
    return _with_stats(_BiasAct.apply(x, bias, noise, noise_w, float(bias_scale), a, float(slope), eps), stats_eps, eps)


def _with_stats(out, asked, fused):
    if asked is None:
        return out
    return (out[0], (out[1], out[2])) if fused is not None else (out, None)


# stays here, not with the rest of BatchNorm in _ops/norm.py: its eval path reads ``bias_act``, which tools/flip_probe.py rebinds
def batch_norm(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, batches=None,
               act_slope=None):
    """nn.BatchNorm2d semantics (biased variance for the normalisation, unbiased for the running estimate): fused
    kernels in training mode (``batches``: the module's ``num_batches_tracked``, counted by the same launch that moves the
    running estimates), one per-channel affine with the running statistics in eval mode."""
    if training:
        return _BatchNormTrain.apply(x, weight, bias, float(eps), running_mean, running_var, float(momentum), batches,
                                     act_slope)[0]
    xc = chan_affine(x, None, -running_mean)          # centred, like the training path
    rstd = torch.rsqrt(running_var + eps)
    y = chan_affine(xc, rstd * weight if weight is not None else rstd, bias)
    return y if act_slope is None else bias_act(y, act='lrelu', slope=act_slope)


def layer_tail(x, bias=None, noise=None, noise_w=None, style=None, bias_scale=1.0, act=None, slope=0.2, blur=False,
               eps=1e-8):
    """InstanceNorm+style of act(blur?(x) + noise_w*noise + bias*bias_scale): the generator layer after its conv.
    Large planes take the fused forward / backward passes (_LayerTail); small or ragged ones compose the two ops."""
    a = ACT_LRELU if act == 'lrelu' else ACT_NONE
    if x.dim() == 4 and noise is not None and noise.dim() == 4 and noise.shape[0] != x.shape[0]:
        noise = noise.expand(x.shape[0], *noise.shape[1:])
    hw = x.shape[2] * x.shape[3] if x.dim() == 4 else 0
    if hw >= STATS_MIN_PLANE and hw % 4 == 0 and (not blur or blur_fusable(x)):
        return _LayerTail.apply(x, bias, noise, noise_w, style, float(bias_scale), a, float(slope), bool(blur),
                                float(eps))
    y = bias_act(x, bias, noise, noise_w, bias_scale, act, slope, blur)
    return instnorm_style(y, style, eps)


def instnorm_style(x, style=None, eps=1e-8, stats=None):
    """``stats``: (mean, rstd) of ``x`` for this ``eps`` from ``bias_act(..., stats_eps=eps)`` (saves the pass)."""
    if stats is None:
        return _InstNormStyle.apply(x, style, float(eps))
    return _InstNormStyle.apply(x, style, float(eps), stats[0], stats[1])


def style_mod(x, style):
    """AdaIN's affine WITHOUT the normalisation (``use_instancenorm=False``, stylegan/architectures.py:497-526 with the
    norm list empty): ``x * (ys + 1) + yb`` with ``style`` = (N, 2C) = [ys | yb].  A per-(sample, channel) affine is the
    per-channel affine kernel on the (1, N*C, H, W) view; its backward is made of differentiable ops, so R1-style
    double backward is closed."""
    n, c = int(x.shape[0]), int(x.shape[1])
    st = style.reshape(n, 2, c)
    ys1 = (st[:, 0] + 1.0).reshape(-1).contiguous()
    yb = st[:, 1].reshape(-1).contiguous()
    return chan_affine(x.reshape(1, n * c, *x.shape[2:]), ys1, yb).reshape(x.shape)


def layer_tail_deferred(x, bias=None, noise=None, noise_w=None, style=None, bias_scale=1.0, act=None, slope=0.2,
                        blur=False, eps=1e-8):
    """ops.layer_tail without the normalisation pass: returns a ``Deferred`` (see there) for a modulated consumer."""
    a = ACT_LRELU if act == 'lrelu' else ACT_NONE
    link = RgbGradLink() if not blur else None
    y, s_, t_, mean, rstd = _LayerTailDeferred.apply(x, bias, noise, noise_w, style, float(bias_scale), a, float(slope),
                                                     bool(blur), float(eps), link)
    return Deferred(y, s_, t_, mean, rstd, style, link)


def conv_mod_tail(d, weight, scale, bias=None, noise=None, noise_w=None, style=None, bias_scale=1.0, act=None, slope=0.2,
                  eps=1e-8):
    """3x3 layer + its tail on a deferred input, deferred output (``_ConvModTail``)."""
    a = ACT_LRELU if act == 'lrelu' else ACT_NONE
    d.read()
    link = RgbGradLink()
    y, s_, t_, mean, rstd = _ConvModTail.apply(d.a, d.s, d.t, weight, bias, noise, noise_w, style, float(scale),
                                               float(bias_scale), a, float(slope), float(eps), link)
    return Deferred(y, s_, t_, mean, rstd, style, link)


def torgb_mod(d, weight, bias, scale, bias_scale=1.0):
    d.read()
    return _ToRGBMod.apply(d.a, d.s, d.t, weight, bias, float(scale), float(bias_scale), d.link)


def torgb_mod_ok(d, weight):
    if not isinstance(d, Deferred):
        return False
    n, c, h, w = d.a.shape
    return tuple(weight.shape[1:]) == (c, 1, 1) and weight.shape[0] <= 4 and c <= 16 and (h * w) % 4 == 0


