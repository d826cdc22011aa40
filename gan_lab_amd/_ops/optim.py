"""Whole-network parameter passes: spectral normalisation, orthogonal regularisation, Adam, RMSprop / SGD / optimistic Adam, the
step-scalar block, the lagged (EWMA) generator.

Drives csrc/spectral.hip, csrc/ortho.hip, csrc/sample.hip (``ewma_many``), csrc/optim.hip and the optimiser entry points of
csrc/pointwise.hip;
composed in gan_lab_amd/spectral_norm.py, ortho_reg.py, optim.py, sampling.py and graphs.py.  Re-exported by ``gan_lab_amd.ops``."""
import ctypes

import torch

from .. import _lib
from .._lib import check
from .core import _c, _inplace, _p, _same_numel, _st


# ---- spectral normalisation: every weight of a critic per launch (csrc/spectral.hip) -----------------------------------
SN_EPS = 1e-12      # torch.nn.utils.spectral_norm's eps


class SnTable(object):
    """Device-resident job table of ``ganlab_sn_refresh`` / ``ganlab_sn_backward``.  ``layers``: one dict per weight with
    the float32 GPU tensors ``w`` (the parameter, viewed as (shape[0], -1)), ``w_sn``, ``g_sn``, ``gw`` (same numel), ``u``
    (shape[0]), ``v`` (numel / shape[0]) and ``sigma`` (1); every one contiguous and 16-byte aligned.  Built and uploaded once
    (outside any capture), together with the scratch the passes use; keeps the tensors it points at alive."""

    def __init__(self, layers):
        if not layers:
            raise ValueError('SnTable: no layers')
        RC, TC, EB = _lib.SN_ROW_CHUNK, _lib.SN_COL_TILE, _lib.SN_ELEM_BLOCK
        self.layers = [dict(d) for d in layers]
        dev = self.layers[0]['w'].device
        geo, need = [], 0
        for d in self.layers:
            w = d['w']
            R = int(w.shape[0])
            K = w.numel() // R
            want = {'w': R * K, 'w_sn': R * K, 'g_sn': R * K, 'gw': R * K, 'u': R, 'v': K, 'sigma': 1}
            for name, n in want.items():
                t = d[name]
                _c(t, f'SnTable {name}')
                if not t.is_contiguous() or t.numel() != n or t.data_ptr() % 16 or t.device != dev:
                    raise ValueError(f'SnTable: {name} must be contiguous, 16-byte aligned, on {dev}, with {n} elements '
                                     f'(got {tuple(t.shape)} at {t.data_ptr():#x} on {t.device})')
            nrc, nct, neb = (R + RC - 1) // RC, (K + TC - 1) // TC, (R * K + EB - 1) // EB
            offs = []
            for n in (nrc * K, R, neb):
                offs.append(need)
                need += (n + 3) // 4 * 4
            geo.append((R, K, nrc * nct, (R + 3) // 4, neb, offs))
        self.scratch = torch.zeros(need, dtype=torch.float32, device=dev)
        arr = (_lib.SnJob * len(self.layers))()
        bt = bs = be = 0
        base = self.scratch.data_ptr()
        for j, d, (R, K, nt, ns, ne, offs) in zip(arr, self.layers, geo):
            j.w, j.w_sn, j.g_sn, j.gw = d['w'].data_ptr(), d['w_sn'].data_ptr(), d['g_sn'].data_ptr(), d['gw'].data_ptr()
            j.u, j.v, j.sigma = d['u'].data_ptr(), d['v'].data_ptr(), d['sigma'].data_ptr()
            j.tpart, j.s, j.dpart = base + 4 * offs[0], base + 4 * offs[1], base + 4 * offs[2]
            j.R, j.K, j.blk_t0, j.blk_s0, j.blk_e0 = R, K, bt, bs, be
            bt, bs, be = bt + nt, bs + ns, be + ne
        self.blocks = (bt, bs, be)
        self.n = len(self.layers)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def sn_refresh(table, iterate):
    """One power iteration (``iterate``) of every layer of ``table``, then sigma = u^T W v and W_sn = W / sigma: 4 launches,
    2 without the iteration.  The caller reports the rewritten W_sn range (``bump_weight_epoch``)."""
    bt, bs, be = table.blocks
    check(_lib.lib().ganlab_sn_refresh(table.table.data_ptr(), table.n, bt, bs, be, 1 if iterate else 0, SN_EPS, _st()),
          'sn_refresh')


def sn_backward(table):
    """gW += (g_sn - <g_sn, W_sn> u v^T) / sigma for every layer of ``table`` (2 launches)."""
    check(_lib.lib().ganlab_sn_backward(table.table.data_ptr(), table.n, table.blocks[2], _st()), 'sn_backward')


# ---- orthogonal regularisation: every weight of a network per launch (csrc/ortho.hip) ----------------------------------
def ortho_plan(shapes):
    """Host-side layout of the job table of ``ganlab_ortho_apply`` for weights of the given (R, K) shapes.  -> (entries,
    scratch floats, (Gram blocks, apply blocks)); ``entries[i]`` is None for a layer with R == 1 (no off-diagonal element: its
    penalty and gradient are exactly 0, it is left out) and else a dict with ``form`` (row form when R <= K, else column form:
    the m x m Gram matrix has m = min(R, K)), ``m``, the float offsets ``s``, ``q`` (None in row form) and ``part`` into the
    scratch, ``n_part`` and the first block ``blk_g0`` / ``blk_a0`` of either pass.  Pure arithmetic: no GPU, no library."""
    T, QR = _lib.ORTHO_TILE, _lib.ORTHO_QROWS
    entries, need, bg, ba = [], 0, 0, 0

    def take(n):
        nonlocal need
        o = need
        need += (n + 3) // 4 * 4
        return o

    for R, K in shapes:
        R, K = int(R), int(K)
        if R < 1 or K < 1:
            raise ValueError(f'ortho_plan: bad weight shape ({R}, {K})')
        if R == 1:
            entries.append(None)
            continue
        row = R <= K
        m = R if row else K
        tm = (m + T - 1) // T
        n_part = tm * tm + (0 if row else (R + QR - 1) // QR)
        e = dict(R=R, K=K, form=_lib.ORTHO_ROW if row else _lib.ORTHO_COL, m=m, s=take(m * m), q=None if row else take(R),
                 part=take(n_part), n_part=n_part, blk_g0=bg, blk_a0=ba)
        bg += n_part
        ba += ((R + T - 1) // T) * ((K + T - 1) // T)
        entries.append(e)
    return entries, need, (bg, ba)


class OrthoTable(object):
    """Device-resident job table of ``ganlab_ortho_apply``.  ``layers``: one dict per weight with the float32 GPU tensors ``w``
    (the parameter, viewed as (shape[0], -1)) and ``gw`` (its gradient slot, same numel), both contiguous and 16-byte aligned.
    Built and uploaded once (outside any capture), together with the scratch (the m x m Gram matrices, q, the partial sums) and
    the results: ``penalties`` holds one float per layer (0 for a skipped one) and then the total.  Keeps the tensors it points
    at alive."""

    def __init__(self, layers):
        if not layers:
            raise ValueError('OrthoTable: no layers')
        self.layers = [dict(d) for d in layers]
        dev = self.layers[0]['w'].device
        shapes = []
        for d in self.layers:
            w = d['w']
            R = int(w.shape[0])
            K = w.numel() // R
            for name in ('w', 'gw'):
                t = d[name]
                _c(t, f'OrthoTable {name}')
                if not t.is_contiguous() or t.numel() != R * K or t.data_ptr() % 16 or t.device != dev:
                    raise ValueError(f'OrthoTable: {name} must be contiguous, 16-byte aligned, on {dev}, with {R * K} elements '
                                     f'(got {tuple(t.shape)} at {t.data_ptr():#x} on {t.device})')
            shapes.append((R, K))
        self.plan, need, self.blocks = ortho_plan(shapes)
        self.scratch = torch.zeros(max(need, 4), dtype=torch.float32, device=dev)
        self.penalties = torch.zeros(len(self.layers) + 1, dtype=torch.float32, device=dev)
        live = [(i, d, e) for i, (d, e) in enumerate(zip(self.layers, self.plan)) if e is not None]
        self.n = len(live)
        arr = (_lib.OrthoJob * max(self.n, 1))()
        base, pen = self.scratch.data_ptr(), self.penalties.data_ptr()
        for j, (i, d, e) in zip(arr, live):
            j.w, j.gw = d['w'].data_ptr(), d['gw'].data_ptr()
            j.s, j.part, j.penalty = base + 4 * e['s'], base + 4 * e['part'], pen + 4 * i
            j.q = base + 4 * e['q'] if e['q'] is not None else None
            j.R, j.K, j.form, j.n_part, j.blk_g0, j.blk_a0 = e['R'], e['K'], e['form'], e['n_part'], e['blk_g0'], e['blk_a0']
        self.total = self.penalties[len(self.layers):]      # 1 element: beta * sum over all layers
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def ortho_apply(table, beta):
    """gw += 4 beta ((Wm Wm^T) o (1 - I)) Wm for every layer of ``table``, and ``table.penalties`` = beta * sum(M^2) per layer
    and in total: 3 launches whatever the number of layers (none when every layer was skipped)."""
    beta = float(beta)
    if not (0.0 <= beta < float('inf')):
        raise ValueError(f'ortho_apply: beta must be a finite number >= 0 (got {beta!r})')
    if table.n == 0:
        return
    bg, ba = table.blocks
    check(_lib.lib().ganlab_ortho_apply(table.table.data_ptr(), table.n, bg, ba, beta, _p(table.total), _st()), 'ortho_apply')


def lerp_rows(a, b, t):
    a, b, t = _c(a), _c(b), _c(t)
    out = torch.empty_like(a)
    n = a.shape[0]
    check(_lib.lib().ganlab_lerp_rows_f32(_p(a), _p(b), _p(t), _p(out), n, a.numel() // n, _st()), 'lerp_rows')
    return out


def _adam_operands(op, p, g, m, v):
    named = [('p', p), ('g', g), ('m', m), ('v', v)]
    for what, t in named:
        _inplace(t, f'{op} {what}')
    _same_numel(op, named)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2):
    _adam_operands('adam_step', p, g, m, v)
    check(_lib.lib().ganlab_adam_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, bc1, bc2,
                                     _st()), 'adam')


def adam_step_dev(p, g, m, v, scalars, beta1, beta2, eps, wd):
    """``adam_step`` with (lr, 1 - beta1^t, 1 - beta2^t) read from the three floats at ``scalars`` (a device pointer)."""
    _adam_operands('adam_step_dev', p, g, m, v)
    if isinstance(scalars, bool) or not isinstance(scalars, int) or scalars <= 0:
        raise TypeError(f'gan_lab_amd.ops: adam_step_dev scalars must be a device address inside the step-scalar block (got '
                        f'{scalars!r})')
    check(_lib.lib().ganlab_adam_dev_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), ctypes.c_void_p(scalars), beta1, beta2, eps,
                                         wd, _st()), 'adam_dev')


# ---- RMSprop, SGD with momentum, optimistic Adam (csrc/optim.hip) ---------------------------------------------------------------
def _optim_operands(op, named):
    """The checks ``_adam_operands`` makes, over ``named`` = [(what, tensor)]; a ``None`` tensor (a null ``buf``) is left out."""
    named = [(what, t) for what, t in named if t is not None]
    for what, t in named:
        _inplace(t, f'{op} {what}')
    _same_numel(op, named)


def _dev_scalars(op, scalars):
    if isinstance(scalars, bool) or not isinstance(scalars, int) or scalars <= 0:
        raise TypeError(f'gan_lab_amd.ops: {op} scalars must be a device address inside the step-scalar block (got {scalars!r})')
    return ctypes.c_void_p(scalars)


def _momentum_buf(op, momentum, buf):
    momentum = float(momentum)
    if not (0.0 <= momentum < float('inf')):
        raise ValueError(f'gan_lab_amd.ops: {op} momentum must be a finite number >= 0 (got {momentum!r})')
    if momentum > 0.0 and buf is None:
        raise TypeError(f'gan_lab_amd.ops: {op} with momentum > 0 needs its momentum buffer (got None)')
    return momentum, (buf if momentum > 0.0 else None)


def rmsprop_step(p, g, sq, buf, lr, alpha, eps, wd, momentum):
    """One ``torch.optim.RMSprop(centered=False)`` step over flat float32 GPU tensors; ``buf`` is None with ``momentum`` = 0."""
    momentum, buf = _momentum_buf('rmsprop_step', momentum, buf)
    _optim_operands('rmsprop_step', [('p', p), ('g', g), ('sq', sq), ('buf', buf)])
    check(_lib.lib().ganlab_rmsprop_f32(_p(p), _p(g), _p(sq), _p(buf), p.numel(), lr, alpha, eps, wd, momentum, _st()),
          'rmsprop')


def rmsprop_step_dev(p, g, sq, buf, scalars, alpha, eps, wd, momentum):
    """``rmsprop_step`` with lr read from the first of the three floats at ``scalars`` (a device pointer)."""
    momentum, buf = _momentum_buf('rmsprop_step_dev', momentum, buf)
    _optim_operands('rmsprop_step_dev', [('p', p), ('g', g), ('sq', sq), ('buf', buf)])
    check(_lib.lib().ganlab_rmsprop_dev_f32(_p(p), _p(g), _p(sq), _p(buf), p.numel(), _dev_scalars('rmsprop_step_dev', scalars),
                                            alpha, eps, wd, momentum, _st()), 'rmsprop_dev')


def sgd_step(p, g, buf, lr, wd, momentum, first):
    """One ``torch.optim.SGD(dampening=0, nesterov=False)`` step; ``first``: the momentum buffer is set to g' instead of updated
    (torch's first step).  ``buf`` is None with ``momentum`` = 0."""
    momentum, buf = _momentum_buf('sgd_step', momentum, buf)
    _optim_operands('sgd_step', [('p', p), ('g', g), ('buf', buf)])
    check(_lib.lib().ganlab_sgd_f32(_p(p), _p(g), _p(buf), p.numel(), lr, wd, momentum, 1 if first else 0, _st()), 'sgd')


def sgd_step_dev(p, g, buf, scalars, wd, momentum):
    """``sgd_step`` with (lr, first) read from the first two of the three floats at ``scalars``; first = 1.0 on step 1, else 0.0."""
    momentum, buf = _momentum_buf('sgd_step_dev', momentum, buf)
    _optim_operands('sgd_step_dev', [('p', p), ('g', g), ('buf', buf)])
    check(_lib.lib().ganlab_sgd_dev_f32(_p(p), _p(g), _p(buf), p.numel(), _dev_scalars('sgd_step_dev', scalars), wd, momentum,
                                        _st()), 'sgd_dev')


def oadam_step(p, g, m, v, prev, lr, beta1, beta2, eps, wd, bc1, bc2):
    """One optimistic Adam step (Daskalakis et al. 2018): p -= 2 lr d - lr prev, prev = d, d Adam's bias-corrected direction."""
    _optim_operands('oadam_step', [('p', p), ('g', g), ('m', m), ('v', v), ('prev', prev)])
    check(_lib.lib().ganlab_oadam_f32(_p(p), _p(g), _p(m), _p(v), _p(prev), p.numel(), lr, beta1, beta2, eps, wd, bc1, bc2,
                                      _st()), 'oadam')


def oadam_step_dev(p, g, m, v, prev, scalars, beta1, beta2, eps, wd):
    """``oadam_step`` with (lr, 1 - beta1^t, 1 - beta2^t) read from the three floats at ``scalars`` (a device pointer)."""
    _optim_operands('oadam_step_dev', [('p', p), ('g', g), ('m', m), ('v', v), ('prev', prev)])
    check(_lib.lib().ganlab_oadam_dev_f32(_p(p), _p(g), _p(m), _p(v), _p(prev), p.numel(), _dev_scalars('oadam_step_dev', scalars),
                                          beta1, beta2, eps, wd, _st()), 'oadam_dev')


def set_step_scalars(block, rng_base, floats):
    f = [float(v) for v in floats] + [0.0] * (6 - len(floats))
    check(_lib.lib().ganlab_set_step_scalars(ctypes.c_void_p(block.data_ptr()), int(rng_base) & (2 ** 64 - 1), *f[:6],
                                             _st()), 'set_step_scalars')


def ewma_step(lagged, p, beta):
    named = [('lagged', lagged), ('p', p)]
    for what, t in named:
        _inplace(t, f'ewma_step {what}')
    _same_numel('ewma_step', named)
    check(_lib.lib().ganlab_ewma_f32(_p(lagged), _p(p), p.numel(), beta, _st()), 'ewma')


class EwmaTable(object):
    """Device-resident job table of ``ganlab_ewma_many_f32``.  ``pairs``: [(lagged, src)], contiguous float32 GPU tensors of equal
    size on one device, no two of them overlapping.  Built and uploaded once (outside any capture); keeps the tensors it points
    at alive."""

    def __init__(self, pairs):
        self.pairs = [(a, b) for a, b in pairs]
        if not self.pairs:
            raise ValueError('EwmaTable: no segments')
        if len(self.pairs) > 65535:
            raise ValueError(f'EwmaTable: at most 65535 segments (got {len(self.pairs)})')
        dev = self.pairs[0][0].device
        arr = (_lib.EwmaJob * len(self.pairs))()
        for j, (lagged, src) in zip(arr, self.pairs):
            for t, what in ((lagged, 'EwmaTable lagged'), (src, 'EwmaTable src')):
                _c(t, what)
                if not t.is_contiguous() or t.device != dev:
                    raise ValueError(f'{what} must be contiguous and on {dev} (got {tuple(t.shape)} on {t.device})')
            if lagged.numel() != src.numel() or lagged.numel() < 1 or lagged.data_ptr() == src.data_ptr():
                raise ValueError(f'EwmaTable: a segment needs two distinct tensors of one size >= 1 (got {tuple(lagged.shape)}, '
                                 f'{tuple(src.shape)})')
            j.dst, j.src, j.count = lagged.data_ptr(), src.data_ptr(), lagged.numel()
        self.n = len(self.pairs)
        self.pointers = self._pointers()
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)

    def _pointers(self):
        return tuple(t.data_ptr() for pair in self.pairs for t in pair)

    def is_current(self):
        """Do the tensors still lie where the uploaded table points?"""
        return self.pointers == self._pointers()


def ewma_many(table, decay):
    """``lagged = decay * lagged + (1 - decay) * src`` for every segment of ``table`` in one launch; ``decay`` = 0 copies."""
    decay = float(decay)
    if not (0.0 <= decay < 1.0):
        raise ValueError(f'ewma_many: decay must lie in [0, 1) (got {decay!r})')
    if not table.is_current():
        raise RuntimeError('ewma_many: a tensor of the table moved since it was built; build a new EwmaTable')
    check(_lib.lib().ganlab_ewma_many_f32(table.table.data_ptr(), table.n, decay, _st()), 'ewma_many')
