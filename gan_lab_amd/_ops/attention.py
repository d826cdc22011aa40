"""Self-attention, the 2x2 max pool and the gated residual of the attention block: first order only.

Drives csrc/attention.hip; composed in gan_lab_amd/attention.py.  ``k_dot`` writes the gate's gradient and takes its output
through ``core._take``.  Re-exported by ``gan_lab_amd.ops``."""
import torch
from torch.autograd import Function

from .. import _lib
from .._lib import check
from .core import _c, _new, _p, _sink, _st, _sunk, _take, _want_param_grads
from .pointwise import k_scale_dev


# ---------------------------------------------------------------------------------------------- #
# self-attention (csrc/attention.hip; attention.py): first-order only
# ---------------------------------------------------------------------------------------------- #
_ATTN_SECOND_ORDER = ('self_attention: double backward through {} is not implemented (use hinge + spectral norm with '
                      'gradient_penalty=None on a critic with attention)')


def _attn_dims(q, k, v):
    if not (q.dim() >= 3 and k.dim() >= 3 and v.dim() >= 3):
        raise ValueError('attention: q, k, v must be (N, D, L...) tensors')
    n, dk, dv = q.shape[0], q.shape[1], v.shape[1]
    l, s = q[0, 0].numel(), k[0, 0].numel()
    if k.shape[0] != n or v.shape[0] != n or k.shape[1] != dk or v[0, 0].numel() != s:
        raise ValueError(f'attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit')
    return n, dk, dv, l, s


def attention_ok(n, dk, dv, l, s):
    """Does the fused kernel take this geometry (``ganlab_attn_supported``)?"""
    return bool(_lib.lib().ganlab_attn_supported(int(n), int(dk), int(dv), int(l), int(s)))


def k_attn_fwd(q, k, v):
    q, k, v = _c(q, 'attention q'), _c(k, 'attention k'), _c(v, 'attention v')
    n, dk, dv, l, s = _attn_dims(q, k, v)
    o, lse = _new((n, dv) + tuple(q.shape[2:]), q), _new((n, l), q)
    check(_lib.lib().ganlab_attn_fwd_f32(_p(q), _p(k), _p(v), _p(o), _p(lse), n, dk, dv, l, s, _st()), 'attn_fwd')
    return o, lse


def k_attn_bwd(q, k, v, o, lse, go):
    go = _c(go)
    n, dk, dv, l, s = _attn_dims(q, k, v)
    L = _lib.lib()
    ws = _new(((L.ganlab_attn_bwd_workspace(n, l) + 3) // 4,), q)
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    check(L.ganlab_attn_bwd_f32(_p(q), _p(k), _p(v), _p(o), _p(lse), _p(go), _p(gq), _p(gk), _p(gv), n, dk, dv, l, s,
                                _p(ws), ws.numel() * 4, _st()), 'attn_bwd')
    return gq, gk, gv


class _Attention(Function):
    """o = softmax_s(q^T k) applied to v, channel-major operands; saves q, k, v, o and the (N, L) log-sum-exp - never the map."""

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _c(q, 'attention q'), _c(k, 'attention k'), _c(v, 'attention v')
        o, lse = k_attn_fwd(q, k, v)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        gq, gk, gv = _AttentionBwd.apply(go, q, k, v, o, lse)
        return gq, gk, gv


class _AttentionBwd(Function):
    @staticmethod
    def forward(ctx, go, q, k, v, o, lse):
        return k_attn_bwd(q, k, v, o, lse, go)

    @staticmethod
    def backward(ctx, *gg):
        raise NotImplementedError(_ATTN_SECOND_ORDER.format('attention'))


def _pool_dims(x):
    if x.dim() < 2 or x.shape[-1] % 2 or x.shape[-2] % 2:
        raise ValueError(f'max_pool2x2: H and W must be even (got {tuple(x.shape)})')
    h, w = x.shape[-2], x.shape[-1]
    return x.numel() // (h * w), h, w


def k_maxpool2x2(x):
    x = _c(x, 'max_pool2x2 input')
    planes, h, w = _pool_dims(x)
    L = _lib.lib()
    y = _new(tuple(x.shape[:-2]) + (h // 2, w // 2), x)
    bits = torch.empty(L.ganlab_maxpool2x2_bits_bytes(planes, h, w), dtype=torch.uint8, device=x.device)
    check(L.ganlab_maxpool2x2_f32(_p(x), _p(y), _p(bits), planes, h, w, _st()), 'maxpool2x2')
    return y, bits


def k_maxpool2x2_bwd(gy, bits, shape):
    gy = _c(gy)
    h, w = shape[-2], shape[-1]
    gx = _new(tuple(shape), gy)
    check(_lib.lib().ganlab_maxpool2x2_bwd_f32(_p(gy), _p(bits), _p(gx), gx.numel() // (h * w), h, w, _st()),
          'maxpool2x2_bwd')
    return gx


class _MaxPool2x2(Function):
    @staticmethod
    def forward(ctx, x):
        y, bits = k_maxpool2x2(x)
        ctx.bits, ctx.shape = bits, tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        return _MaxPool2x2Bwd.apply(gy, ctx.bits, ctx.shape)


class _MaxPool2x2Bwd(Function):
    @staticmethod
    def forward(ctx, gy, bits, shape):
        return k_maxpool2x2_bwd(gy, bits, shape)

    @staticmethod
    def backward(ctx, gg):
        raise NotImplementedError(_ATTN_SECOND_ORDER.format('max_pool2x2'))


def k_gated_residual(x, y, gamma):
    x, y, gamma = _c(x), _c(y), _c(gamma, 'gated_residual gamma')
    assert x.shape == y.shape and gamma.numel() == 1
    out = torch.empty_like(x)
    check(_lib.lib().ganlab_gated_residual_f32(_p(x), _p(y), _p(gamma), _p(out), x.numel(), _st()), 'gated_residual')
    return out


def k_dot(a, b, sink=None):
    a, b = _c(a), _c(b)
    assert a.shape == b.shape
    L = _lib.lib()
    ws = _new(((L.ganlab_dot_workspace(a.numel()) + 3) // 4,), a)
    out = _take(sink, (1,), a) if sink is not None else _new((1,), a)
    check(L.ganlab_dot_f32(_p(a), _p(b), _p(out), a.numel(), _p(ws), ws.numel() * 4, _st()), 'dot')
    return out


class _GatedResidual(Function):
    """out = x + gamma * y with ``gamma`` a one-element device tensor (the attention block's learned gate)."""

    @staticmethod
    def forward(ctx, x, y, gamma):
        ctx.save_for_backward(y, gamma)
        ctx.gamma_ref = gamma
        return k_gated_residual(x, y, gamma)

    @staticmethod
    def backward(ctx, g):
        y, gamma = ctx.saved_tensors
        want_y = ctx.needs_input_grad[1]
        want_g = ctx.needs_input_grad[2] and _want_param_grads()
        _sink('ggamma', ctx.gamma_ref if want_g else None)
        gy, gg = _GatedResidualBwd.apply(g, y, gamma, bool(want_y), bool(want_g))
        if _sunk('ggamma'):
            want_g = False
        return (g if ctx.needs_input_grad[0] else None), (gy if want_y else None), \
            (gg.view(gamma.shape) if want_g else None)


class _GatedResidualBwd(Function):
    """(dy, dgamma) = (gamma * g, <g, y>): the dot in fp64 partials added in a fixed order."""

    @staticmethod
    def forward(ctx, g, y, gamma, want_y, want_g):
        g = _c(g)
        gy = k_scale_dev(g, gamma, 1.0) if want_y else None
        gg = k_dot(g, y, sink='ggamma') if want_g else None
        return gy, gg

    @staticmethod
    def backward(ctx, *gg):
        raise NotImplementedError(_ATTN_SECOND_ORDER.format('the gated residual'))


def attention(q, k, v):
    """SAGAN attention core on channel-major operands q (N, Dk, L...), k (N, Dk, S...), v (N, Dv, S...) -> (N, Dv, L...):
    ``softmax_s(sum_d q[n,d,l] k[n,d,s])`` applied to ``v``, no ``1/sqrt(d)`` scale.  One fused kernel forward, three backward;
    the (L, S) map is never stored.  Differentiable once."""
    return _Attention.apply(q, k, v)


def max_pool2x2(x):
    """2x2 / stride-2 max pool over the last two dimensions (even sizes); ties go to the first of the four, as in ATen.
    Differentiable once."""
    return _MaxPool2x2.apply(x)


def gated_residual(x, y, gamma):
    """``x + gamma * y`` with a one-element device tensor ``gamma``.  Differentiable once."""
    return _GatedResidual.apply(x, y, gamma)
