"""Plain restatements of the fused arena optimisers beside Adam (csrc/optim.hip; gan_lab_amd/optim.py): RMSprop, SGD with momentum
and optimistic Adam, in float64 (the yardstick) and float32 (the CPU's evaluation of the same formulas, one rounding per
operation), with a forward error bound per step in the manner of ``pointwise_reference.adam_reference``.

Scalars are formed as Python floats and then rounded to float32 (``f32``), which is what a kernel receives for a scalar argument.

The bounds count fp32 roundings, u = 2^-24 each, on quantities of the float64 run; FMA contraction only removes roundings.  A
square root and a quotient are allowed one ulp = 2 u each: correctly rounded forms cost u, and the allowance covers a compiler
that picks an approximate form refined to one ulp."""
import math

import numpy as np

from pointwise_reference import EPS32, f32

U = EPS32


def _as(dtype, *xs):
    return tuple(np.asarray(x, dtype=dtype) for x in xs)


def _zero_err(p, names):
    return {k: np.zeros_like(np.asarray(p, dtype=np.float64)) for k in ('p',) + tuple(names)}


def _decayed(p, g, wd, err, dt):
    """g' = g + wd p and its bound: the product and the sum round once each, and p's own error enters through wd."""
    if wd == 0.0:
        return g, np.zeros(np.shape(g))
    gi = g + dt(wd) * p
    eg = 2 * U * (np.abs(g) + np.abs(wd * p)) + wd * err['p'] if err is not None else None
    return gi, eg


# ---- RMSprop ---------------------------------------------------------------------------------------------------------------------
def rmsprop_reference(p, g, sq, buf, lr, alpha, eps, wd, momentum, dtype=np.float64, variant=None, err=None):
    """One step of torch.optim.RMSprop(centered=False):
        g' = g + wd p;  sq' = alpha sq + (1 - alpha) g'^2;  d = g' / (sqrt(sq') + eps);
        momentum > 0: buf' = momentum buf + d, p' = p - lr buf';  else p' = p - lr d
    -> (p', sq', buf').  ``variant``: 'eps_inside' (d = g' / sqrt(sq' + eps)).  ``err``: dict(p, sq, buf) of running bounds on
    |fp32 evaluation - this|, advanced by one step:
        sq':  alpha e_sq + (1 - alpha) 2 |g'| e_g + 4 u (alpha sq + (1 - alpha) g'^2)       (1 - alpha, g'^2, the products, the sum)
        den = sqrt(sq') + eps:  e_sq / (2 sqrt(sq')) + 3 u den                              (root 2 u, sum u; vanishes with sq')
        d:    2 u |d| + e_g / den + |d| e_den / den                                          (the quotient)
        buf': momentum e_buf + e_d + 2 u (|momentum buf| + |d|)                              (product, sum)
        p':   e_p + lr e_x + u |lr x| + u |p'|,  x = buf' or d                               (product, difference)."""
    dt = np.dtype(dtype).type
    p, g, sq, buf = _as(dtype, p, g, sq, buf)
    gi, eg = _decayed(p, g, wd, err, dt)
    sqn = dt(alpha) * sq + (dt(1) - dt(alpha)) * gi * gi
    den = np.sqrt(sqn + dt(eps)) if variant == 'eps_inside' else np.sqrt(sqn) + dt(eps)
    d = gi / den
    if momentum > 0:
        bufn = dt(momentum) * buf + d
        x = bufn
    else:
        bufn = buf
        x = d
    pn = p - dt(lr) * x
    if err is not None:
        esq = alpha * err['sq'] + (1.0 - alpha) * 2 * np.abs(gi) * eg + 4 * U * (alpha * sq + (1.0 - alpha) * gi * gi)
        root = np.sqrt(sqn)
        eden = np.divide(esq, 2.0 * root, out=np.zeros_like(root), where=root > 0) + 3 * U * den
        ed = 2 * U * np.abs(d) + eg / den + np.abs(d) * eden / den
        if momentum > 0:
            ex = momentum * err['buf'] + ed + 2 * U * (np.abs(momentum * buf) + np.abs(d))
            err['buf'] = ex
        else:
            ex = ed
        err['p'], err['sq'] = err['p'] + lr * ex + U * np.abs(lr * x) + U * np.abs(pn), esq
    return pn, sqn, bufn


# ---- SGD -------------------------------------------------------------------------------------------------------------------------
def sgd_reference(p, g, buf, lr, wd, momentum, first, dtype=np.float64, variant=None, err=None):
    """One step of torch.optim.SGD(dampening=0, nesterov=False):
        g' = g + wd p;  momentum > 0: buf' = g' on the first step, else momentum buf + g';  p' = p - lr buf';  else p' = p - lr g'
    -> (p', buf').  ``variant``: 'dampening' (buf' = momentum buf + (1 - 0.1) g' after the first step), 'first_ignored' (the first
    step updates the buffer it finds instead of replacing it).  ``err``: dict(p, buf):
        buf': e_g on the first step, else momentum e_buf + e_g + 2 u (|momentum buf| + |g'|)
        p':   e_p + lr e_x + u |lr x| + u |p'|,  x = buf' or g'."""
    dt = np.dtype(dtype).type
    p, g, buf = _as(dtype, p, g, buf)
    gi, eg = _decayed(p, g, wd, err, dt)
    if momentum > 0:
        if first and variant != 'first_ignored':
            bufn = gi + dt(0)
        elif variant == 'dampening' and not first:
            bufn = dt(momentum) * buf + (dt(1) - dt(0.1)) * gi
        else:
            bufn = dt(momentum) * buf + gi
        x = bufn
    else:
        bufn, x = buf, gi
    pn = p - dt(lr) * x
    if err is not None:
        if momentum > 0:
            ex = eg if first else momentum * err['buf'] + eg + 2 * U * (np.abs(momentum * buf) + np.abs(gi))
            err['buf'] = ex
        else:
            ex = eg
        err['p'] = err['p'] + lr * ex + U * np.abs(lr * x) + U * np.abs(pn)
    return pn, bufn


# ---- optimistic Adam -------------------------------------------------------------------------------------------------------------
def oadam_reference(p, g, m, v, prev, lr, b1, b2, eps, wd, bc1, bc2, dtype=np.float64, variant=None, err=None):
    """One step of optimistic Adam (Daskalakis et al. 2018, Algorithm 1) in the kernel's form:
        g' = g + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  d = (m' / bc1) / (sqrt(v') / sqrt(bc2) + eps);
        p' = p - (2 lr d - lr prev);  prev' = d
    -> (p', m', v', prev').  ``variant``: 'prev_first' (prev is overwritten by d before it is used: plain Adam).  ``err``:
    dict(p, m, v, prev); m' and v' as in ``pointwise_reference.adam_reference``;
        den = sqrt(v') rsqrt(bc2) + eps:  e_v / (2 v') (den - eps) + 6 u den       (root 2 u, rsqrt 2 u, product u, sum u)
        d:    4 u |d| + e_m / (bc1 den) + |d| e_den / den                          (two quotients)
        p':   e_p + 2 lr e_d + lr e_prev + 3 u |2 lr d| + 2 u |lr prev| + u |p'|   (2 lr, 2 lr d, lr prev, their difference; the
              last difference)."""
    dt = np.dtype(dtype).type
    p, g, m, v, prev = _as(dtype, p, g, m, v, prev)
    gi, eg = _decayed(p, g, wd, err, dt)
    mi = dt(b1) * m + (dt(1) - dt(b1)) * gi
    vi = dt(b2) * v + (dt(1) - dt(b2)) * gi * gi
    den = np.sqrt(vi) / dt(math.sqrt(bc2)) + dt(eps)
    d = (mi / dt(bc1)) / den
    used = d if variant == 'prev_first' else prev
    pn = p - (dt(2) * dt(lr) * d - dt(lr) * used)
    if err is not None:
        em = b1 * err['m'] + (1.0 - b1) * eg + 3 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * gi))
        ev = b2 * err['v'] + (1.0 - b2) * 2 * np.abs(gi) * eg + 4 * U * (b2 * v + (1.0 - b2) * gi * gi)
        rel_v = np.divide(ev, 2.0 * vi, out=np.zeros_like(vi), where=vi > 0)
        eden = rel_v * (den - eps) + 6 * U * den
        ed = 4 * U * np.abs(d) + em / (bc1 * den) + np.abs(d) * eden / den
        err['p'] = (err['p'] + 2 * lr * ed + lr * err['prev'] + 3 * U * np.abs(2 * lr * d) + 2 * U * np.abs(lr * prev) +
                    U * np.abs(pn))
        err['m'], err['v'], err['prev'] = em, ev, ed
    return pn, mi, vi, d


# ---- runs ------------------------------------------------------------------------------------------------------------------------
STATE = {'rmsprop': ('sq', 'buf'), 'sgd': ('buf',), 'oadam': ('m', 'v', 'prev')}


def run(kind, p, grads, dtype=np.float64, variant=None, state=None, **hp):
    """``len(grads)`` steps of optimiser ``kind`` ('rmsprop' | 'sgd' | 'oadam') from zero state (or ``state``: dict of initial
    buffers) -> (dict(p=, <state>...), err, local): ``err`` the bound carried through all steps, ``local`` the bound of the last
    step alone (from exact inputs): the per-step bound.  ``hp``: lr, wd, eps and alpha, momentum (rmsprop); momentum (sgd);
    b1, b2 (oadam) as Python floats; every scalar is rounded to float32 first, the bias corrections after they are formed."""
    names = STATE[kind]
    p = np.asarray(p, dtype=dtype)
    st = {k: np.zeros_like(p) for k in names}
    for k, v in (state or {}).items():
        st[k] = np.asarray(v, dtype=dtype)
    err = _zero_err(p, names)
    local = None
    h = {k: f32(v) for k, v in hp.items()}
    for t, g in enumerate(grads, 1):
        local = _zero_err(p, names)
        for e in (local, err):
            if kind == 'rmsprop':
                out = rmsprop_reference(p, g, st['sq'], st['buf'], h['lr'], h['alpha'], h['eps'], h['wd'], h['momentum'], dtype,
                                        variant, e)
            elif kind == 'sgd':
                out = sgd_reference(p, g, st['buf'], h['lr'], h['wd'], h['momentum'], t == 1, dtype, variant, e)
            else:
                bc1, bc2 = f32(1 - hp['b1'] ** t), f32(1 - hp['b2'] ** t)
                out = oadam_reference(p, g, st['m'], st['v'], st['prev'], h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], bc1, bc2,
                                      dtype, variant, e)
        p = out[0]
        st = dict(zip(names, out[1:]))
    return dict(st, p=p), err, local


def inputs(n, steps=8, seed=97):
    """Parameters and ``steps`` gradients (float32 values): normal draws; gradient elements 5 mod 7 are exact zeros and elements
    3 mod 11 lie near 1e-12 in EVERY step (there sq and v stay 0 or ~1e-27 and ``eps`` decides the step), and the parameters at
    3 mod 11 are scaled by 1e-3 so that a change of the step shows against a small ulp."""
    gen = np.random.default_rng(seed + n)
    p = gen.standard_normal(n).astype(np.float32)
    p[3::11] *= np.float32(1e-3)
    grads = []
    for _ in range(steps):
        g = gen.standard_normal(n).astype(np.float32)
        g[5::7] = 0.0
        g[3::11] = (1e-12 * (1.0 + gen.random(g[3::11].shape))).astype(np.float32)
        grads.append(g)
    return p, grads
