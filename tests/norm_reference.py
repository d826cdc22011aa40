"""Plain-torch restatement of the normalisation ops (gan_lab_amd/ops.py: batch_norm, layer_norm; csrc/norm.hip and the row
statistics of csrc/pointwise.hip).  Dtype-generic: in float64 it is the reference of tests/test_gpu_norm.py, in float32 on the
CPU its yardstick.  ``rowsum_plan`` / ``row_stats_chunks`` restate the two split formulas of the launch code, so that the
tests can prove which branch a shape reaches.

A fused activation is LeakyReLU(act_slope) (0 = ReLU) written as z * d with d = 1 where ``mask`` else act_slope; ``mask``
defaults to the reference's own z > 0.  The GPU tests pass the kernel's sign pattern instead (y_gpu > 0), so a pre-activation
that rounds to the other side of zero does not turn into a gradient error of O(1)."""
import torch

EPS = 1e-5


def _leaf(t, dtype):
    return t.detach().to(dtype).cpu().clone().requires_grad_(True) if t is not None else None


def _const(t, dtype):
    return t.detach().to(dtype).cpu() if t is not None else None


def _act(z, act_slope, mask):
    if act_slope is None:
        return z
    mask = (z.detach() > 0) if mask is None else mask.cpu()
    d = torch.where(mask, torch.ones((), dtype=z.dtype), torch.full((), float(act_slope), dtype=z.dtype))
    return z * d


def _bn_normalise(x, mean, var, weight, bias, eps):
    v = [1, -1, 1, 1]
    z = (x - mean.view(v)) * torch.rsqrt(var.view(v) + eps)
    if weight is not None:
        z = z * weight.view(v)
    if bias is not None:
        z = z + bias.view(v)
    return z


def batch_norm_with_grads(x, weight, bias, gy, dtype, act_slope=None, mask=None, eps=EPS):
    """Training-mode BatchNorm2d (+ fused activation) in ``dtype`` on the CPU for the cotangent ``gy`` of the output:
    (z, y, gx, gw, gb, batch mean, biased batch variance); z is the pre-activation, gw / gb are None without the parameter."""
    x, weight, bias = _leaf(x, dtype), _leaf(weight, dtype), _leaf(bias, dtype)
    mean = x.mean(dim=(0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    z = _bn_normalise(x, mean, var, weight, bias, eps)
    y = _act(z, act_slope, mask)
    leaves = [t for t in (x, weight, bias) if t is not None]
    grads = list(torch.autograd.grad(y, leaves, _const(gy, dtype)))
    gx = grads.pop(0)
    gw = grads.pop(0) if weight is not None else None
    gb = grads.pop(0) if bias is not None else None
    return z.detach(), y.detach(), gx, gw, gb, mean.detach(), var.detach()


def batch_norm_eval(x, weight, bias, running_mean, running_var, eps, dtype, act_slope=None, mask=None):
    """Eval-mode BatchNorm2d: the running statistics are constants.  Differentiable in x / weight / bias when those are
    leaves of ``dtype`` already (they are converted, not detached)."""
    x, weight, bias, running_mean, running_var = (t.to(dtype).cpu() if t is not None else None
                                                  for t in (x, weight, bias, running_mean, running_var))
    return _act(_bn_normalise(x, running_mean, running_var, weight, bias, eps), act_slope, mask)


def running_update(xs, momentum, dtype, running_mean=None, running_var=None):
    """nn.BatchNorm2d's running estimates after one training step per element of ``xs`` (start: zeros / ones): each moves by
    ``momentum`` towards the batch mean / the UNBIASED batch variance.  Returns (running_mean, running_var, batches)."""
    c = xs[0].shape[1]
    rm = torch.zeros(c, dtype=dtype) if running_mean is None else running_mean.to(dtype).cpu().clone()
    rv = torch.ones(c, dtype=dtype) if running_var is None else running_var.to(dtype).cpu().clone()
    for x in xs:
        x = x.detach().to(dtype).cpu()
        m = x.numel() // c
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean.view(1, -1, 1, 1)) ** 2).sum(dim=(0, 2, 3)) / max(m - 1, 1)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var
    return rm, rv, len(xs)


def layer_norm_with_grads(x, weight, bias, cot, w2, dtype, act_slope=None, mask=None, eps=EPS):
    """LayerNorm over the row of x (N, M) (+ fused activation), first and second order, in ``dtype`` on the CPU:
        out = sum y * cot,  gx = d out / dx (create_graph),  pen = sum (gx * w2)^2 + out
    Returns (z, y, gx, d pen/dx[, d pen/dw][, d pen/db]) - the gradient of an absent parameter is left out."""
    x, weight, bias = _leaf(x, dtype), _leaf(weight, dtype), _leaf(bias, dtype)
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    z = (x - mean) * torch.rsqrt(var + eps)
    if weight is not None:
        z = z * weight
    if bias is not None:
        z = z + bias
    y = _act(z, act_slope, mask)
    out = (y * _const(cot, dtype)).sum()
    gx, = torch.autograd.grad(out, x, create_graph=True)
    pen = ((gx * _const(w2, dtype)) ** 2).sum() + out
    leaves = [t for t in (x, weight, bias) if t is not None]
    grads = torch.autograd.grad(pen, leaves)
    return (z.detach(), y.detach(), gx.detach()) + tuple(grads)


# ---- the launch code's split formulas ---------------------------------------------------------------------------------------
ROWSUM_MAX_SPLIT = 64
EW_MAX_ITEMS = 2048 * 256          # one grid-stride pass of the element-wise kernels: 2048 blocks of 256 threads


def rowsum_plan(L):
    """(S, len) of ``rowsums_launch`` (csrc/norm.hip) for a row of L elements: S slices of ``len`` elements, the last one
    possibly shorter."""
    s = min(ROWSUM_MAX_SPLIT, max(1, -(-L // 4096)))
    length = -(-(-(-L // s)) // 256) * 256
    return -(-L // length), length


def row_stats_chunks(M):
    """Chunks per row of ``ganlab_row_stats_f32`` (csrc/pointwise.hip); fewer than two, or M % 4 != 0, means the
    one-block-per-row kernel (see ``row_stats_regime``)."""
    return min(64, max(1, -(-(M // 4) // 2048)))


def row_stats_regime(M):
    """'chunked', or the one-block-per-row fallback 'block256' (M >= 1024) / 'wave64' (M < 1024)."""
    if M % 4 == 0 and row_stats_chunks(M) >= 2:
        return 'chunked'
    return 'block256' if M >= 1024 else 'wave64'


def second_pass(items):
    """True when an element-wise kernel over ``items`` work items runs its grid-stride loop more than once."""
    return items > EW_MAX_ITEMS


# ---- the cases of tests/test_gpu_norm.py (asserted branch by branch in tests/test_norm_host.py) ---------------------------
SLOPES = (None, 0.0, 0.2)
# BatchNorm (N, C, H, W) -> the row-sum plan (S, len) over L = N*H*W it is there for
BN_SHAPES = {
    (5, 6, 9, 11): (1, 512),            # odd HW: scalar apply
    (8, 3, 32, 32): (2, 4096),          # two full slices of four whole segments each
    (3, 4, 36, 40): (2, 2304),          # ragged last slice, slice boundaries inside segments
    (4, 8, 264, 260): (64, 4352),       # the cap of 64 slices, len > 4096, float4 apply with a second grid-stride pass
    (3, 2, 295, 297): (61, 4352),       # odd HW beyond one grid-stride pass: scalar apply and ln_project twice round
    (1, 4, 4, 4): (1, 256),             # one sample
}
# (shape, parameters present: 'wb' / 'w' / 'b' / '', input mean, input std)
BN_CASES = [(s, 'wb', 0.5, 2.0) for s in BN_SHAPES] + \
    [(s, p, 0.5, 2.0) for s in ((8, 3, 32, 32), (3, 4, 36, 40)) for p in ('b', 'w', '')] + \
    [((8, 3, 32, 32), 'wb', 200.0, 1.0)]
# LayerNorm (N, M) -> (statistics regime, chunks, row-sum plan (S, len))
LN_SHAPES = {
    (3, 7): ('wave64', 1, (1, 256)),
    (5, 1028): ('block256', 1, (1, 1280)),
    (4, 1020): ('wave64', 1, (1, 1024)),
    (3, 4101): ('block256', 1, (2, 2304)),          # M % 4 != 0; ragged second row-sum slice
    (2, 8192): ('block256', 1, (2, 4096)),          # the largest row of one statistics chunk; two full row-sum slices
    (2, 8196): ('chunked', 2, (3, 2816)),           # the smallest row of two statistics chunks
    (2, 269120): ('chunked', 33, (62, 4352)),       # row sums at the cap; every element-wise kernel twice round
    (1, 528392): ('chunked', 64, (63, 8448)),       # the statistics' cap of 64 chunks; a single row
}
LN_CASES = [(s, 'wb', 0.2, 1.5) for s in LN_SHAPES] + \
    [(s, p, 0.2, 1.5) for s in ((3, 4101), (2, 8192)) for p in ('', 'w')] + \
    [((2, 8192), 'wb', 300.0, 1.0)]


def case_id(case):
    shape, params, mean, _ = case
    return 'x'.join(map(str, shape)) + '-' + (params or 'none') + ('-mean%g' % mean if mean > 1 else '')


def _seed(shape, mean):
    return (sum((i + 1) * d for i, d in enumerate(shape)) * 7 + int(mean)) % (2 ** 31)


def bn_inputs(shape, params, mean, std):
    """(x, weight, bias, gy) in float32 on the CPU; weight / bias None when absent from ``params``."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, mean))
    x = torch.randn(n, c, h, w, generator=g) * std + mean
    weight, bias = torch.randn(c, generator=g) * 0.3 + 1.0, torch.randn(c, generator=g) * 0.3
    gy = torch.randn(n, c, h, w, generator=g)
    return x, (weight if 'w' in params else None), (bias if 'b' in params else None), gy


def ln_inputs(shape, params, mean, std):
    """(x, weight, bias, cot, w2) in float32 on the CPU."""
    n, m = shape
    g = torch.Generator().manual_seed(_seed(shape, mean))
    x = torch.randn(n, m, generator=g) * std + mean
    weight, bias = torch.randn(m, generator=g) * 0.3 + 1.0, torch.randn(m, generator=g) * 0.3
    cot, w2 = torch.randn(n, m, generator=g), torch.randn(n, m, generator=g)
    return x, (weight if 'w' in params else None), (bias if 'b' in params else None), cot, w2
