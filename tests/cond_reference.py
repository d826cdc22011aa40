"""Plain-torch restatement of the class-conditioning ops (gan_lab_amd/ops.py: cond_batch_norm, class_projection).
Dtype-generic: in float64 it is the reference of tests/test_gpu_cond.py, in float32 on the CPU its yardstick."""
import torch
import torch.nn.functional as F


def cond_batch_norm(x, weight, bias, labels, eps=1e-5, dtype=None):
    """Training-mode BatchNorm without affine, then row ``labels[n]`` of the (K, C) tables as sample n's scale and shift."""
    if dtype is not None:
        x, weight, bias = x.to(dtype), weight.to(dtype), bias.to(dtype)
    labels = labels.long()
    xhat = F.batch_norm(x, None, None, None, None, True, 0.0, eps)
    return xhat * weight[labels][:, :, None, None] + bias[labels][:, :, None, None]


def cond_batch_norm_eval(x, weight, bias, labels, running_mean, running_var, eps=1e-5, dtype=None):
    if dtype is not None:
        x, weight, bias, running_mean, running_var = (t.to(dtype) for t in (x, weight, bias, running_mean, running_var))
    labels = labels.long()
    xhat = F.batch_norm(x, running_mean, running_var, None, None, False, 0.0, eps)
    return xhat * weight[labels][:, :, None, None] + bias[labels][:, :, None, None]


def projection(f, W, labels, base=None, dtype=None):
    """out[n] = base[n] + <W[labels[n]], f[n]>."""
    if dtype is not None:
        f, W, base = f.to(dtype), W.to(dtype), (base.to(dtype) if base is not None else None)
    out = (W[labels.long()] * f).sum(1)
    return out if base is None else base + out


def proj_dfeat(g, W, labels, dtype=None):
    """G(g, W, l)[n, j] = g[n] W[l_n, j]."""
    if dtype is not None:
        g, W = g.to(dtype), W.to(dtype)
    return g[:, None] * W[labels.long()]


def proj_dweight(g, f, labels, num_classes, dtype=None):
    """S(g, f, l)[k, j] = sum_{n: l_n = k} g[n] f[n, j]."""
    if dtype is not None:
        g, f = g.to(dtype), f.to(dtype)
    return torch.zeros(num_classes, f.shape[1], dtype=f.dtype).index_add_(0, labels.long(), g[:, None] * f)


def cond_batch_norm_with_grads(x, weight, bias, labels, gy, dtype, eps=1e-5):
    """(y, gx, d weight, d bias) in ``dtype`` on the CPU for the cotangent ``gy`` of ``y``."""
    x, weight, bias = (t.detach().to(dtype).cpu().clone().requires_grad_(True) for t in (x, weight, bias))
    y = cond_batch_norm(x, weight, bias, labels.cpu(), eps)
    gx, gw, gb = torch.autograd.grad(y, (x, weight, bias), gy.detach().to(dtype).cpu())
    return y.detach(), gx, gw, gb


def projection_with_grads(f, W, labels, base, g, dtype):
    """(out, d f, d W, d base) in ``dtype`` on the CPU for the cotangent ``g`` of ``out``."""
    f, W, base = (t.detach().to(dtype).cpu().clone().requires_grad_(True) for t in (f, W, base))
    out = projection(f, W, labels.cpu(), base)
    gf, gw, gbase = torch.autograd.grad(out, (f, W, base), g.detach().to(dtype).cpu())
    return out.detach(), gf, gw, gbase


def second_order_scalars(proj, x, W, labels):
    """The second-order probes of the projection family with ``proj(f, W, labels)`` the op under test and f = x:
    p = P(x); g = d p.sum() / d x (create_graph, = G);
      dw     = d (g**2).sum() / d W                                          through G's backward (S)
      dx     = d [((g * x).sum(1) * p).sum() + (g**2).sum()] / d x          a mixed scalar: through P's backward with a cotangent
                                                                             that depends on x, and through G
      dx_s   = d (s**2).sum() / d x with s = d (p**2).sum() / d W (create_graph, = S + ...)      through S's backward"""
    p = proj(x, W, labels)
    g, = torch.autograd.grad(p.sum(), x, create_graph=True)
    dw, = torch.autograd.grad((g ** 2).sum(), W, retain_graph=True)
    dx, = torch.autograd.grad(((g * x).sum(1) * p).sum() + (g ** 2).sum(), x, retain_graph=True)
    s, = torch.autograd.grad((p ** 2).sum(), W, create_graph=True)
    dx_s, = torch.autograd.grad((s ** 2).sum(), x)
    return dw, dx, dx_s


def projection_second_order(x, W, labels, dtype):
    x, W = (t.detach().to(dtype).cpu().clone().requires_grad_(True) for t in (x, W))
    return second_order_scalars(projection, x, W, labels.cpu())
