"""Plain-torch restatement of the self-attention ops (gan_lab_amd/ops.py: attention, max_pool2x2; attention.py: the block).
Dtype-generic: in float64 it is the reference of tests/test_gpu_attn.py, in float32 on the CPU its yardstick."""
import torch
import torch.nn.functional as F


def attention(q, k, v):
    """q (N, Dk, L), k (N, Dk, S), v (N, Dv, S) -> o (N, Dv, L), lse (N, L); no 1/sqrt(d) scale."""
    s = torch.einsum('ndl,nds->nls', q, k)
    lse = torch.logsumexp(s, dim=2)
    p = torch.exp(s - lse.unsqueeze(2))
    return torch.einsum('ncs,nls->ncl', v, p), lse


def max_pool2x2(x):
    return F.max_pool2d(x, kernel_size=2, stride=2)


def block(x, w_theta, w_phi, w_g, w_o, gamma):
    """SelfAttention2d.forward with the four 1x1 weights (OIHW) and the scalar gate."""
    n, c, h, w = x.shape
    q = F.conv2d(x, w_theta).reshape(n, -1, h * w)
    k = max_pool2x2(F.conv2d(x, w_phi)).reshape(n, -1, h * w // 4)
    v = max_pool2x2(F.conv2d(x, w_g)).reshape(n, -1, h * w // 4)
    a, _ = attention(q, k, v)
    return x + gamma * F.conv2d(a.reshape(n, -1, h, w), w_o)


def attention_with_grads(q, k, v, d_o, dtype):
    """(o, lse, dq, dk, dv) in ``dtype`` on the CPU for the cotangent ``d_o`` of ``o``."""
    q, k, v = (t.detach().to(dtype).cpu().clone().requires_grad_(True) for t in (q, k, v))
    o, lse = attention(q, k, v)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o.detach().to(dtype).cpu())
    return o.detach(), lse.detach(), dq, dk, dv
