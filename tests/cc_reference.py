"""Plain-torch restatement of the classifier-based conditioning losses (gan_lab_amd/ops.py: class_cross_entropy,
class_contrastive; csrc/cond_loss.hip) and of their analytic gradients as explicit functions.
Dtype-generic: in float64 it is the reference of tests/test_gpu_cond_loss.py, in float32 on the CPU its yardstick.

    h (N, E) embeddings, proxy (K, E), labels (N,);  hh, ph = rows divided by max(norm, 1e-12)
    s_i = hh_i . ph_{y_i},  S_ij = hh_i . hh_j,  t = temperature
    ce    l_i = LSE_k z_ik - z_{i,y_i}
    2c    u_i = s_i/t, A_ij = S_ij/t (j != i);  D_i = LSE({u_i} u {A_ij}), M_i = LSE({u_i} u {A_ij: y_j = y_i});  l_i = D_i - M_i
    d2d   u_i = min(s_i - m_p, 0)/t, A_ij = max(S_ij - m_n, 0)/t over y_j != y_i;  D_i = LSE({u_i} u {A_ij});  l_i = D_i - u_i
Every loss is the mean of l_i.
"""
import torch

EPS = 1e-12
MODES = ('2c', 'd2d')


def _to(dtype, *ts):
    return tuple(t if dtype is None else t.to(dtype) for t in ts)


def normalize(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)


def similarities(h, proxy, labels, dtype=None):
    """(s (N,), S (N, N)) of the normalised rows."""
    h, proxy = _to(dtype, h, proxy)
    hh, ph = normalize(h), normalize(proxy)
    return (hh * ph[labels.long()]).sum(1), hh @ hh.t()


def cross_entropy_rows(z, labels, dtype=None):
    z, = _to(dtype, z)
    return torch.logsumexp(z, dim=1) - z.gather(1, labels.long()[:, None])[:, 0]


def cross_entropy(z, labels, dtype=None):
    return cross_entropy_rows(z, labels, dtype).mean()


def cross_entropy_grad(z, labels, g=1.0, dtype=None):
    """dz_ik = g/N (softmax_ik - [k = y_i])."""
    z, = _to(dtype, z)
    p = torch.softmax(z, dim=1)
    p[torch.arange(z.shape[0], device=z.device), labels.long()] -= 1.0
    return p * (g / z.shape[0])


def _terms(h, proxy, labels, mode, temperature, margin_pos, margin_neg):
    """(u (N,), A (N, N) with -inf where the pair does not count, same (N, N) bool, s, S, hh, ph)."""
    if mode not in MODES:
        raise ValueError(f'mode must be one of {MODES} (got {mode!r})')
    y = labels.long()
    hh, ph = normalize(h), normalize(proxy)
    s, S = (hh * ph[y]).sum(1), hh @ hh.t()
    same = y[:, None] == y[None, :]
    eye = torch.eye(h.shape[0], dtype=torch.bool, device=h.device)
    ninf = torch.full_like(S, float('-inf'))
    if mode == '2c':
        u, A = s / temperature, torch.where(eye, ninf, S / temperature)
    else:
        u = (s - margin_pos).clamp(max=0.0) / temperature
        A = torch.where(same, ninf, (S - margin_neg).clamp(min=0.0) / temperature)
    return u, A, same & ~eye, s, S, hh, ph


def contrastive_rows(h, proxy, labels, mode='2c', temperature=1.0, margin_pos=0.98, margin_neg=0.02, dtype=None):
    h, proxy = _to(dtype, h, proxy)
    u, A, same, *_ = _terms(h, proxy, labels, mode, temperature, margin_pos, margin_neg)
    D = torch.logsumexp(torch.cat((u[:, None], A), dim=1), dim=1)
    if mode == 'd2d':
        return D - u
    M = torch.logsumexp(torch.cat((u[:, None], torch.where(same, A, torch.full_like(A, float('-inf')))), dim=1), dim=1)
    return D - M


def contrastive(h, proxy, labels, mode='2c', temperature=1.0, margin_pos=0.98, margin_neg=0.02, dtype=None):
    return contrastive_rows(h, proxy, labels, mode, temperature, margin_pos, margin_neg, dtype).mean()


def contrastive_grads(h, proxy, labels, mode='2c', temperature=1.0, margin_pos=0.98, margin_neg=0.02, g=1.0, dtype=None):
    """(dh, dproxy) of ``g * contrastive(...)`` from the closed forms: a_ij = dl_i/dS_ij, b_i = dl_i/ds_i, then
    dhh_i = sum_j (a_ij + a_ji) hh_j + b_i ph_{y_i}, dph_k = sum_{i: y_i = k} b_i hh_i, each through the derivative of the
    normalisation, (d - x (x . d)) / max(norm, 1e-12).  The derivative of a clamp is 0 at its kink."""
    h, proxy = _to(dtype, h, proxy)
    y = labels.long()
    t = temperature
    u, A, same, s, S, hh, ph = _terms(h, proxy, labels, mode, t, margin_pos, margin_neg)
    D = torch.logsumexp(torch.cat((u[:, None], A), dim=1), dim=1)
    if mode == '2c':
        M = torch.logsumexp(torch.cat((u[:, None], torch.where(same, A, torch.full_like(A, float('-inf')))), dim=1), dim=1)
        a = (torch.exp(A - D[:, None]) - torch.where(same, torch.exp(A - M[:, None]), torch.zeros_like(A))) / t
        b = (torch.exp(u - D) - torch.exp(u - M)) / t
    else:
        a = torch.where(S > margin_neg, torch.exp(A - D[:, None]), torch.zeros_like(A)) / t      # exp(-inf) = 0 off the set
        b = torch.where(s < margin_pos, torch.exp(u - D) - 1.0, torch.zeros_like(u)) / t
    dhh = (a + a.t()) @ hh + b[:, None] * ph[y]
    dph = torch.zeros_like(proxy).index_add_(0, y, b[:, None] * hh)
    scale = g / h.shape[0]

    def through_norm(d, xh, x):
        return (d - xh * (xh * d).sum(1, keepdim=True)) / x.norm(dim=1, keepdim=True).clamp_min(EPS)

    return through_norm(dhh, hh, h) * scale, through_norm(dph, ph, proxy) * scale


def cross_entropy_with_grads(z, labels, g, dtype):
    """(loss, rows, dz) in ``dtype`` on the CPU, the gradient by autograd."""
    z = z.detach().to(dtype).cpu().clone().requires_grad_(True)
    rows = cross_entropy_rows(z, labels.cpu())
    loss = rows.mean()
    dz, = torch.autograd.grad(loss * g, z)
    return loss.detach(), rows.detach(), dz


def contrastive_with_grads(h, proxy, labels, g, dtype, **kw):
    """(loss, rows, dh, dproxy) in ``dtype`` on the CPU, the gradients by autograd."""
    h, proxy = (t.detach().to(dtype).cpu().clone().requires_grad_(True) for t in (h, proxy))
    rows = contrastive_rows(h, proxy, labels.cpu(), **kw)
    loss = rows.mean()
    dh, dp = torch.autograd.grad(loss * g, (h, proxy))
    return loss.detach(), rows.detach(), dh, dp
