"""The arithmetic of a feature quantisation layer for the ResNet GAN critic (Zhao et al., ICML 2020, "Feature Quantization Improves
GAN Training": nearest-code assignment, straight-through output, commitment term, Laplace-smoothed EMA dictionary - the VQ-VAE-2
``Quantize`` layer) in plain torch, parameterised by dtype: float64 is the truth, float32 the CPU yardstick of a GPU test.  The
layer itself is not in the package yet; tests/test_fq_host.py checks this statement of it.

``h`` (N, C, H, W), channel-major; its rows are the M = N H W vectors ``h[n, :, y, x]``.  ``embed`` (K, C).

    idx[m]  = argmin_k (|e_k|^2 - 2 <h_m, e_k>)        the lowest k of a tie (torch.argmin's rule on the CPU is checked by a test)
    out     = h + (q - h),  q[m] = embed[idx[m]]
    commit  = mean over all elements of (q - h)^2
    dh      = dout + dcommit (2 / numel) (h - q)
    update  : n_k = #{m: idx[m] = k}, S_k = sum of those rows; cluster_size <- d cluster_size + (1 - d) n_k; embed_avg <- d embed_avg +
              (1 - d) S_k; n = sum_k cluster_size; embed_k <- embed_avg_k / ((cluster_size_k + eps) / (n + K eps) n), eps = 1e-5
    perplexity = exp(-sum_k p_k log p_k), p_k = n_k / M
"""
import torch

EPS = 1e-5


def rows(h):
    """(N, C, H, W) -> (M, C): row m = n H W + y W + x."""
    return h.permute(0, 2, 3, 1).reshape(-1, h.shape[1])


def unrows(r, shape):
    n, c, hh, ww = shape
    return r.reshape(n, hh, ww, c).permute(0, 3, 1, 2).contiguous()


def scores(h, embed, dtype=torch.float64):
    """(M, K): |e_k|^2 - 2 <h_m, e_k>."""
    r, e = rows(h).to(dtype), embed.to(dtype)
    return (e * e).sum(1)[None, :] - 2.0 * (r @ e.t())


def first_argmin(s):
    """argmin over the last axis, the lowest index of a tie (independent of torch.argmin's tie rule)."""
    k = s.shape[-1]
    cand = torch.where(s == s.min(-1, keepdim=True).values, torch.arange(k)[None, :], torch.full((1, 1), k))
    return cand.min(-1).values


def assign(h, embed, dtype=torch.float64):
    """idx (N, H, W) int32."""
    return first_argmin(scores(h, embed, dtype)).to(torch.int32).reshape(h.shape[0], h.shape[2], h.shape[3])


def forward(h, embed, idx, dtype=torch.float64):
    """(out, commit) for a given assignment."""
    hd = h.to(dtype)
    q = unrows(embed.to(dtype)[idx.reshape(-1).long()], h.shape)
    d = q - hd
    return hd + d, (d * d).mean()


def backward(h, embed, idx, dout, dcommit, dtype=torch.float64):
    """dh; ``dout`` None = zero, ``dcommit`` None = zero."""
    hd = h.to(dtype)
    q = unrows(embed.to(dtype)[idx.reshape(-1).long()], h.shape)
    dh = torch.zeros_like(hd) if dout is None else dout.to(dtype).clone()
    if dcommit is not None:
        dh = dh + float(dcommit) * (2.0 / h.numel()) * (hd - q)
    return dh


def stats(h, idx, k, dtype=torch.float64):
    """(n_k (K,), S_k (K, C))."""
    r, flat = rows(h).to(dtype), idx.reshape(-1).long()
    n_k = torch.bincount(flat, minlength=k).to(dtype)
    s_k = torch.zeros(k, r.shape[1], dtype=dtype).index_add_(0, flat, r)
    return n_k, s_k


def update(h, idx, embed_avg, cluster_size, decay, dtype=torch.float64):
    """-> (embed, embed_avg, cluster_size, perplexity) after one update."""
    k = cluster_size.shape[0]
    n_k, s_k = stats(h, idx, k, dtype)
    cs = decay * cluster_size.to(dtype) + (1.0 - decay) * n_k
    ea = decay * embed_avg.to(dtype) + (1.0 - decay) * s_k
    n = cs.sum()
    smoothed = (cs + EPS) / (n + k * EPS) * n
    p = n_k / n_k.sum()
    ent = -(p[p > 0] * p[p > 0].log()).sum()
    return ea / smoothed[:, None], ea, cs, ent.exp()


def run(h, embed, embed_avg, cluster_size, decay, dout, dcommit, dtype=torch.float64, idx=None):
    """Everything for one pass: dict(idx, out, commit, dh, embed, embed_avg, cluster_size, perplexity).  ``idx`` None: assigned in
    ``dtype``."""
    idx = assign(h, embed, dtype) if idx is None else idx
    out, commit = forward(h, embed, idx, dtype)
    e, ea, cs, ppl = update(h, idx, embed_avg, cluster_size, decay, dtype)
    return dict(idx=idx, out=out, commit=commit, dh=backward(h, embed, idx, dout, dcommit, dtype), embed=e, embed_avg=ea,
                cluster_size=cs, perplexity=ppl)


def gaps(h, embed):
    """Per row, in float64: (gap between the best and the second-best score, |h_m|^2 + |e_best|^2); one code: an infinite gap."""
    s = scores(h, embed)
    r, e = rows(h).double(), embed.double()
    best = first_argmin(s)
    scale = (r * r).sum(1) + (e * e).sum(1)[best]
    if s.shape[1] == 1:
        return torch.full_like(scale, float('inf')), scale
    two = s.topk(2, dim=1, largest=False).values
    return two[:, 1] - two[:, 0], scale


def optimality(h, embed, idx):
    """How far the chosen codes are from optimal, per row in float64: (score[chosen] - min score, |h_m|^2 + max(|e_chosen|^2,
    |e_best|^2))."""
    s = scores(h, embed)
    r, e = rows(h).double(), embed.double()
    en = (e * e).sum(1)
    best, chosen = first_argmin(s), idx.reshape(-1).long()
    excess = s.gather(1, chosen[:, None])[:, 0] - s.min(1).values
    return excess, (r * r).sum(1) + torch.maximum(en[chosen], en[best])
