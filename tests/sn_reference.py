"""Float64 restatement of spectral normalisation with one power iteration (the arithmetic of
``torch.nn.utils.spectral_norm``), for the tests of gan_lab_amd/spectral_norm.py and csrc/spectral.hip.

For a parameter ``W`` viewed as ``Wm = W.reshape(Cout, -1)`` with stored unit vectors ``u``, ``v`` and ``eps = 1e-12``:

    iterate:   t = Wm^T u ; v <- t / max(|t|, eps) ; s = Wm v ; u <- s / max(|s|, eps)
    always:    sigma = u^T Wm v ;  W_sn = W / sigma
    backward:  gW = (g_sn - <g_sn, W_sn> u v^T) / sigma          (u, v constants)
"""
import torch

EPS = 1e-12


def _f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def refresh(W, u, v=None, iterate=True, eps=EPS):
    """-> (u, v, sigma, W_sn) in float64; ``v`` may be None when ``iterate`` (it is recomputed from u first)."""
    W, u = _f64(W), _f64(u)
    Wm = W.reshape(W.shape[0], -1)
    if iterate:
        t = Wm.t() @ u
        v = t / max(t.norm().item(), eps)
        s = Wm @ v
        u = s / max(s.norm().item(), eps)
    else:
        v = _f64(v)
    sigma = torch.dot(u, Wm @ v)
    return u, v, sigma, W / sigma


def backward(g_sn, W, u, v, sigma):
    """Gradient towards W of a loss whose gradient towards W_sn = W / sigma(W) is ``g_sn`` (u, v constants)."""
    g, W, u, v = _f64(g_sn), _f64(W), _f64(u), _f64(v)
    sigma = float(sigma)
    W_sn = W / sigma
    return (g - (g * W_sn).sum() * torch.outer(u, v).reshape(W.shape)) / sigma


def hinge_disc(d_fake, d_real):
    return torch.relu(1 - d_real).mean() + torch.relu(1 + d_fake).mean()


def hinge_gen(d_fake):
    return -d_fake.mean()
