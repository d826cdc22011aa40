"""Float64 torch-CPU restatement of BigGAN's orthogonal regulariser (Brock et al. 2019, eq. 3), the yardstick of
tests/test_ortho_host.py and tests/test_gpu_ortho.py.  ``penalty`` is written literally from the formula and ``gradient`` is
its autograd derivative; ``closed_form``, ``row_form`` and ``column_form`` restate what the kernels compute."""
import torch


def _wm(W):
    W = W.detach().double()
    return W.reshape(W.shape[0], -1)


def penalty(W, beta):
    """beta * || (Wm Wm^T) o (1 - I) ||_F^2 with Wm = W.reshape(Cout, -1); differentiable in W (float64)."""
    Wm = W.reshape(W.shape[0], -1)
    eye = torch.eye(Wm.shape[0], dtype=Wm.dtype)
    return beta * (((Wm @ Wm.t()) * (1 - eye)) ** 2).sum()


def gradient(W, beta):
    """(penalty, d penalty / d W) by autograd of ``penalty``, float64, in the shape of W."""
    leaf = W.detach().double().clone().requires_grad_(True)
    p = penalty(leaf, beta)
    g, = torch.autograd.grad(p, leaf)
    return p.detach(), g


def closed_form(W, beta):
    """4 beta M Wm, M = (Wm Wm^T) o (1 - I)."""
    Wm = _wm(W)
    M = Wm @ Wm.t()
    M = M - torch.diag(torch.diagonal(M))
    return (4 * beta * M @ Wm).reshape(W.shape)


def row_form(W, beta):
    """(penalty, gradient) through S = Wm Wm^T with its diagonal zeroed: G = S Wm, penalty = beta sum(S^2)."""
    Wm = _wm(W)
    S = Wm @ Wm.t()
    S.fill_diagonal_(0.)
    return beta * (S ** 2).sum(), (4 * beta * S @ Wm).reshape(W.shape)


def column_form(W, beta):
    """(penalty, gradient) through S = Wm^T Wm and q = squared row norms: G = Wm S - q o Wm, penalty = beta (sum(S^2) - sum(q^2))."""
    Wm = _wm(W)
    S = Wm.t() @ Wm
    q = (Wm ** 2).sum(dim=1)
    return beta * ((S ** 2).sum() - (q ** 2).sum()), (4 * beta * (Wm @ S - q[:, None] * Wm)).reshape(W.shape)
