"""Plain torch restatement of BigGAN's generator conditioning (Brock et al. 2019, section 3 and appendix B; self-modulation: Chen
et al. 2019) as gan_lab_amd/hier_latent.py builds it - written from the papers, usable in fp32 and float64, gradients by autograd.

    chunk layout    chunk = len_latent // (B + 1); the first linear reads z[:, :len_latent - B * chunk], block b the next chunk
    cond_b[n]       = [z_b[n], shared[labels[n]]]                      (whichever parts are on)
    modulation      gain_j = 1 + s_j cond_b W_j^T (N, C_j), shift_j = s_j cond_b W_j^T, laid side by side in one (N, T) buffer
    modulated BN    y = act((x - mean) * rstd * gain[n, c] + shift[n, c]), batch statistics (biased variance) in training mode,
                    the running ones as constants in eval mode
"""
import torch
import torch.nn.functional as F


def chunk_layout(len_latent, blocks):
    """-> (width of the first linear's input, [(offset, width)] per block)."""
    if len_latent < blocks + 1:
        raise ValueError('len_latent < blocks + 1')
    chunk = len_latent // (blocks + 1)
    first = len_latent - blocks * chunk
    return first, [(first + b * chunk, chunk) for b in range(blocks)]


def cond(z, z_off, z_len, shared=None, labels=None):
    """cond_b (N, z_len + E)."""
    parts = [z[:, z_off:z_off + z_len]]
    if shared is not None:
        parts.append(shared[labels.long()])
    return torch.cat(parts, dim=1)


def modulation(z, jobs, shared=None, labels=None, dtype=None):
    """The flat (N, T) buffer.  ``jobs``: [(W (C, D), z_off, z_len, scale, one)] in column order."""
    dtype = dtype or z.dtype
    z = z.to(dtype)
    shared = shared.to(dtype) if shared is not None else None
    cols = []
    for W, z_off, z_len, scale, one in jobs:
        cols.append(one + scale * F.linear(cond(z, z_off, z_len, shared, labels), W.to(dtype)))
    return torch.cat(cols, dim=1)


def modulation_with_grads(z, jobs, shared, labels, g, dtype):
    """-> [out, dz, dshared (or None), dW_0, dW_1, ...] in ``dtype``."""
    zl = z.detach().to(dtype).requires_grad_(True)
    sl = shared.detach().to(dtype).requires_grad_(True) if shared is not None else None
    Ws = [W.detach().to(dtype).requires_grad_(True) for W, *_ in jobs]
    out = modulation(zl, [(W,) + tuple(j[1:]) for W, j in zip(Ws, jobs)], sl, labels)
    leaves = [zl] + ([sl] if sl is not None else []) + Ws
    grads = torch.autograd.grad(out, leaves, g.to(dtype), allow_unused=True)
    grads = [torch.zeros_like(l) if gr is None else gr for gr, l in zip(grads, leaves)]
    dz, rest = grads[0], grads[1:]
    dshared = rest.pop(0) if sl is not None else None
    return [out.detach(), dz, dshared] + list(rest)


def mod_batch_norm(x, gain, shift, eps=1e-5, act_slope=None, dtype=None):
    """Training mode: batch statistics, biased variance."""
    dtype = dtype or x.dtype
    x = x.to(dtype)
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    y = (x - mean) * torch.rsqrt(var + eps) * gain.to(dtype)[:, :, None, None] + shift.to(dtype)[:, :, None, None]
    return y if act_slope is None else F.leaky_relu(y, act_slope)


def mod_batch_norm_eval(x, gain, shift, running_mean, running_var, eps=1e-5, act_slope=None, dtype=None):
    """Eval mode: the running statistics are constants."""
    dtype = dtype or x.dtype
    x = x.to(dtype)
    mean, var = running_mean.to(dtype)[None, :, None, None], running_var.to(dtype)[None, :, None, None]
    y = (x - mean) * torch.rsqrt(var + eps) * gain.to(dtype)[:, :, None, None] + shift.to(dtype)[:, :, None, None]
    return y if act_slope is None else F.leaky_relu(y, act_slope)


def mod_batch_norm_with_grads(x, gain, shift, gy, dtype, eps=1e-5):
    """-> (y, gx, dgain, dshift) in ``dtype``."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gain, shift)]
    y = mod_batch_norm(*leaves, eps=eps)
    return (y.detach(),) + torch.autograd.grad(y, leaves, gy.to(dtype))


def generator(gen, z, labels=None):
    """The forward of a gan_lab_amd ResNet generator built with hier_latent / shared_embed, composed from torch ops on the
    generator's own parameters (any device / dtype they have); gradients by autograd.  Nearest upsampling, ReLU, no blur, no
    attention - the networks' defaults."""
    from gan_lab_amd.resnetgan.resblocks import ResBlock2d
    from gan_lab_amd.utils.custom_layers import Conv2dEx, ModulatedBatchNorm2d
    seq = list(gen.generator_model)
    blocks = [m for m in seq if isinstance(m, ResBlock2d)]
    first = seq[1].linear.weight.shape[1]
    z = z.view(-1, gen.len_latent)
    shared = gen.shared.weight if gen.shared_embed else None
    lin = seq[1]
    h = F.linear(z[:, :first], lin.linear.weight * lin.scale, lin.linear.bias)
    h = h.view(z.shape[0], -1, 4, 4)

    def norm(m, h, c):
        gain = 1 + m.gain.scale * F.linear(c, m.gain.linear.weight)
        shift = m.shift.scale * F.linear(c, m.shift.linear.weight)
        return F.relu(mod_batch_norm(h, gain, shift, eps=m.eps))

    def conv(m, h):
        return F.conv2d(h, m.conv2d.weight * m.scale, m.conv2d.bias, padding=m.padding)

    for blk, (_, z_off, z_len) in zip(blocks, gen.hier.norms[::2]):
        c = cond(z, z_off, z_len, shared, labels)
        n1, n2 = [m for m in blk.modules() if isinstance(m, ModulatedBatchNorm2d)]
        c1, c2, cs = blk.convs
        up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')      # noqa: E731
        a = conv(c1, up(norm(n1, h, c)))
        a = conv(c2, norm(n2, a, c))
        h = conv(cs, up(h)) + a
    bn = seq[-4].norm
    h = F.relu(F.batch_norm(h, None, None, bn.weight, bn.bias, True, 0.0, bn.eps))
    last = seq[-2]
    assert isinstance(last, Conv2dEx)
    return torch.tanh(conv(last, h))
