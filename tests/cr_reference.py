"""Float64 restatement of consistency regularisation (gan_lab_amd/consistency.py; csrc/cr.hip) on the CPU: the image transform from
its definition, the two mean squared differences with their gradients, and the three critic terms and the generator term as plain
functions of critic and generator callables."""
import numpy as np
import torch


def transform(x, params):
    """``y[n,c,i,j] = x[n,c,i-dy, f(j-dx)]``, f(k) = W-1-k when the row's flip is set, 0 where i-dy or j-dx leaves the image;
    ``params`` rows are (flip, dx, dy, 0).  Element by element, from the definition; keeps ``x``'s dtype."""
    x = np.asarray(x)
    params = np.asarray(params)
    n_, c_, h, w = x.shape
    y = np.zeros_like(x)
    for n in range(n_):
        flip, dx, dy = int(params[n][0]), int(params[n][1]), int(params[n][2])
        for i in range(h):
            si = i - dy
            if si < 0 or si >= h:
                continue
            for j in range(w):
                k = j - dx
                if k < 0 or k >= w:
                    continue
                y[n, :, i, j] = x[n, :, si, w - 1 - k if flip else k]
    return y


def transform_t(x, params):
    """``transform`` of a torch tensor (any float dtype), as a constant: the critic step transforms detached batches."""
    return torch.from_numpy(transform(x.detach().cpu().numpy(), np.asarray(params))).to(x.dtype)


def msd(a, b):
    """Mean over the batch of the squared difference of two score vectors (float64 torch; differentiable)."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b) ** 2).mean()


def msd_grads(a, b, gout=1.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ga = 2.0 / a.size * (a - b) * gout
    return ga, -ga


def imsd(a, b):
    """Mean over every element of the squared difference of two image batches (float64 torch; differentiable)."""
    return ((a.double() - b.double()) ** 2).mean()


imsd_grads = msd_grads        # the same formula over all elements


def perturb(z, noise, sigma):
    return z + sigma * noise


def critic_terms(disc, gen, x, z, noise, params, sigma, real=True, fake=True, latent=True):
    """The unweighted critic-step terms {'cr_real', 'cr_fake', 'cr_latent_d'} (those asked for) for a critic ``disc(images)`` and
    a generator ``gen(latents)`` (labels, if any, closed over; called once, under no_grad, on ``[z; z']`` when ``latent`` - its
    BatchNorm statistics are taken over both halves - else on ``z``).  ``params``: (2N, 4) rows, [0, N) for the generated batch and
    [N, 2N) for the real one.  Also returns (G(z), D(G(z)), D(x)) for the adversarial part of the loss."""
    n = z.shape[0]
    with torch.no_grad():
        if latent:
            both = gen(torch.cat((z, perturb(z, noise, sigma))))
            g_z, g_zp = both[:n], both[n:]
        else:
            g_z = gen(z)
    d_gen, d_real = disc(g_z), disc(x)
    out = {}
    if real:
        out['cr_real'] = msd(d_real, disc(transform_t(x, params[n:])))
    if fake:
        out['cr_fake'] = msd(d_gen, disc(transform_t(g_z, params[:n])))
    if latent:
        out['cr_latent_d'] = msd(d_gen, disc(g_zp))
    return out, (g_z, d_gen, d_real)


def generator_term(gen, z, noise, sigma):
    """imsd(G(z), G(z')) with ONE generator pass over ``[z; z']``; also returns G(z) (the half that goes on to the critic)."""
    n = z.shape[0]
    both = gen(torch.cat((z, perturb(z, noise, sigma))))
    return imsd(both[:n], both[n:]), both[:n]
