"""Spectral normalisation of the ResNet GAN critic (Miyato et al. 2018), batched over all of its layers.

``config.spectral_norm = True`` (ResNet GAN only, default False) divides every ``Conv2dEx`` (3x3 and the 1x1 skips) and
``LinearEx`` weight of ``Discriminator32PixResnet`` / ``Discriminator64PixResnet`` by an estimate of its largest singular
value.  The arithmetic is ``torch.nn.utils.spectral_norm``'s with one power iteration: for a parameter ``W`` viewed as
``Wm = W.reshape(Cout, -1)``, stored unit vectors ``u``, ``v`` and ``eps = 1e-12``

    iterate:   t = Wm^T u ; v <- t / max(|t|, eps) ; s = Wm v ; u <- s / max(|s|, eps)
    always:    sigma = u^T Wm v ;  W_sn = W / sigma
    backward:  gW = (g_sn - <g_sn, W_sn> u v^T) / sigma          (u, v constants)

What differs from torch's per-layer hooks is WHERE it runs.  The layers never compute anything: the manager below owns one
flat ``W_sn`` buffer next to the critic's parameter arena, and the layers read their slice of it (``weight_override``) as
an ordinary leaf tensor.  ``refresh`` rewrites the whole buffer in 4 launches (2 without the power iteration) and
``backward`` folds the gradients that the step left on ``W_sn`` back into the parameter-gradient arena in 2, whatever the
number of layers (csrc/spectral.hip) - per-layer hooks would add about 6 small launches per layer and forward.  The
parameter keys (``conv2d.weight`` / ``linear.weight``), arenas, Adam moments and checkpoints keep their layout; ``u`` and
``v`` are the buffers ``conv2d.weight_u`` / ``conv2d.weight_v`` (``linear.weight_u`` / ``linear.weight_v``) of the layers -
views into the manager's storage - and travel through ``state_dict``.

Schedule (resnetgan/learner.py): ``refresh(iterate=True)`` at the start of every critic step, ``refresh(iterate=False)``
at the start of every generator step and before any other use of the critic - sigma and ``W_sn`` then follow the moved
weights with the stored ``u``, ``v``.  That is one power iteration per critic UPDATE, not one per training-mode forward
as with torch's hook (which would iterate two or three times per critic step here: generated batch, real batch, penalty).
A fresh manager runs 15 iterating refreshes, like torch at registration.

The penalties' double backward differentiates towards the critic's INPUT, so it only ever leaves a first-order gradient
on ``W_sn``; the backward above is first-order and is applied once per step, after ``loss.backward()``.
"""
import torch

from . import ops

_ALIGN = 4          # floats: every slot 16-byte aligned (optim.ParamArena's rule; the kernels' float4 path relies on it)
INIT_ITERS = 15     # torch.nn.utils.spectral_norm runs 15 power iterations when it is registered


def _round_up(n, m):
    return (n + m - 1) // m * m


def validate_config(config):
    """``config.spectral_norm`` against the options it excludes; raises ValueError.  -> bool (is it on?)."""
    on = getattr(config, 'spectral_norm', False)
    if not isinstance(on, bool):
        raise ValueError(f'config.spectral_norm must be a bool (got {on!r})')
    if on and getattr(config, 'model', 'ResNet GAN') != 'ResNet GAN':
        raise ValueError('config.spectral_norm is a ResNet GAN option (the progressive critics are not normalised)')
    if on and getattr(config, 'use_equalized_lr', False):
        raise ValueError('config.spectral_norm excludes config.use_equalized_lr: a constant runtime scale of the weight '
                         'cancels in W / sigma(W)')
    return on


def check_save_format(spectral_norm, reference_format):
    """A reference-format checkpoint has no place for u, v (the reference has no spectral normalisation)."""
    if spectral_norm and reference_format:
        raise ValueError('spectral_norm=True cannot be saved with reference_format=True: the reference has no spectral '
                         'normalisation (weight_u / weight_v would be dropped and W is not the weight the critic applies)')


def normalised_layers(critic):
    """[(prefix, container module, weight parameter)] of every Conv2dEx / LinearEx of ``critic``, in module order."""
    from .utils.custom_layers import Conv2dEx, LinearEx
    out = []
    for name, m in critic.named_modules():
        if isinstance(m, Conv2dEx):
            out.append((name + '.conv2d', m, m.conv2d))
        elif isinstance(m, LinearEx):
            out.append((name + '.linear', m, m.linear))
    return out


def register_uv(critic):
    """Give every normalised layer its ``weight_u`` / ``weight_v`` buffers (random unit vectors, as torch initialises them);
    a ``SpectralNorm`` manager later re-homes them into its own storage."""
    for _, layer, holder in normalised_layers(critic):
        if layer.equalized_lr:
            raise ValueError('spectral_norm=True excludes equalized_lr=True: a constant runtime scale of the weight cancels '
                             'in W / sigma(W)')
        w = holder.weight
        r, k = w.shape[0], w.numel() // w.shape[0]
        for name, n in (('weight_u', r), ('weight_v', k)):
            holder.register_buffer(name, torch.nn.functional.normalize(w.new_empty(n).normal_(0, 1), dim=0, eps=ops.SN_EPS))
    critic.sn = None


class SpectralNorm(object):
    """``sn = SpectralNorm(critic, arena)``: the critic (built with ``spectral_norm=True``) whose parameters live in
    ``arena`` (an ``optim.ParamArena``) reads normalised weights from here on.

    ``init_iters``: iterating refreshes run now - ``INIT_ITERS`` for a new critic, 0 when the buffers already hold a
    trained ``u``, ``v`` (a checkpoint was loaded into the critic and its arenas are rebuilt)."""

    def __init__(self, critic, arena, init_iters=INIT_ITERS):
        layers = normalised_layers(critic)
        if not layers or not hasattr(layers[0][2], 'weight_u'):
            raise ValueError('SpectralNorm: the critic was not built with spectral_norm=True')
        self.critic, self.arena = critic, arena
        dev = arena.flat.device
        self.names, self.offsets, self.sizes, self.uv_offsets, self.shapes = [], [], [], [], []
        off = uv = 0
        for prefix, _, holder in layers:
            w = holder.weight
            r, k = w.shape[0], w.numel() // w.shape[0]
            self.names.append(prefix + '.weight')
            self.shapes.append((r, k))
            self.offsets.append(off)
            self.sizes.append(w.numel())
            off += _round_up(w.numel(), _ALIGN)
            self.uv_offsets.append((uv, uv + _round_up(r, _ALIGN), uv + _round_up(r, _ALIGN) + _round_up(k, _ALIGN)))
            uv += _round_up(r, _ALIGN) + _round_up(k, _ALIGN) + _ALIGN
        self.total = off
        self.serial = 0                      # ops.direct_param_grads writes each W_sn gradient slot once per step
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)       # W_sn of every layer
        self.gflat = torch.zeros(off, dtype=torch.float32, device=dev)      # d loss / d W_sn
        self.uv = torch.zeros(uv, dtype=torch.float32, device=dev)          # per layer: u | v | sigma
        self.weights, self.sigmas, jobs = [], [], []
        for (prefix, layer, holder), o, n, (ou, ov, osg), (r, k) in zip(layers, self.offsets, self.sizes, self.uv_offsets,
                                                                       self.shapes):
            p = holder.weight
            if getattr(p, '_ganlab_arena', None) is not arena:
                raise ValueError(f'SpectralNorm: {prefix}.weight does not live in the given arena')
            u, v, sg = self.uv[ou:ou + r], self.uv[ov:ov + k], self.uv[osg:osg + 1]
            with torch.no_grad():
                u.copy_(holder.weight_u)
                v.copy_(holder.weight_v)
            holder._buffers['weight_u'], holder._buffers['weight_v'] = u, v      # same keys, the manager's storage
            # a leaf with its .grad preset, like an arena parameter: ops.direct_param_grads sinks work on it as they do there
            w_sn = torch.empty(0, dtype=torch.float32, device=dev).requires_grad_(True)
            w_sn.data = self.flat[o:o + n].view(p.shape)
            w_sn.grad = self.gflat[o:o + n].view(p.shape)
            w_sn._ganlab_arena = self
            layer.weight_override = w_sn
            self.weights.append(w_sn)
            self.sigmas.append(sg)
            jobs.append(dict(w=p.data, w_sn=w_sn.data, g_sn=w_sn.grad, gw=p.grad, u=u, v=v, sigma=sg))
        self.table = ops.SnTable(jobs)
        critic.sn = self
        for _ in range(int(init_iters)):
            self.refresh(iterate=True)
        if not init_iters:
            self.refresh(iterate=False)

    def _check_attached(self):
        if not self.arena.is_attached():
            raise RuntimeError('SpectralNorm: the critic\'s parameters left their arena (the job table points into it); '
                               'rebuild the arena and the manager')

    def refresh(self, iterate):
        """sigma and W_sn of every layer from the current weights, after one power iteration when ``iterate``."""
        self._check_attached()
        ops.sn_refresh(self.table, bool(iterate))
        lo = self.flat.data_ptr()
        ops.bump_weight_epoch([(lo, lo + 4 * self.total)])      # every packed form of every W_sn: one batched re-pack

    def backward(self):
        """Call once after ``loss.backward()``: the gradients the step left on W_sn, through the normalisation, are
        ACCUMULATED into the parameter-gradient arena; the W_sn gradient buffer is zeroed for the next step."""
        self._check_attached()
        ops.sn_backward(self.table)
        self.zero_grad()

    def zero_grad(self):
        self.gflat.zero_()
        self.serial += 1

    def requires_grad_(self, flag):
        """With the critic frozen (generator step) no gradient towards W_sn is computed either."""
        for w in self.weights:
            w.requires_grad_(flag)

    def sigma(self):
        """{parameter key: stored sigma (a 1-element device tensor)}."""
        return dict(zip(self.names, self.sigmas))

    @staticmethod
    def validate_config(config):
        return validate_config(config)
