"""One seeded run of a ResNet GAN 32-pixel learner under the six-part ADA policy at fixed p = 0.5, in a process of its own
(tests/test_gpu_ada_ext.py starts two): three critic and generator iterations, then one JSON line with the losses, the stream
position, p, whether every tensor is finite and a SHA-256 digest of every tensor of both networks and of the ADA state."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import contextlib
    import io
    import numpy as np
    import torch
    from gan_lab_amd import rng
    from gan_lab_amd.config import make_config
    from gan_lab_amd.resnetgan.learner import GANLearner
    gen = torch.Generator().manual_seed(5)
    reals = [(torch.rand(4, 3, 32, 32, generator=gen) * 2 - 1).cuda() for _ in range(3)]
    torch.manual_seed(4)
    np.random.seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        cfg = make_config('resnetgan', dev='cuda', pin_memory=False, res_samples=32, res_dataset=32, batch_size=4,
                          num_iters_save_model=10 ** 9, log_every=0, len_latent=16, random_seed=4,
                          ada='blit,geom,color,filter,noise,cutout', ada_p=0.5, ada_target=None)
        cfg.fmap_g, cfg.fmap_d = 8, 8
        L = GANLearner(cfg)
    L.gen_model.train()
    L.disc_model.train()
    losses = []
    for x in reals:
        L.set_requires_grad_disc(True)
        ld = L.d_step(x)
        L.set_requires_grad_disc(False)
        lg = L.g_step()
        losses.append((float(ld), float(lg)))
    torch.cuda.synchronize()
    state = [('g.' + k, v) for k, v in L.gen_model.state_dict().items()] + \
        [('d.' + k, v) for k, v in L.disc_model.state_dict().items()] + [('ada', L.ada.state)]
    digests = {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in state}
    finite = all(bool(torch.isfinite(v).all()) for _, v in state if v.is_floating_point())
    print(json.dumps(dict(losses=losses, offset=rng._STATE['offset'], p=L.ada.p, finite=finite, digests=digests)))


if __name__ == '__main__':
    main()
