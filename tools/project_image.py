#!/usr/bin/env python3
"""Project images into the latent space of a trained StyleGAN (gan_lab_amd/project.py).

    python tools/project_image.py --checkpoint model.tar --out outdir [--space w|w+] [--steps 1000] [--seed 0] a.png b.png ...

Loads the checkpoint into a StyleGANLearner built from the configuration the checkpoint carries, resizes every image to the
generator's current resolution, projects them together and writes

    outdir/ws.npy           (N, L, D) float32: the projected dlatents
    outdir/projection.png   one row per image: the target beside its reconstruction
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_targets(paths, res):
    """(N, 3, res, res) float32 in [0, 1] from image files (PIL; resized with its bicubic filter where the size differs)."""
    from PIL import Image
    out = []
    for path in paths:
        img = Image.open(path).convert('RGB')
        if img.size != (res, res):
            img = img.resize((res, res), Image.BICUBIC)
        out.append(torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.)
    return torch.stack(out)


def side_by_side(targets, images):
    """uint8 (N * R, 2 * R, 3): row n = target n beside reconstruction n."""
    pair = torch.cat((targets.cpu(), images.detach().cpu().clamp(0., 1.)), dim=3)            # (N, 3, R, 2R)
    return (pair.permute(0, 2, 3, 1).reshape(-1, pair.shape[3], 3) * 255.).round().to(torch.uint8).numpy()


def load_learner(checkpoint, dev):
    """A StyleGANLearner with the architecture the checkpoint was trained with, and the checkpoint loaded into it."""
    from gan_lab_amd import checkpoint as ckpt
    from gan_lab_amd.config import make_config
    from gan_lab_amd.stylegan.learner import StyleGANLearner
    conf = ckpt.config_dict(ckpt.load_checkpoint(checkpoint))
    if str(conf.get('model', '')).casefold() != 'stylegan':
        raise SystemExit(f'{checkpoint}: a {conf.get("model")!r} checkpoint; only StyleGAN has a W space')
    defaults = vars(make_config('stylegan', dev=dev, pin_memory=False))
    arch = {k: conf[k] for k in ckpt.ARCH_FIELDS if k in conf and k in defaults and k != 'model'}
    learner = StyleGANLearner(make_config('stylegan', dev=dev, pin_memory=False, **arch))
    learner.load_model(checkpoint)
    return learner


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('images', nargs='+')
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--space', default='w', choices=('w', 'w+'))
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--noise_mode', default='const', choices=('const', 'none'))
    ap.add_argument('--snapshot', action='store_true', help='project into the live generator instead of the time-averaged one')
    ap.add_argument('--dev', default='cuda')
    args = ap.parse_args()
    learner = load_learner(args.checkpoint, args.dev)
    res = int(learner.gen_model.curr_res)
    targets = load_targets(args.images, res)
    out = learner.project(targets.to(args.dev), steps=args.steps, space=args.space, noise_mode=args.noise_mode, seed=args.seed,
                          time_average=not args.snapshot)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, 'ws.npy'), out.ws.cpu().numpy())
    from PIL import Image
    Image.fromarray(side_by_side(targets, out.images)).save(os.path.join(args.out, 'projection.png'))
    loss = out.loss.cpu()
    for path, first, last in zip(args.images, loss[0].tolist(), loss[-1].tolist()):
        print(f'{path}: loss {first:.6g} -> {last:.6g}')
    print(f'wrote {os.path.join(args.out, "ws.npy")} and {os.path.join(args.out, "projection.png")}')


if __name__ == '__main__':
    main()
