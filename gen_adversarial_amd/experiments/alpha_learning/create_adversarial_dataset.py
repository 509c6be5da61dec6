"""
Adversarial set for alpha learning (reference: src/experiments/alpha_learning/create_adversarial_dataset.py:19-121): FGSM at a fixed
L2 bound (4 / 2 / 4 for resnet-50 / vgg-11 / resnext-50) against the reconstruction-only defender (all alphas 0) under EoT 32; an
image is kept iff the attack reports `success and bound > 0` (images the defender already misclassifies come back with bound 0
and are dropped), until `n_samples` are found.  Kept adversaries are written as 8-bit PNG / JPEG under their own name,
`<results_folder>/<class folder>/<file name>`, like :107-112.  Several images go through the batched attack path per call.

    python -m gen_adversarial_amd.experiments.alpha_learning.create_adversarial_dataset --images_folder ... --n_samples 500 ...
"""
from __future__ import annotations

import argparse
import os
from typing import List, Tuple

import numpy as np
import torch

from ...attacks.l2_attacks import FGSM
from ...defenses.wrappers import EoTWrapper
from .common_utils import DEFENDERS

L2_BOUNDS = {'resnet-50': 4.0, 'vgg-11': 2.0, 'resnext-50': 4.0}


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser('Create Adversarial Dataset for Learning Alphas')
    parser.add_argument('--images_folder', type=str, required=True, help='Folder with images to make adversarial')
    parser.add_argument('--n_samples', type=int, required=True,
                        help='You likely want to run BO on a subset of the whole training dataset.')
    parser.add_argument('--results_folder', type=str, required=True, help='folder to save image adversaries')
    parser.add_argument('--classifier_path', type=str, required=True, help='path to the pre-trained classifier to be attacked')
    parser.add_argument('--autoencoder_path', type=str, required=True, help='path to the pre-trained HL Autoencoder')
    parser.add_argument('--classifier_type', type=str, choices=['resnet-50', 'vgg-11', 'resnext-50'], help='type of classifier')
    parser.add_argument('--batch_images', type=int, default=8, help='images per attack call')
    parser.add_argument('--seed', type=int, default=0, help='seed of the shuffle (the reference shuffles unseeded)')
    return parser.parse_args(argv)


def named_folder_dataset(folder: str, size: int) -> Tuple[torch.Tensor, List[Tuple[str, str]], torch.Tensor]:
    """ImageNameLabelDataset: the images of experiments.test_defense.folder_dataset (same order, same labels) with their
    (class folder, file name)"""
    import pathlib
    from ..test_defense import IMAGE_PATTERNS, folder_dataset
    images, labels = folder_dataset(folder, size)
    samples = sorted(p for pat in IMAGE_PATTERNS for p in pathlib.Path(folder).rglob(pat))
    names = [tuple(p.absolute().as_posix().split('/')[-2:]) for p in samples]
    return images, names, labels


def save_adversary(results_folder: str, name: Tuple[str, str], adversary: torch.Tensor):
    """adversary: (3, H, W) in [0, 1] -> results_folder/<class>/<file name>, values truncated to 8 bits (:112)"""
    from PIL import Image
    folder_name = f'{results_folder}/{name[0]}/'
    os.makedirs(folder_name, exist_ok=True)
    Image.fromarray((adversary * 255).permute(1, 2, 0).cpu().numpy().astype(np.uint8)).save(f'{folder_name}/{name[1]}')


def build_defender(args, device: str):
    """the reconstruction-only defender of :48-85 under EoT 32"""
    classifier, defender, n_alphas, _, args.image_size = DEFENDERS[args.classifier_type]
    base = classifier(args.classifier_path, device)
    n = len(getattr(args, 'initial_alphas', [0.] * n_alphas))
    model = defender(base, args.autoencoder_path, [0. for _ in range(n)], device=device).eval()     # reconstruction only
    return EoTWrapper(model, getattr(args, 'eot_steps', 32)).eval()


def create(net, attack, images: torch.Tensor, names: List[Tuple[str, str]], labels: torch.Tensor, n_samples: int, results_folder: str,
           batch_images: int = 8, seed: int = 0, device: str = None) -> List[Tuple[str, str]]:
    """attack the images in a shuffled order, `batch_images` per call, and save those with `success and bound > 0` until
    `n_samples` are kept; returns the kept names in the order they were found"""
    order = torch.randperm(images.shape[0], generator=torch.Generator().manual_seed(seed)).tolist()   # samples from all classes
    kept: List[Tuple[str, str]] = []
    for i in range(0, len(order), batch_images):
        if len(kept) >= n_samples:
            break
        idx = order[i:i + batch_images]
        x, y = torch.clamp(images[idx], 0., 1.), labels[idx]
        if device is not None:
            x, y = x.to(device), y.to(device)
        success, bound, adversary = attack(x, y, net)
        success = torch.as_tensor(success).view(-1)
        bound = torch.as_tensor(bound, dtype=torch.float32).view(-1)
        for j, k in enumerate(idx):
            if len(kept) >= n_samples:
                break
            if bool(success[j]) and float(bound[j]) > 0.:
                save_adversary(results_folder, names[k], adversary[j])
                kept.append(names[k])
    return kept


def main(args, net=None, device: str = 'cuda:0'):
    attack = FGSM(l2_bound=L2_BOUNDS[args.classifier_type])
    if net is None:
        net = build_defender(args, device)
    elif getattr(args, 'image_size', None) is None:      # an injected defender (tests) may come with its own image size
        args.image_size = DEFENDERS[args.classifier_type][4]
    images, names, labels = named_folder_dataset(args.images_folder, args.image_size)
    return create(net, attack, images, names, labels, args.n_samples, args.results_folder,
                  batch_images=getattr(args, 'batch_images', 8), seed=getattr(args, 'seed', 0), device=device)


if __name__ == '__main__':
    main(parse_args())
