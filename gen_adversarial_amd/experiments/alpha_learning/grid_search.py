"""
Random search over the interpolation alphas (reference: src/experiments/alpha_learning/grid_search.py:9-77), same arguments and
the same two files: `<results_folder>/<autoencoder_name>_<classifier_type>/grid_search/{alphas,accuracies}.npy`, [n_steps, n] and
[n_steps, 1], the layout `get_best_combination` reads.  The candidates are scored several per engine pass
(AlphaEvaluator.objective_many); `--seed` and `--candidates_per_pass` are additions.

    python -m gen_adversarial_amd.experiments.alpha_learning.grid_search --adv_images_path ... --n_steps 100 ...
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .common_utils import AlphaEvaluator, random_search


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser('Load an MLVGM purification model and compute some alphas')
    parser.add_argument('--adv_images_path', type=str, required=True, help='Precomputed adversaries to use for evaluation')
    parser.add_argument('--n_steps', type=int, required=True)
    parser.add_argument('--classifier_path', type=str, required=True, help='path to the pre-trained classifier to be attacked')
    parser.add_argument('--classifier_type', type=str, choices=['resnet-50', 'vgg-11', 'resnext-50'], help='type of classifier')
    parser.add_argument('--autoencoder_path', type=str, required=True, help='path to the pre-trained autoencoder acting as a defense')
    parser.add_argument('--autoencoder_name', type=str, required=True, help='used to determine results folder')
    parser.add_argument('--results_folder', type=str, required=True, help='folder to save .numpy files with results')
    parser.add_argument('--seed', type=int, default=0, help='seed of the uniform alpha draws')
    parser.add_argument('--candidates_per_pass', type=int, default=None, help='alpha vectors per engine pass (default: from the row budget)')
    parser.add_argument('--batch_images', type=int, default=8, help='images per engine pass')
    args = parser.parse_args(argv)
    args.results_folder = f'{args.results_folder}/{args.autoencoder_name}_{args.classifier_type}/grid_search/'
    os.makedirs(args.results_folder, exist_ok=True)
    return args


def save_results(folder: str, alphas: np.ndarray, accuracies: np.ndarray):
    """alphas [n_steps, n], accuracies [n_steps, 1] as float32 (grid_search.py:71-72)"""
    os.makedirs(folder, exist_ok=True)
    np.save(f'{folder}/alphas.npy', np.asarray(alphas, dtype=np.float32))
    np.save(f'{folder}/accuracies.npy', np.asarray(accuracies, dtype=np.float32).reshape(-1, 1))


@torch.no_grad()
def main(args, evaluator: AlphaEvaluator = None):
    if evaluator is None:
        evaluator = AlphaEvaluator(args, 'cuda:0', batch_images=getattr(args, 'batch_images', 8))
    alphas, accuracies = random_search(evaluator, args.n_steps, seed=getattr(args, 'seed', 0),
                                       candidates_per_pass=getattr(args, 'candidates_per_pass', None))
    save_results(args.results_folder, alphas, accuracies)
    return alphas, accuracies


if __name__ == '__main__':
    main(parse_args())
