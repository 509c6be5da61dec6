"""
Gradient descent on the interpolation alphas: the first-order tool beside grid_search.py and bayesian_optimization.py (not in the
reference, whose two searches treat the defender as a black box).  `AlphaEvaluator.loss_and_gradient` gives the mean cross-entropy of
the EoT-mean logits on the adversarial set and its exact gradient in all alphas from one forward and one backward pass per chunk;
this script runs projected Adam on [0, 1]^n with it (plain torch on the host).  Every `--eval_every` steps, and at the end, the
current vector is scored with `objective_function` (EoT accuracy, the quantity the searches maximise).  Files:
`<results_folder>/<autoencoder_name>_<classifier_type>/gradient_descent/{alphas,accuracies,losses}.npy`, [k, n], [k, 1], [k, 1] for
the k scored vectors — `alphas.npy` / `accuracies.npy` in the grid_search layout `get_best_combination` reads.

The loss is a surrogate of the accuracy, and every pass has fresh latent draws (a stochastic gradient).  Whether descent on it finds
better alphas than the Bayesian search has not been measured: no full-size checkpoint has been run through this script.

    python -m gen_adversarial_amd.experiments.alpha_learning.gradient_descent --adv_images_path ... --steps 100 --lr 0.05 ...
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .common_utils import AlphaEvaluator, get_best_combination, get_cosine_alphas, get_linear_alphas
from .grid_search import save_results


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser('Load an MLVGM purification model and learn its alphas by gradient descent')
    parser.add_argument('--adv_images_path', type=str, required=True, help='Precomputed adversaries to use for evaluation')
    parser.add_argument('--n_steps', type=int, default=None, help='as for grid_search: used as --steps when that is not given')
    parser.add_argument('--classifier_path', type=str, required=True, help='path to the pre-trained classifier to be attacked')
    parser.add_argument('--classifier_type', type=str, choices=['resnet-50', 'vgg-11', 'resnext-50'], help='type of classifier')
    parser.add_argument('--autoencoder_path', type=str, required=True, help='path to the pre-trained autoencoder acting as a defense')
    parser.add_argument('--autoencoder_name', type=str, required=True, help='used to determine results folder')
    parser.add_argument('--results_folder', type=str, required=True, help='folder to save .numpy files with results')
    parser.add_argument('--seed', type=int, default=0, help='seed of the latent draws')
    parser.add_argument('--candidates_per_pass', type=int, default=None, help='accepted for symmetry with grid_search; unused')
    parser.add_argument('--batch_images', type=int, default=8, help='images per engine pass')
    parser.add_argument('--steps', type=int, default=None, help='descent steps (default: --n_steps, else 100)')
    parser.add_argument('--lr', type=float, default=0.05, help='Adam step size')
    parser.add_argument('--init', type=str, default='linear', help='linear | cosine | zeros | best_of:<folder of a finished search>')
    parser.add_argument('--eval_every', type=int, default=10, help='score the current vector every this many steps')
    args = parser.parse_args(argv)
    args.results_folder = f'{args.results_folder}/{args.autoencoder_name}_{args.classifier_type}/gradient_descent/'
    os.makedirs(args.results_folder, exist_ok=True)
    return args


def initial_vector(init: str, n: int) -> torch.Tensor:
    """float64 [n] inside the box"""
    if init == 'linear':
        v = get_linear_alphas(n)
    elif init == 'cosine':
        v = get_cosine_alphas(n)
    elif init == 'zeros':
        v = [0.0] * n
    elif init.startswith('best_of:'):
        v = get_best_combination(init[len('best_of:'):]).tolist()
        if len(v) != n:
            raise ValueError(f'{init}: {len(v)} alphas stored, the defender has {n}')
    else:
        raise ValueError(f"--init must be linear, cosine, zeros or best_of:<folder>, got '{init}'")
    return torch.tensor(v, dtype=torch.float64).clamp_(0.0, 1.0)


def projected_adam(loss_and_gradient, x0: torch.Tensor, steps: int, lr: float, on_step=None, betas=(0.9, 0.999), eps: float = 1e-8):
    """Adam (Kingma & Ba 2015) with every iterate projected onto [0, 1]^n.  loss_and_gradient(list) -> (float, array [n]) is called at
    the `steps + 1` iterates x_0 .. x_steps; on_step(t, x_t, loss_t) sees each of them.  Returns x_steps."""
    x = x0.detach().to(torch.float64).clone()
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(steps + 1):
        loss, g = loss_and_gradient(x.tolist())
        if on_step is not None:
            on_step(t, x, float(loss))
        if t == steps:
            break
        g = torch.as_tensor(np.asarray(g), dtype=torch.float64)
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        step = lr * (m / (1 - betas[0] ** (t + 1))) / ((v / (1 - betas[1] ** (t + 1))).sqrt() + eps)
        x = (x - step).clamp_(0.0, 1.0)
    return x


def main(args, evaluator: AlphaEvaluator = None):
    if evaluator is None:
        evaluator = AlphaEvaluator(args, 'cuda:0', batch_images=getattr(args, 'batch_images', 8))
    n = len(evaluator.defense_model.model.interpolation_alphas)
    steps = getattr(args, 'steps', None)
    steps = (getattr(args, 'n_steps', None) or 100) if steps is None else int(steps)
    eval_every = max(1, int(getattr(args, 'eval_every', 10)))
    if steps < 0:
        raise ValueError('steps must not be negative')
    torch.manual_seed(getattr(args, 'seed', 0))
    rows = []

    def on_step(t, x, loss):
        if t % eval_every == 0 or t == steps:
            acc = float(evaluator.objective_function(x.tolist()))
            print(f'[INFO] step {t}: loss {loss:.6f} accuracy {acc:.4f}')
            rows.append((x.clone().numpy(), acc, loss))

    projected_adam(evaluator.loss_and_gradient, initial_vector(getattr(args, 'init', 'linear'), n), steps,
                   float(getattr(args, 'lr', 0.05)), on_step)
    alphas = np.stack([r[0] for r in rows]).astype(np.float32)
    accuracies = np.asarray([r[1] for r in rows], dtype=np.float32).reshape(-1, 1)
    losses = np.asarray([r[2] for r in rows], dtype=np.float32).reshape(-1, 1)
    save_results(args.results_folder, alphas, accuracies)
    np.save(f'{args.results_folder}/losses.npy', losses)
    return alphas, accuracies, losses


if __name__ == '__main__':
    main(parse_args())
