"""
Alpha-learning objective on the fast forward path (reference: src/experiments/alpha_learning/common_utils.py:15-103).
`AlphaEvaluator.objective_function(alphas)` = EoT-32 accuracy of the defender, with the given interpolation alphas, on
a pre-computed adversarial set, for the three defenders.  The reference walks the set one image at a time; here `batch_images`
images x 32 EoT rows go through the engine per call (the objective is forward-only and embarrassingly parallel over images), and
`objective_many` scores several alpha vectors per call: the candidates and EoT replicas of an image share its encoder pass.
`loss_and_gradient(alphas)` is the first-order tool beside them: mean cross-entropy and its exact gradient in the alphas from one
backward pass (gradient_descent.py).  `random_search` is grid_search.py:44-72; the Bayesian optimisation (bayesian_optimization.py, on the project's own Gaussian-process
surrogate in gp.py instead of BoTorch) proposes `objective_many`-sized rounds.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from ...defenses.ours.models import (CarsTypeClassifier, CelebaGenderClassifier, CelebaIdentityClassifier, E4EStyleGanDefenseModel,
                                      NVAEDefenseModel, TransStyleGanDefenseModel)
from ...defenses.wrappers import EoTWrapper


def get_linear_alphas(n: int) -> list:
    return [i / n for i in range(1, n + 1)]


def get_cosine_alphas(n: int) -> list:
    return [0.5 * (1 - math.cos(math.pi * (i / n))) for i in range(1, n + 1)]


def get_best_combination(folder: str) -> np.ndarray:
    alphas = np.load(f'{folder}/alphas.npy')
    accuracies = np.load(f'{folder}/accuracies.npy')[:, 0]
    return alphas[accuracies.argmax()]


# classifier_type -> (classifier class, defender class, number of alphas, alpha attenuation, image size): the reference's three
# branches (src/experiments/alpha_learning/common_utils.py:39-70)
DEFENDERS = {'vgg-11': (CelebaIdentityClassifier, NVAEDefenseModel, 24, 0.7, 64),
             'resnet-50': (CelebaGenderClassifier, E4EStyleGanDefenseModel, 18, 1.0, 256),
             'resnext-50': (CarsTypeClassifier, TransStyleGanDefenseModel, 16, 0.7, 128)}

# Rows (images x candidates x EoT replicas) of one candidate-batched engine pass.  The shipped NVAE conv plans are tuned for 1024-row
# chunks, so the default fills one: batch_images = 8 at EoT 32 gives 4 candidates per pass.  The StyleGAN defenders
# decode at 1024 / 512 px, where the activations of 256 rows are what a pass can hold: they default to one candidate per pass.
ROW_BUDGET = {'vgg-11': 1024, 'resnet-50': 256, 'resnext-50': 256}


class AlphaEvaluator:
    def __init__(self, args, device, images: torch.Tensor = None, labels: torch.Tensor = None, batch_images: int = 8):
        """args: classifier_type ('vgg-11' | 'resnet-50' | 'resnext-50'), classifier_path, autoencoder_path, [adv_images_path];
        optional initial_alphas (its length = the number of alphas of a reduced checkpoint) and eot_steps."""
        self.device = device
        self.eot_steps = 32
        self.batch_images = batch_images
        if args.classifier_type not in DEFENDERS:
            raise ValueError(f'Unknown classifier type: {args.classifier_type}')
        classifier, defender, n_alphas, self.alpha_attenuation, args.image_size = DEFENDERS[args.classifier_type]
        self.classifier_type = args.classifier_type
        base = classifier(args.classifier_path, device)
        n = len(getattr(args, 'initial_alphas', [0.] * n_alphas))
        self.defense_model = defender(base, args.autoencoder_path, [0. for _ in range(n)],
                                      alpha_attenuation=self.alpha_attenuation, device=device).eval()
        self.eot_steps = getattr(args, 'eot_steps', self.eot_steps)
        self.defense_model = EoTWrapper(self.defense_model, self.eot_steps).eval()
        if images is None:
            from ..test_defense import folder_dataset
            images, labels = folder_dataset(args.adv_images_path, args.image_size)
        self.images, self.labels = images.to(device), labels.to(device)

    @torch.no_grad()
    def per_image_verdicts(self, alphas: Sequence[float]) -> torch.Tensor:
        """the (N,) bool tensor the objective averages: EoT-mean prediction == label, per image of the adversarial set"""
        alphas = alphas.cpu().tolist() if isinstance(alphas, torch.Tensor) else list(alphas)
        self.defense_model.model.interpolation_alphas = [a * self.alpha_attenuation for a in alphas]
        hits = []
        for i in range(0, self.images.shape[0], self.batch_images):
            x, y = self.images[i:i + self.batch_images], self.labels[i:i + self.batch_images]
            hits.append(torch.eq(self.defense_model(x).argmax(dim=1), y))
        return torch.cat(hits)

    @torch.no_grad()
    def objective_function(self, alphas: Sequence[float]) -> float:
        return torch.mean(self.per_image_verdicts(alphas).to(torch.float32)).item()

    def loss_and_gradient(self, alphas: Sequence[float]):
        """(float, float64 [n]): the mean over the adversarial set of the cross-entropy of the EoT-mean logits, and its gradient in the
        UN-attenuated vector the caller passes (the defender differentiates in its stored alphas = alphas * alpha_attenuation, so
        its gradient is multiplied by the attenuation).  One forward and one backward pass per `batch_images` chunk
        (EoTWrapper.loss_and_alpha_grad); fresh draws per chunk, like the objective."""
        alphas = alphas.cpu().tolist() if isinstance(alphas, torch.Tensor) else list(alphas)
        self.defense_model.model.interpolation_alphas = [a * self.alpha_attenuation for a in alphas]
        loss, grad, count = 0.0, np.zeros(len(alphas), dtype=np.float64), self.images.shape[0]
        for i in range(0, count, self.batch_images):
            x, y = self.images[i:i + self.batch_images], self.labels[i:i + self.batch_images]
            l, g = self.defense_model.loss_and_alpha_grad(x, y)
            loss += float(l.double().sum())
            grad += g.double().sum(dim=0).cpu().numpy()
        return loss / count, grad * (self.alpha_attenuation / count)

    def default_candidates_per_pass(self) -> int:
        """candidates per engine pass from the row budget: ROW_BUDGET // (batch_images x EoT), at least 1"""
        return max(1, ROW_BUDGET[self.classifier_type] // (self.batch_images * self.eot_steps))

    @torch.no_grad()
    def per_image_verdicts_many(self, alphas, candidates_per_pass: int = None) -> np.ndarray:
        """[K, n] alpha vectors -> bool [K, N]: row k = per_image_verdicts(alphas[k]) with fresh draws.  `candidates_per_pass`
        candidates x `batch_images` images x EoT rows go through the engine per call; the encoder runs once per image of a call,
        every (image, candidate, replica) row has its own latent draws, the EoT mean is over each candidate's own replicas."""
        a = alphas.detach().to('cpu', torch.float64) if isinstance(alphas, torch.Tensor) else torch.tensor(np.asarray(alphas), dtype=torch.float64)
        if a.dim() != 2:
            raise ValueError(f'[K, n] alphas expected, got {tuple(a.shape)}')
        a = a * self.alpha_attenuation                       # in double, like `a * alpha_attenuation` on the list (:88)
        cpp = self.default_candidates_per_pass() if candidates_per_pass is None else int(candidates_per_pass)
        if cpp < 1:
            raise ValueError('candidates_per_pass must be at least 1')
        model = self.defense_model.model
        out = np.zeros((a.shape[0], self.images.shape[0]), dtype=bool)
        for k0 in range(0, a.shape[0], cpp):
            cand = a[k0:k0 + cpp]
            for i in range(0, self.images.shape[0], self.batch_images):
                x, y = self.images[i:i + self.batch_images], self.labels[i:i + self.batch_images]
                logits = model.forward_candidates(x, cand, rep=self.eot_steps)            # [B, k, EoT, classes]
                pred = logits.mean(dim=2).argmax(dim=2)                                   # [B, k]
                out[k0:k0 + cand.shape[0], i:i + x.shape[0]] = torch.eq(pred, y.view(-1, 1)).t().cpu().numpy()
        return out

    @torch.no_grad()
    def objective_many(self, alphas, candidates_per_pass: int = None) -> np.ndarray:
        """[K, n] alpha vectors -> float32 [K]: objective_function of every candidate"""
        return self.per_image_verdicts_many(alphas, candidates_per_pass).astype(np.float32).mean(axis=1)


@torch.no_grad()
def random_search(evaluator: AlphaEvaluator, n_steps: int, seed: int = 0, candidates_per_pass: int = None):
    """uniform random alphas, keep all (alphas, accuracy) pairs — grid_search.py:44-72; the candidates are scored
    `candidates_per_pass` at a time (AlphaEvaluator.objective_many)"""
    n = len(evaluator.defense_model.model.interpolation_alphas)
    g = torch.Generator().manual_seed(seed)
    all_alphas = torch.stack([torch.rand(n, generator=g) for _ in range(n_steps)])
    acc = evaluator.objective_many(all_alphas, candidates_per_pass)
    return all_alphas.numpy(), np.asarray(acc, dtype=np.float32).reshape(-1, 1)
