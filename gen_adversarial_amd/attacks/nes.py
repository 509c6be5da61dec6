"""
NES (Ilyas, Engstrom, Athalye & Lin 2018): a score-based black-box attack under the other attacks' protocol
(`attack(image, gt_label, net) -> (success, bound, adv)`).  It never asks the defender for a gradient: per step and image it queries
the logits at x +- sigma * u_i for `pairs` Gaussian directions u_i, estimates

    g = 1 / (2 sigma pairs) * sum_i [L(x + sigma u_i) - L(x - sigma u_i)] * u_i

and takes the PGD step and projection with g.  The figure that stands next to the white-box ones when the question is whether a
stochastic purifier's robustness is obfuscated gradients.  Not in the reference tree; new code.

The directions come from the library's counter-based generator (ga_randn's, include/ga_ops.h) and are never stored:
u_i of image b at step t is the normal of (seed, draw = t, tensor = GA_RANDN_STREAM_NES, row = image_index[b] * pairs + i, element).
Every query is therefore a function of (seed, step, image index, sample) and of x_adv alone: it does not change when finished images
leave the batch, when the queries are cut into other chunks (`query_images`), or when the image is attacked alone, and the CPU
restatement (attacks/nes_ref.py) replays it.  Two backends, one contract: device tensors go through ga_nes_perturb / ga_nes_grad
(csrc/nes.hip; the loss differences and the first rows stay on the device), CPU tensors through nes_ref — so the attack also runs on
the oracle defender and on toy nets.  `net` is only ever called under torch.no_grad(): the defenders serve the queries from their
forward-only engines.
"A function of x_adv" is the whole claim: what a stochastic defender answers to a query is the defender's business (its own draws
depend on how it is called), so trajectories after step 0 are only as repeatable as the defender's noise is.
Images are (B, 3, H, W), as in the other attacks: the per-image norms and steps broadcast over three trailing dimensions.
"""
from __future__ import annotations

import numpy as np
import torch

from ..noise import STREAM_NES
from . import nes_ref
from .pgd import PGDLinf

START_DRAW = 0xFFFFFFFF         # the draw of the random start: no step index reaches it


def _first_rows_device(rows, device) -> torch.Tensor:
    """python first rows -> the unsigned words ga_nes_* read, as an int32 tensor with the same bits"""
    return torch.from_numpy(np.asarray(rows, dtype=np.uint32).view(np.int32).copy()).to(device)


def perturb(x: torch.Tensor, pairs: int, seed: int, draw: int, rows, sigma: float, lo: float = 0.0, hi: float = 1.0,
            tensor: int = STREAM_NES) -> torch.Tensor:
    """x [B, ...] -> the 2 * pairs queries of every image, [B * pairs * 2, ...]: row (b * pairs + i) * 2 + s is
    clamp(x[b] + (s ? -sigma : +sigma) * z(b, i), lo, hi).  `rows`: a device int32 tensor (unsigned bits) for device x, a sequence of
    ints for CPU x — the first row of every image."""
    B, inner = x.shape[0], x[0].numel()
    if x.is_cuda:
        from .. import _lib as L
        if x.dtype != torch.float32 or rows.dtype != torch.int32 or rows.numel() != B or rows.device != x.device:
            raise TypeError('ga_nes_perturb: fp32 images and one int32 first row per image on the same device expected')
        x, rows = x.contiguous(), rows.contiguous()
        y = torch.empty((B * pairs * 2,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
        L.check(L.lib.ga_nes_perturb(x.data_ptr(), y.data_ptr(), B, inner, pairs, seed, draw, tensor, 0, rows.data_ptr(), sigma, lo, hi,
                                     torch.cuda.current_stream(x.device).cuda_stream), 'ga_nes_perturb')
        return y
    y = nes_ref.reference_perturb(x.reshape(B, inner).numpy(), pairs, seed, draw, tensor, image_row=rows, sigma=sigma, lo=lo, hi=hi)
    return torch.from_numpy(y).to(x.dtype).reshape((B * pairs * 2,) + tuple(x.shape[1:]))


def grad(c: torch.Tensor, like: torch.Tensor, pairs: int, seed: int, draw: int, rows, scale: float, tensor: int = STREAM_NES) -> torch.Tensor:
    """c [B * pairs] loss differences -> g shaped like `like` [B, ...]: g[b] = scale * sum_i c[b * pairs + i] * z(b, i)"""
    B, inner = like.shape[0], like[0].numel()
    if like.is_cuda:
        from .. import _lib as L
        c = c.to(torch.float32).contiguous()
        if c.numel() != B * pairs or c.device != like.device or rows.dtype != torch.int32 or rows.numel() != B:
            raise TypeError('ga_nes_grad: one loss difference per pair and one int32 first row per image on the images\' device expected')
        g = torch.empty(like.shape, device=like.device, dtype=torch.float32)
        L.check(L.lib.ga_nes_grad(c.data_ptr(), g.data_ptr(), B, inner, pairs, seed, draw, tensor, 0, rows.contiguous().data_ptr(), scale,
                                  torch.cuda.current_stream(like.device).cuda_stream), 'ga_nes_grad')
        return g
    g = nes_ref.reference_grad(c.double().numpy(), B, inner, pairs, seed, draw, tensor, image_row=rows, scale=scale)
    return torch.from_numpy(g).to(like.dtype).reshape(like.shape)


def margin_loss(logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """max_{j != y} z_j - z_y per row: positive exactly where the row is misclassified"""
    other = logits.scatter(1, y.view(-1, 1), float('-inf')).amax(dim=1)
    return other - logits.gather(1, y.view(-1, 1)).squeeze(1)


class NESAttack:
    batched = True      # `image` may hold several images: each is attacked independently, with its own rows of the generator

    def __init__(self, norm: str = 'Linf', eps: float = 8.0 / 255.0, step_size: float = 2.0 / 255.0, steps: int = 40, pairs: int = 64,
                 sigma: float = 1e-3, loss: str = 'margin', seed: int = 0, query_images: int = None, random_start: bool = False):
        if norm not in ('Linf', 'L2') or loss not in ('margin', 'ce'):
            raise ValueError("norm: 'Linf' or 'L2', loss: 'margin' or 'ce' expected")
        if steps < 0 or steps >= START_DRAW or pairs <= 0 or sigma <= 0 or not 0 <= int(seed) < 1 << 64:
            raise ValueError('0 <= steps < 2^32 - 1, pairs > 0, sigma > 0 and 0 <= seed < 2^64 expected')
        self.norm, self.eps, self.step_size, self.steps, self.pairs, self.sigma = norm, eps, step_size, steps, int(pairs), float(sigma)
        self.loss, self.seed, self.random_start = loss, int(seed), random_start
        self.query_images = query_images    # images per query call of `net` (2 * pairs rows each); None: all active images at once
        self.image_index = None             # tensor [B] of dataset indices: image b draws at rows image_index[b] * pairs + i; None: arange(B)
        self.queries = 0                    # rows `net` was asked for in the last call

    def _loss(self, logits, y):
        return margin_loss(logits, y) if self.loss == 'margin' else torch.nn.functional.cross_entropy(logits, y, reduction='none')

    def _net(self, net, x):
        self.queries += x.shape[0]
        with torch.no_grad():
            return net(x)

    def _project(self, x, x_orig):
        if self.norm == 'Linf':
            return torch.min(torch.max(x, x_orig - self.eps), x_orig + self.eps).clamp(0.0, 1.0)
        d = x - x_orig
        n = d.flatten(1).norm(dim=1).clamp_min(1e-30).view(-1, 1, 1, 1)
        return (x_orig + d * (self.eps / n).clamp(max=1.0)).clamp(0.0, 1.0)     # the clamp moves every pixel towards x_orig: still inside

    def _step(self, x_adv, x_orig, g):
        if self.norm == 'Linf':
            return PGDLinf.step(x_adv, x_orig, g, self.eps, self.step_size)
        n = g.flatten(1).norm(dim=1).clamp_min(1e-30).view(-1, 1, 1, 1)
        return self._project(x_adv + self.step_size * g / n, x_orig)

    def _start(self, x_orig, rows):
        """the random start, from z = sample 0 of every image at START_DRAW (the + row of a perturbation of 0 with sigma 1 is z itself):
        Linf: x + eps * erf(z / sqrt 2), which is uniform in the cube like PGD's start, since erf(z / sqrt 2) is uniform on (-1, 1);
        L2: x + eps * z / |z|, a uniform direction on the sphere; then the projection on [0, 1]"""
        z = perturb(torch.zeros_like(x_orig), 1, self.seed, START_DRAW, rows, 1.0, 1.0, 0.0)[0::2]
        if self.norm == 'Linf':
            return self._project(x_orig + self.eps * torch.erf(z * 0.5 ** 0.5), x_orig)
        return self._project(x_orig + self.eps * z / z.flatten(1).norm(dim=1).view(-1, 1, 1, 1), x_orig)

    def estimate(self, net, x, y, rows, draw: int):
        """the NES estimate of d(loss)/dx at x [B, 3, H, W]: query_images images, 2 * pairs * query_images rows, per call of `net`"""
        B, m = x.shape[0], self.query_images or x.shape[0]
        out = []
        for lo in range(0, B, m):
            xs, ys, rs = x[lo:lo + m], y[lo:lo + m], rows[lo:lo + m]
            loss = self._loss(self._net(net, perturb(xs, self.pairs, self.seed, draw, rs, self.sigma)), ys.repeat_interleave(2 * self.pairs))
            c = loss[0::2] - loss[1::2]
            out.append(grad(c, xs, self.pairs, self.seed, draw, rs, 1.0 / (2.0 * self.sigma * self.pairs)))
        return torch.cat(out)

    def _rows(self, B, device):
        idx = list(range(B)) if self.image_index is None else [int(i) for i in torch.as_tensor(self.image_index).view(-1).tolist()]
        if len(idx) != B:
            raise ValueError(f'image_index names {len(idx)} images, the call has {B}')
        rows = nes_ref.image_rows(B, self.pairs, image_row=[i * self.pairs for i in idx])
        return _first_rows_device(rows, device) if device.type == 'cuda' else torch.tensor(rows, dtype=torch.int64)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, gt_label: torch.Tensor, net):
        x_orig = image.detach()
        B = x_orig.shape[0]
        rows = self._rows(B, x_orig.device)
        self.queries = 0
        x_adv = x_orig.clone()
        if self.random_start:
            x_adv = self._start(x_orig, rows)
        success = torch.zeros(B, dtype=torch.bool, device=x_orig.device)
        best = x_orig.clone()
        act = torch.arange(B, device=x_orig.device)              # the images still attacked: finished ones leave the calls
        for t in range(self.steps + 1):
            wrong = self._net(net, x_adv[act]).argmax(dim=-1) != gt_label[act]        # the check of x_adv itself
            done = act[wrong]
            best[done] = x_adv[done]
            success[done] = True
            act = act[~wrong]
            if act.numel() == 0 or t == self.steps:
                break
            g = self.estimate(net, x_adv[act], gt_label[act], rows[act], t)
            x_adv[act] = self._step(x_adv[act], x_orig[act], g)
        d = (best - x_orig).flatten(1)
        bound = d.abs().amax(dim=1) if self.norm == 'Linf' else d.norm(dim=1)
        if B == 1:
            return bool(success.item()), float(bound.item()), best
        return success, bound, best
