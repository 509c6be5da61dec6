"""
Square Attack (Andriushchenko, Croce, Flammarion & Hein 2020): the score-based black-box random search of AutoAttack's standard
set, under the other attacks' protocol (`attack(image, gt_label, net) -> (success, bound, adv)`).  It asks the defender for no
gradient and estimates none: per iteration and image it proposes one change of the current iterate inside a square window
(L∞: the window set to x ± eps per channel; L2: the authors' bump moved into one window with the budget freed from a second one),
queries the logits of the proposal once, and keeps it where the loss improved.  Not in the reference tree (its AutoAttack notes
"Square Attack is not tested"); this is the project's restatement of the paper, not the authors' RNG stream.

The proposals come from the library's counter-based generator (ga_randn's, include/ga_ops.h): the window positions, channel signs
and bump orientation of image b at iteration t are integer functions of (seed, draw = t, tensor = GA_RANDN_STREAM_SQUARE,
row = image_index[b]).  Every proposal is therefore a function of (seed, iteration, image index) and of x_adv alone: it does not
change when finished images leave the batch or when the image is attacked alone, and the CPU restatement (attacks/square_ref.py)
replays it.  Two backends, one contract: device tensors go through ga_square_linf / ga_square_l2 (csrc/square.hip: one launch per
iteration for all active images, no per-image loop on the host), CPU tensors through square_ref — so the attack also runs on the
oracle defender and on toy nets.  `net` is only ever called under torch.no_grad(): the defenders serve the queries from their
forward-only engines.
"A function of x_adv" is the whole claim: what a stochastic defender answers to a query is the defender's business (its own draws
depend on how it is called), and with its answers the accept decisions, so trajectories after the start are only as repeatable as
the defender's noise is.
Images are (B, C <= 32, H, W); the random start takes its signs from the NES generator's normals and needs C H W % 4 == 0.
"""
from __future__ import annotations

import numpy as np
import torch

from ..noise import STREAM_SQUARE
from . import nes, square_ref
from .nes import START_DRAW, _first_rows_device, margin_loss


def propose(norm: str, x_orig: torch.Tensor, x_adv: torch.Tensor, s: int, seed: int, draw: int, rows, eps: float, table=None,
            lo: float = 0.0, hi: float = 1.0, tensor: int = STREAM_SQUARE) -> torch.Tensor:
    """one proposal per image [B, C, H, W].  `rows`: a device int32 tensor (unsigned bits) for device images, a sequence of ints for
    CPU images — counter word 1 of every image.  `table` (L2): eta(s), on the images' device for device images."""
    B, C, H, W = x_orig.shape
    if x_orig.is_cuda:
        from .. import _lib as L
        if x_orig.dtype != torch.float32 or x_adv.dtype != torch.float32 or x_adv.shape != x_orig.shape or x_adv.device != x_orig.device \
                or rows.dtype != torch.int32 or rows.numel() != B or rows.device != x_orig.device:
            raise TypeError('ga_square_*: fp32 images of one shape and one int32 row per image on the same device expected')
        x_orig, x_adv, rows = x_orig.contiguous(), x_adv.contiguous(), rows.contiguous()
        y = torch.empty_like(x_orig)
        stream = torch.cuda.current_stream(x_orig.device).cuda_stream
        if norm == 'Linf':
            L.check(L.lib.ga_square_linf(x_orig.data_ptr(), x_adv.data_ptr(), y.data_ptr(), B, C, H, W, s, seed, draw, tensor, 0, rows.data_ptr(),
                                         eps, lo, hi, stream), 'ga_square_linf')
        else:
            if table.dtype != torch.float32 or tuple(table.shape) != (s, s) or table.device != x_orig.device:
                raise TypeError('ga_square_l2: the fp32 [s, s] bump table on the images\' device expected')
            L.check(L.lib.ga_square_l2(x_orig.data_ptr(), x_adv.data_ptr(), y.data_ptr(), table.contiguous().data_ptr(), B, C, H, W, s, seed, draw,
                                       tensor, 0, rows.data_ptr(), eps, lo, hi, stream), 'ga_square_l2')
        return y
    rows = [int(r) for r in rows]
    if norm == 'Linf':
        y = square_ref.reference_linf(x_orig.numpy(), x_adv.numpy(), s, seed, draw, tensor, image_row=rows, eps=eps, lo=lo, hi=hi)
    else:
        y = square_ref.reference_l2(x_orig.numpy(), x_adv.numpy(), np.asarray(table), seed, draw, tensor, image_row=rows, eps=eps, lo=lo, hi=hi)
    return torch.from_numpy(y).to(x_orig.dtype)


class SquareAttack:
    batched = True      # `image` may hold several images: each is attacked independently, with its own row of the generator

    def __init__(self, norm: str = 'L2', eps: float = 0.5, n_queries: int = 5000, p_init: float = 0.8, loss: str = 'margin', seed: int = 0):
        if norm not in ('Linf', 'L2') or loss not in ('margin', 'ce'):
            raise ValueError("norm: 'Linf' or 'L2', loss: 'margin' or 'ce' expected")
        if not 1 <= n_queries < START_DRAW or not 0.0 < p_init <= 1.0 or eps <= 0 or not 0 <= int(seed) < 1 << 64:
            raise ValueError('1 <= n_queries < 2^32 - 1, 0 < p_init <= 1, eps > 0 and 0 <= seed < 2^64 expected')
        self.norm, self.eps, self.n_queries, self.p_init, self.loss, self.seed = norm, float(eps), int(n_queries), float(p_init), loss, int(seed)
        self.image_index = None             # tensor [B] of dataset indices: image b draws at row image_index[b]; None: arange(B)
        self.queries = 0                    # rows `net` was asked for in the last call
        self._tables = {}                   # (side, device) -> eta(side)

    def _loss(self, logits, y):
        return margin_loss(logits, y) if self.loss == 'margin' else torch.nn.functional.cross_entropy(logits, y, reduction='none')

    def _net(self, net, x):
        self.queries += x.shape[0]
        with torch.no_grad():
            return net(x)

    def _rows(self, B, device):
        idx = list(range(B)) if self.image_index is None else [int(i) for i in torch.as_tensor(self.image_index).view(-1).tolist()]
        if len(idx) != B:
            raise ValueError(f'image_index names {len(idx)} images, the call has {B}')
        rows = square_ref.image_rows(B, image_row=idx)
        return _first_rows_device(rows, device) if device.type == 'cuda' else torch.tensor(rows, dtype=torch.int64)

    def _table(self, s, like):
        """eta(s) as a tensor on `like`'s device: fp32 for the device kernel, the same values in `like`'s dtype on the CPU"""
        key = (s, like.device, like.dtype)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(square_ref.eta(s)).to(device=like.device, dtype=like.dtype)
        return self._tables[key]

    def _start(self, x_orig, rows):
        """the starting point, from z = the one NES sample of every image at START_DRAW (the + row of a perturbation of 0 with sigma 1
        is z itself), batch-wide: Linf: vertical stripes x + eps * sign(z[b, ch, 0, w]); L2: the image tiled from its top-left corner
        with eta(s0) bumps, s0 = max(2, min(H, W) // 5), the tile at (i, j) signed by sign(z[b, ch, i * s0, j * s0]), scaled to norm
        eps; then the clamp to [0, 1]"""
        z = nes.perturb(torch.zeros_like(x_orig), 1, self.seed, START_DRAW, rows, 1.0, 1.0, 0.0, tensor=STREAM_SQUARE)[0::2]
        sign = torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
        if self.norm == 'Linf':
            return (x_orig + self.eps * sign[:, :, :1, :]).clamp(0.0, 1.0)
        H, W = x_orig.shape[2:]
        s0 = max(2, min(H, W) // 5)
        th, tw = H // s0, W // s0
        tiles = sign[:, :, 0:th * s0:s0, 0:tw * s0:s0].repeat_interleave(s0, dim=2).repeat_interleave(s0, dim=3)
        d = torch.zeros_like(x_orig)
        d[:, :, :th * s0, :tw * s0] = tiles * self._table(s0, x_orig).repeat(th, tw)
        n = d.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
        return (x_orig + d * (self.eps / n)).clamp(0.0, 1.0)

    def side(self, it: int, H: int, W: int) -> int:
        return square_ref.side(square_ref.p_schedule(self.p_init, it, self.n_queries), H, W, self.norm)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, gt_label: torch.Tensor, net):
        x_orig = image.detach()
        B, _, H, W = x_orig.shape
        gt_label = gt_label.view(-1)
        rows = self._rows(B, x_orig.device)
        self.queries = 0
        x_adv = self._start(x_orig, rows)
        logits = self._net(net, x_adv)                              # the starting loss: query 1 of n_queries
        loss_best = self._loss(logits, gt_label).clone()
        act = (logits.argmax(dim=-1) == gt_label).nonzero().flatten()          # the images still attacked: finished ones leave the calls
        for it in range(self.n_queries - 1):
            if act.numel() == 0:
                break
            s = self.side(it, H, W)
            table = self._table(s, x_orig) if self.norm == 'L2' else None
            y = propose(self.norm, x_orig[act], x_adv[act], s, self.seed, it, rows[act], self.eps, table)
            logits = self._net(net, y)
            loss = self._loss(logits, gt_label[act])
            wrong = logits.argmax(dim=-1) != gt_label[act]
            take = (loss > loss_best[act]) | wrong                  # the authors' rule: improved, or misclassified
            idx = act[take]
            x_adv[idx] = y[take]
            loss_best[idx] = loss[take]
            act = act[~wrong]                                       # misclassified images leave and keep that iterate
        success = torch.ones(B, dtype=torch.bool, device=x_orig.device)
        success[act] = False
        best = torch.where(success.view(-1, 1, 1, 1), x_adv, x_orig)
        d = (best - x_orig).flatten(1)
        bound = d.abs().amax(dim=1) if self.norm == 'Linf' else d.norm(dim=1)
        if B == 1:
            return bool(success.item()), float(bound.item()), best
        return success, bound, best
