"""
CPU restatement of ga_nes_perturb / ga_nes_grad (include/ga_ops.h, csrc/nes.hip) on top of noise.reference_randn, in float64.

The direction of sample i of image b is z(b, i, e) = the ga_randn normal (scale 1) of (seed, draw, tensor, row = image_row[b] + i,
element e); image_row = None means image_row[b] = row0 + b * pairs.
  perturb:  y[(b * pairs + i) * 2 + s, e] = clamp(x[b, e] + (s ? -sigma : +sigma) * z(b, i, e), lo, hi);  lo > hi: no clamp
  grad:     g[b, e] = scale * sum_i c[b * pairs + i] * z(b, i, e)
numpy only, like noise.py: the CPU backend of attacks.nes.NESAttack, and the reference the kernels are tested against.
"""
from __future__ import annotations

import numpy as np

from ..noise import STREAM_NES, reference_randn


def image_rows(images: int, pairs: int, row0: int = 0, image_row=None) -> list:
    """first row of every image; refuses what the library refuses (a row past 2^32)"""
    if images <= 0 or pairs <= 0:
        raise ValueError('images > 0 and pairs > 0 expected')
    rows = [int(row0) + b * pairs for b in range(images)] if image_row is None else [int(r) for r in image_row]
    if len(rows) != images or min(rows) < 0 or max(rows) + pairs > 1 << 32:
        raise ValueError('one first row per image, 0 <= image_row[b] and image_row[b] + pairs <= 2^32 expected')
    return rows


def directions(images: int, inner: int, pairs: int, seed: int, draw: int, tensor: int = STREAM_NES, row0: int = 0,
               image_row=None) -> np.ndarray:
    """z as float64 [images, pairs, inner]"""
    rows = image_rows(images, pairs, row0, image_row)
    return np.stack([reference_randn(seed, draw, tensor, r, pairs, inner) for r in rows])


def reference_perturb(x, pairs: int, seed: int, draw: int, tensor: int = STREAM_NES, row0: int = 0, image_row=None, sigma: float = 1e-3,
                      lo: float = 1.0, hi: float = 0.0) -> np.ndarray:
    """x [images, inner] -> float64 [images * pairs * 2, inner]"""
    x = np.asarray(x, dtype=np.float64)
    images, inner = x.shape
    z = directions(images, inner, pairs, seed, draw, tensor, row0, image_row)
    y = np.stack([x[:, None, :] + float(sigma) * z, x[:, None, :] - float(sigma) * z], axis=2)       # [images, pairs, 2, inner]
    if lo <= hi:
        y = np.clip(y, lo, hi)
    return y.reshape(images * pairs * 2, inner)


def reference_grad(c, images: int, inner: int, pairs: int, seed: int, draw: int, tensor: int = STREAM_NES, row0: int = 0, image_row=None,
                   scale: float = 1.0) -> np.ndarray:
    """c [images * pairs] -> float64 [images, inner]"""
    c = np.asarray(c, dtype=np.float64).reshape(images, pairs)
    z = directions(images, inner, pairs, seed, draw, tensor, row0, image_row)
    return float(scale) * np.stack([c[b] @ z[b] for b in range(images)])     # per image: the same sum alone or in a batch
