"""
CPU restatement of ga_square_linf / ga_square_l2 (include/ga_ops.h, csrc/square.hip) and of the schedules of Square Attack
(Andriushchenko, Croce, Flammarion & Hein 2020), on top of noise.philox4x32_10.

This is the project's restatement of the paper: the reference tree has no Square Attack to pin it against (its AutoAttack says
"Square Attack is not tested"), and the random choices are this library's counter-based stream, not the authors' RNG stream — so
trajectories are comparable with the authors' code in distribution only.

The choices of image b at draw t are integers (host and device agree bit for bit):
  Wd = philox(0, image_row[b], tensor, t), Vd = philox(1, image_row[b], tensor, t) under the key of `seed`;
  pos(word, n) = (word * n) >> 32;  window 1 at (pos(Wd0, H - s + 1), pos(Wd1, W - s + 1)), window 2 (L2) at the same of Vd0, Vd1;
  sign[ch] = + where bit ch of Wd2 is set;  the L2 bump is transposed where bit 0 of Wd3 is set.
image_row = None means image_row[b] = row0 + b.
reference_linf works in the dtype of its images (one addition per rewritten element: fp32 in, the kernel's bits out);
reference_l2 works in float64.  numpy only, like noise.py: the CPU backend of attacks.square.SquareAttack, and the reference the
kernels are tested against.
"""
from __future__ import annotations

import math

import numpy as np

from ..noise import STREAM_SQUARE, philox4x32_10

MAX_CHANNELS = 32            # one sign bit per channel


def image_rows(images: int, row0: int = 0, image_row=None) -> list:
    """counter word 1 of every image; refuses what the library refuses (a row past 2^32)"""
    if images <= 0:
        raise ValueError('images > 0 expected')
    rows = [int(row0) + b for b in range(images)] if image_row is None else [int(r) for r in image_row]
    if len(rows) != images or min(rows) < 0 or max(rows) >= 1 << 32:
        raise ValueError('one row per image, 0 <= image_row[b] < 2^32 expected')
    return rows


def windows(images: int, H: int, W: int, s: int, seed: int, draw: int, tensor: int = STREAM_SQUARE, row0: int = 0, image_row=None) -> dict:
    """the choices of every image: int arrays h1, w1, h2, w2 [images], uint32 `signs` (bit ch), bool `transposed`"""
    if not 1 <= s <= min(H, W):
        raise ValueError('1 <= s <= min(H, W) expected')
    rows = image_rows(images, row0, image_row)
    c = np.empty((2, images, 4), dtype=np.uint64)
    c[0, :, 0], c[1, :, 0] = 0, 1
    c[:, :, 1] = np.asarray(rows, dtype=np.uint64)[None, :]
    c[:, :, 2] = int(tensor) & 0xFFFFFFFF
    c[:, :, 3] = int(draw) & 0xFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)

    def pos(word, n):
        return ((word * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    return {'h1': pos(x[0, :, 0], H - s + 1), 'w1': pos(x[0, :, 1], W - s + 1), 'h2': pos(x[1, :, 0], H - s + 1), 'w2': pos(x[1, :, 1], W - s + 1),
            'signs': x[0, :, 2].astype(np.uint32), 'transposed': (x[0, :, 3] & np.uint64(1)).astype(bool)}


def channel_signs(word: int, C: int, dtype=np.float64) -> np.ndarray:
    """[C] of +1 / -1 from the bits of `word`"""
    return np.array([1.0 if (int(word) >> ch) & 1 else -1.0 for ch in range(C)], dtype=dtype)


def _images(x_orig, x_adv, dtype=None):
    x_orig, x_adv = np.asarray(x_orig, dtype=dtype), np.asarray(x_adv, dtype=dtype)
    if x_orig.ndim != 4 or x_orig.shape != x_adv.shape or x_orig.shape[1] > MAX_CHANNELS:
        raise ValueError('x_orig, x_adv: [images, C <= 32, H, W] of one shape expected')
    return x_orig, x_adv


def reference_linf(x_orig, x_adv, s: int, seed: int, draw: int, tensor: int = STREAM_SQUARE, row0: int = 0, image_row=None,
                   eps: float = 8.0 / 255.0, lo: float = 0.0, hi: float = 1.0) -> np.ndarray:
    """y = x_adv outside window 1, clamp(x_orig +- eps, lo, hi) inside, one sign per channel; in the images' dtype.  lo > hi: no clamp"""
    x_orig, x_adv = _images(x_orig, x_adv)
    B, C, H, W = x_orig.shape
    dt = x_orig.dtype.type
    win = windows(B, H, W, s, seed, draw, tensor, row0, image_row)
    y = x_adv.copy()
    for b in range(B):
        h, w = int(win['h1'][b]), int(win['w1'][b])
        sg = channel_signs(win['signs'][b], C, x_orig.dtype)[:, None, None]
        v = x_orig[b, :, h:h + s, w:w + s] + sg * dt(eps)
        y[b, :, h:h + s, w:w + s] = np.clip(v, dt(lo), dt(hi)) if lo <= hi else v
    return y


def reference_l2(x_orig, x_adv, table, seed: int, draw: int, tensor: int = STREAM_SQUARE, row0: int = 0, image_row=None, eps: float = 0.5,
                 lo: float = 0.0, hi: float = 1.0, parts: list = None) -> np.ndarray:
    """the L2 proposal in float64 (ga_ops.h has the formulas); `table` is eta(s) as the device holds it.  Per image: an image's
    result is the same alone or in a batch.  `parts`, when a list, receives one dict of intermediates per image."""
    x_orig, x_adv = _images(x_orig, x_adv, np.float64)
    B, C, H, W = x_orig.shape
    table = np.asarray(table, dtype=np.float64)
    s = table.shape[0]
    if table.shape != (s, s):
        raise ValueError('table: [s, s] expected')
    win = windows(B, H, W, s, seed, draw, tensor, row0, image_row)
    eps = float(eps)
    y = np.empty_like(x_orig)
    for b in range(B):
        h1, w1, h2, w2 = (int(win[k][b]) for k in ('h1', 'w1', 'h2', 'w2'))
        d = x_adv[b] - x_orig[b]
        union = np.zeros((H, W), dtype=bool)
        union[h1:h1 + s, w1:w1 + s] = True
        union[h2:h2 + s, w2:w2 + s] = True
        n_img2 = float((d ** 2).sum())
        n_win2 = (d ** 2)[:, union].sum(axis=1)                                         # [C]
        d1 = d[:, h1:h1 + s, w1:w1 + s]
        n_1 = math.sqrt(float((d1 ** 2).sum()))
        bump = table.T if win['transposed'][b] else table
        old = d1 / (1e-12 + n_1)
        new = channel_signs(win['signs'][b], C)[:, None, None] * bump[None] + old       # [C, s, s]
        n_new = np.sqrt((new ** 2).sum(axis=(1, 2)))
        target = np.sqrt(max(eps * eps - n_img2, 0.0) / C + n_win2)
        scale = target / (1e-12 + n_new)
        d2 = d.copy()
        d2[:, h2:h2 + s, w2:w2 + s] = 0.0
        d2[:, h1:h1 + s, w1:w1 + s] = scale[:, None, None] * new
        n_d2 = math.sqrt(float((d2 ** 2).sum()))
        f = eps / (1e-12 + n_d2)
        v = x_orig[b] + d2 * f
        y[b] = np.clip(v, lo, hi) if lo <= hi else v
        if parts is not None:
            parts.append({'h1': h1, 'w1': w1, 'h2': h2, 'w2': w2, 'union': union, 'd': d, 'n_img2': n_img2, 'n_win2': n_win2, 'n_1': n_1,
                          'old': old, 'new': new, 'n_new': n_new, 'target': target, 'scale': scale, 'd2': d2, 'n_d2': n_d2, 'f': f})
    return y


def _eta_rectangles(x: int, y: int) -> np.ndarray:
    """a normalised sum of centred nested rectangles weighted 1 / (k + 1)^2, [x, y]"""
    delta = np.zeros((x, y))
    xc, yc = x // 2 + 1, y // 2 + 1
    r0, r1 = xc - 1, yc - 1
    for k in range(max(xc, yc)):
        delta[max(r0, 0):min(r0 + 2 * k + 1, x), max(r1, 0):min(r1 + 2 * k + 1, y)] += 1.0 / (k + 1) ** 2
        r0, r1 = r0 - 1, r1 - 1
    return delta / np.sqrt((delta ** 2).sum())


def eta(s: int) -> np.ndarray:
    """the authors' "meta pseudo-Gaussian" bump [s, s]: the upper s // 2 rows a positive hill, the lower rows a negative one, unit L2
    norm; computed in float64, stored fp32 (the table the device reads)"""
    if s < 2:
        raise ValueError('s >= 2 expected')
    delta = np.zeros((s, s))
    delta[:s // 2] = _eta_rectangles(s // 2, s)
    delta[s // 2:] = -_eta_rectangles(s - s // 2, s)
    return (delta / np.sqrt((delta ** 2).sum())).astype(np.float32)


def side(p: float, H: int, W: int, norm: str) -> int:
    """the window side for the fraction p of the pixels: round(sqrt(p H W)), at least 1 and at most min(H, W); for L2 at least 3,
    odd, and at most min(H, W) - 1 made odd"""
    s = max(int(round(math.sqrt(p * H * W))), 1)
    if norm == 'Linf':
        return min(s, H, W)
    if min(H, W) < 4:
        raise ValueError('L2 windows need images of at least 4 x 4')
    s = max(s, 3)
    s += 1 - s % 2
    cap = min(H, W) - 1
    return min(s, cap - (1 - cap % 2))


def p_schedule(p_init: float, it: int, n_iters: int) -> float:
    """the authors' piecewise halving of p, its break points (of 10,000 iterations) rescaled to n_iters"""
    it = int(it / n_iters * 10000)
    for k, edge in enumerate((10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)):
        if it <= edge:
            return p_init / 2 ** k
    return p_init / 512
