"""
CPU restatement of ga_randn (include/ga_ops.h, csrc/randn.hip): the same integers, evaluated in float64.

The value of element e of absolute row R of tensor `stream` at draw `draw` under `seed` is a pure function of
(seed, draw, stream, R, e):
  Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) on the counter (e // 4, R mod 2^32, stream, draw) gives four words
  x0..x3 for elements 4q .. 4q+3;  u_k = ((x_k >> 9) + 0.5) * 2^-23;  Box-Muller on (u0, u1) and (u2, u3):
  z_2j = sqrt(-2 ln u_2j) cos(2 pi u_2j+1),  z_2j+1 = sqrt(-2 ln u_2j) sin(2 pi u_2j+1).
Nothing here touches torch or the GPU: numpy only, so that any box can say "seed 7, draw 12" and get the numbers.
"""
from __future__ import annotations

import numpy as np

STREAM_INPUT = 2147483648          # GA_RANDN_STREAM_INPUT: the input noise; latent group i draws with stream = i
STREAM_NES = 2147483649            # GA_RANDN_STREAM_NES: the directions of the NES attack (attacks/nes_ref.py)
STREAM_SQUARE = 2147483650         # GA_RANDN_STREAM_SQUARE: the windows, signs and orientations of Square Attack (attacks/square_ref.py)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """counter: [..., 4] 32-bit words, key: [2] words -> uint32 [..., 4].  uint64 arithmetic: a 32 x 32 product fits."""
    c = np.asarray(counter, dtype=np.uint64)
    if c.shape[-1] != 4:
        raise ValueError('counter: [..., 4] words expected')
    c0, c1, c2, c3 = (c[..., i] & _MASK for i in range(4))
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def reference_bits(seed: int, draw: int, stream: int, row0: int, rows: int, inner: int) -> np.ndarray:
    """uint32 [rows, inner]: the words ga_randn stores with mode = 1"""
    if inner % 4 or inner <= 0 or rows <= 0 or row0 < 0 or row0 + rows > 1 << 32:
        raise ValueError('rows > 0, inner % 4 == 0 and row0 + rows <= 2^32 expected')
    quads = inner // 4
    c = np.empty((rows, quads, 4), dtype=np.uint64)
    c[..., 0] = np.arange(quads, dtype=np.uint64)[None, :]
    c[..., 1] = ((np.arange(rows, dtype=np.uint64) + np.uint64(row0)) & _MASK)[:, None]
    c[..., 2] = np.uint64(int(stream) & 0xFFFFFFFF)
    c[..., 3] = np.uint64(int(draw) & 0xFFFFFFFF)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32)).reshape(rows, inner)


def reference_uniforms(bits: np.ndarray) -> np.ndarray:
    """float64 uniforms of the words: ((x >> 9) + 0.5) * 2^-23, strictly inside (0, 1)"""
    return ((np.asarray(bits, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def reference_randn(seed: int, draw: int, stream: int, row0: int, rows: int, inner: int, scale: float = 1.0,
                    dtype=np.float64) -> np.ndarray:
    """[rows, inner] of scale * z, computed in float64 and cast to `dtype` at the end"""
    u = reference_uniforms(reference_bits(seed, draw, stream, row0, rows, inner)).reshape(rows, inner // 2, 2)
    rad = np.sqrt(-2.0 * np.log(u[..., 0]))
    ang = 2.0 * np.pi * u[..., 1]
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(rows, inner)
    return (float(scale) * z).astype(dtype)
