"""
The index maps of ga_dwconv5's two collapsed forms, pinned in float64 without the library (gen_adversarial_amd/csrc/dwconv5.hip
builds the same tables per workgroup):
  forward : dw5(nearest_x2(x)) is four 3x3 filters on x padded by 1, one per output parity (a, b); tap (kh, kw) of the 5x5
            lands on source offset ((a + kh) >> 1, (b + kw) >> 1)
  adjoint : pool2_sum(dw5(dy)) is one 6x6 stride-2 filter on dy padded by 2, w6[r][s] = sum_{a,b in {0,1}} w[r - a][s - b]
Random asymmetric taps on non-square 3 x 5 sources; both identities to 1e-12 (measured 4e-15).
"""
import torch
import torch.nn.functional as F

import opref as R

TOL = 1e-12
N, HS, WS, C = 2, 3, 5, 4


def d(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def parity_filters(w):
    """w [25][C] -> w3 [2][2][3][3][C]"""
    w5 = w.view(5, 5, -1)
    w3 = torch.zeros(2, 2, 3, 3, w5.shape[-1], dtype=w.dtype)
    for a in range(2):
        for b in range(2):
            for kh in range(5):
                for kw in range(5):
                    w3[a, b, (a + kh) >> 1, (b + kw) >> 1] += w5[kh, kw]
    return w3


def pooled_filter(w):
    """w [25][C] -> w6 [6][6][C]"""
    w5 = w.view(5, 5, -1)
    w6 = torch.zeros(6, 6, w5.shape[-1], dtype=w.dtype)
    for a in range(2):
        for b in range(2):
            w6[a:a + 5, b:b + 5] += w5
    return w6


def test_up2_forward_is_four_3x3_filters_on_the_source():
    x, w = d(N, HS, WS, C, seed=1), d(25, C, seed=2, scale=0.2)
    ref = R.dwconv5(x, w, up2=True)
    w3 = parity_filters(w)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(N, 2 * HS, 2 * WS, C, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            acc = torch.zeros(N, HS, WS, C, dtype=torch.float64)
            for r in range(3):
                for s in range(3):
                    acc = acc + w3[a, b, r, s] * xp[:, r:r + HS, s:s + WS]
            y[:, a::2, b::2] = acc
    err = (y - ref).abs().max().item()
    print(f'forward identity: {err:.3e}')
    assert err <= TOL


def test_pool2_adjoint_is_one_6x6_stride_2_filter_on_dy():
    dy, w = d(N, 2 * HS, 2 * WS, C, seed=3), d(25, C, seed=4, scale=0.2)
    ref = R.dwconv5(dy, w, pool2=True)
    w6 = pooled_filter(w)
    dp = F.pad(dy, (0, 0, 2, 2, 2, 2))
    y = torch.zeros(N, HS, WS, C, dtype=torch.float64)
    for r in range(6):
        for s in range(6):
            y = y + w6[r, s] * dp[:, r:r + 2 * HS:2, s:s + 2 * WS:2]
    err = (y - ref).abs().max().item()
    print(f'adjoint identity: {err:.3e}')
    assert err <= TOL
