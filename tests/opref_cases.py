"""
Seeded inputs of the op-level edge tests that contain a kink (ReLU / LeakyReLU / PReLU at 0, clamp bounds, max-pool ties).
tests/test_ops_edges_gpu.py and tests/test_ops_edges2_gpu.py run the kernels on them; tests/test_opref_cpu.py asserts, with
the float64 reference alone, that no more than opref.KINK_CAP of each case's decisions lie within opref.KINK_REL of a tie, so
the share a GPU test may leave out of a gradient comparison is bounded before any kernel runs.  All tensors are fp32 CPU
tensors.
"""
import torch

import opref as R


def g(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen) * scale


def u(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def se_case():
    """ga_se_excite fused backward: K = 3 cotangents per forward row, N = 6, P = 5 x 7, C = 132, Hd = 16"""
    K, N, P, C, Hd = 3, 6, 35, 132, 16
    return dict(K=K, N=N, P=P, C=C, Hd=Hd, res_scale=float(torch.tensor(0.1)), t=g(N // K, P, C, seed=1), dout=g(N, P, C, seed=2),
                w1=g(Hd, C, seed=3, scale=0.3), b1=g(Hd, seed=4), w2=g(C, Hd, seed=5, scale=0.5), b2=g(C, seed=6))


def dml_case():
    K, N, H, W, nmix, ld = 3, 6, 6, 10, 10, 100
    return dict(K=K, N=N, H=H, W=W, nmix=nmix, ld=ld, logits=g(N // K, H, W, ld, seed=1, scale=1.5),
                dimg_nhwc=g(N, H, W, 3, seed=2), dimg_nchw=g(N, 3, H, W, seed=3))


def maxpool_case(N=6, K=3, H=6, W=10, C=12):
    x = g(N // K, H, W, C, seed=1)
    x[0, 0, 0, 0] = x[0, 0, 1, 0] = x[0, 1, 0, 0] = 5.0            # three-way tie: the first in scan order wins
    x[1, 2, 3, 5] = x[1, 3, 3, 5] = 4.0                            # tie between (0, 1) and (1, 1) of a window
    x[1, 4:6, 8:10, 7] = 3.0                                       # a constant window
    return dict(K=K, x=x, dy=g(N, H // 2, W // 2, C, seed=2))


def interleave_case():
    K, N, H, W, C = 3, 6, 6, 10, 12
    return dict(K=K, N=N, H=H, W=W, C=C, planes=g(N, H // 2, W // 2, 4 * C, seed=1), dact_x=g(N // K, H, W, C, seed=2),
                slope=u(C, seed=3) - 0.3, scale=u(C, seed=4) + 0.5, shift=g(C, seed=5, scale=0.3),
                addend=g(N, H, W, C, seed=6), addend2=g(N, H, W, C, seed=7))


def image_case():
    """2 images, rep = 2, K = 3: N = 12 cotangent rows; noise of unit scale on images in [0, 1]: about a third of the pixels
    clamp on each side"""
    B, rep, K, C, H, W = 2, 2, 3, 3, 6, 10
    return dict(B=B, rep=rep, K=K, C=C, H=H, W=W, x=u(B, C, H, W, seed=1), noise=g(B * rep, C, H, W, seed=2),
                coef=torch.tensor([0.9, 1.0, 1.1, 1.2]), dy=g(B * rep * K, H, W, C, seed=3))


ADAIN_SHAPES = [(3, 35, 36, True), (3, 35, 36, False), (2, 1024, 8, True)]


def adain_case(N, P, C, noisy, offset=0.0):
    """offset: a per-channel constant of `offset` standard deviations (alternating sign) added to x"""
    x = g(N, P, C, seed=1)
    if offset:
        x = x + offset * (1 - 2 * (torch.arange(C) % 2)).float() * (1 + 0.1 * u(C, seed=9))
    return dict(x=x, noise=g(N, P, seed=2) if noisy else None, wn=g(C, seed=3, scale=0.5) if noisy else None,
                style=torch.cat([u(N, C, seed=4) + 0.5, g(N, C, seed=5)], dim=1), dy=g(N, P, C, seed=6))


def sample_case():
    N, P, C = 3, 35, 6
    return dict(t=g(N, P, 2 * C, seed=1), eps=g(N, C, P, seed=2), f0=float(torch.tensor(0.7)), dz=g(N, P, C, seed=3))


def prelu_case():
    rows, C = 37, 12
    x = g(rows, C, seed=1)
    x[0, :4] = 0.0
    x[36, 8:] = 0.0
    x[17, 5] = -0.0
    return dict(x=x, slope=u(C, seed=2) - 0.3, dy=g(rows, C, seed=3))


def modout_case(P=35):
    N, C = 3, 12
    return dict(t=g(N, P, C, seed=1), scale=1.0 + 0.2 * g(N, C, seed=2), add=g(P, C, seed=3), dout=g(N, P, C, seed=4))


GCONV_WINDOWS = [(1, 1), (1, 2), (2, 1), (2, 2)]
GCONV_ANCHORED_CG = [4, 12]


def gconv_anchored_case(cg, KH, KW):
    """ga_gconv as a sub-kernel of a stride-2 transpose: window anchored at the output pixel (pad 0, Ho = Hi), G = 3 groups,
    N = 6 cotangent rows of 9 x 11 pixels (594 pixels: the third workgroup is ragged) on 2 rows of the ReLU' source"""
    K, N, H, W, G = 3, 6, 9, 11, 3
    C = G * cg
    return dict(K=K, N=N, H=H, W=W, G=G, C=C, x=g(N, H, W, C, seed=1), w=g(C, KH * KW * cg, seed=2, scale=(KH * KW * cg) ** -0.5),
                dact_x=g(N // K, H, W, C, seed=3))


AVGPOOL_SHAPES = [(1, 4), (15, 72), (49, 132)]


def avgpool_case(P, C):
    N = 3
    return dict(x=g(N, P, C, seed=1), dy=g(N, C, seed=2))


def kink_sites():
    """(name, pre-activation in float64, kink positions) of every seeded case above"""
    out = []
    for cg in GCONV_ANCHORED_CG:
        for KH, KW in GCONV_WINDOWS:
            out.append((f'gconv act\' cg={cg} {KH}x{KW}', R.f64(gconv_anchored_case(cg, KH, KW)['dact_x']), (0.0,)))
    for P, C in AVGPOOL_SHAPES:
        out.append((f'avgpool_act act\' P={P} C={C}', R.f64(avgpool_case(P, C)['x']), (0.0,)))
    s = se_case()
    t, w1, b1 = R.f64(s['t'], s['w1'], s['b1'])
    out.append(('se_excite hid', t.mean(dim=1) @ w1.t() + b1, (0.0,)))
    d = dml_case()
    out.append(('dml clamps', R.dml_pre(R.f64(d['logits']), d['nmix']), (-1.0, 1.0)))
    il = interleave_case()
    out.append(('interleave2 prelu', R.f64(il['dact_x']), (0.0,)))
    im = image_case()
    out.append(('image_io clamp', R.image_pre(*R.f64(im['x'], im['noise'], im['coef']), im['rep']), (0.0, 1.0)))
    for shp in ADAIN_SHAPES:
        for off in (0.0, 8.0):
            a = adain_case(*shp, offset=off)
            out.append((f'adain {shp} offset {off}', R.avae_adain_pre(*R.f64(a['x'], a['noise'], a['wn'])), (0.0,)))
    out.append(('avae sample', R.f64(sample_case()['t']), (0.0,)))
    for P in (35, 700):
        m = modout_case(P)
        out.append((f'modout P={P}', R.modout_u(*R.f64(m['t'], m['scale'], m['add'])), (0.0,)))
    return out
