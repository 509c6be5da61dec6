"""
The second float64 sweep: ga_attn, ga_layernorm, ga_resize2_crop, ga_gconv, ga_gauss_blur, ga_rowchan_reduce and ga_avgpool_act
against tests/opref.py (written from include/ga_ops.h), at the shapes where their index arithmetic is not trivially right.
Conventions and tolerances are those of tests/test_ops_edges_gpu.py (whose Out / launch / near / exact are used as they are):
outputs start as NaN with one trailing sentinel row, pad channels under a pitch hold the sentinel and must keep it, selections
and copies are compared for equality, everything else may differ from float64 by at most opref.bound() = 4 x the error of the
same formula in fp32 on the CPU (floor 2^-22 of max |ref|).  For the long sums -- P V and dS K over Tk keys, the reductions
over P >= 4095 pixels -- that fp32 CPU formula adds in the order the kernels' comments document (opref.weighted_rows_in_groups,
opref.lane_sum / segment_sum: strided partial sums per lane or key group, then the tree, lane or segment order), because
PyTorch's pairwise sum can beat a correct fixed-order kernel; it is never the kernel's own output.  The blur reference adds its
taps in tap order as it stands.  Every other yardstick is the plain formula.  The two capped-grid cases of this sweep
(resize2_crop, gconv's generic kernel) are in test_ops_edges_gpu.py::test_second_trip_of_the_capped_grid.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

import opref as R   # noqa: E402
import opref_cases as CS   # noqa: E402
from gen_adversarial_amd import _lib as L   # noqa: E402
from test_ops_edges_gpu import SENT, Out, dev, exact, f32, launch, near   # noqa: E402
from test_ops_gpu import g   # noqa: E402


def padded(*shape, used):
    """an Out whose channels [0, used) start as NaN and whose pad channels hold the sentinel"""
    o = Out(*shape)
    o.t[..., used:] = SENT
    return o


def split(o, used):
    """the written channels of a finished pitched output; the pad channels must still hold the sentinel"""
    t = o.done()
    assert bool((t[..., used:] == SENT).all()), 'pad channels were written'
    return t[..., :used]


def untouched(*outs):
    torch.cuda.synchronize()
    for o in outs:
        t = o.done()
        assert bool((torch.isnan(t) | (t == SENT)).all()), 'a refused call wrote its output'


# =====================================================================================================================
# ga_attn
# =====================================================================================================================
def _attn_inputs(dh, heads, Tk, qscale=1.0):
    N, Tq, E = 2, 16, heads * dh
    return g(N, Tq, E, seed=1) * qscale, g(N, Tk, E, seed=2), g(N, Tk, E, seed=3), g(N, Tq, E, seed=4)


def _attn_run(q, k, v, dout, heads, dh, scale):
    """forward and backward with ldq = E + 4, ldo = E + 8, lddq = E + 4; k | v and dk | dv are the halves of one 2E + 8 wide tensor"""
    N, Tq, E = q.shape
    Tk, ldq, ldo, ldkv = k.shape[1], E + 4, E + 8, 2 * E + 8
    kv = torch.full((N, Tk, ldkv), SENT)
    kv[..., :E], kv[..., E:2 * E] = k, v
    kvd = dev(kv)
    out, p = padded(N, Tq, ldo, used=E), Out(N, heads, Tq, Tk)
    io = dict(q=dev(R.pitched(q, ldq, SENT)), k=kvd, v=kvd.data_ptr() + 4 * E, p=p, ldq=ldq, ldk=ldkv, ldv=ldkv, ldo=ldo,
              N=N, Tq=Tq, Tk=Tk, heads=heads, dh=dh, scale=scale)
    launch(L.AttnDesc, out=out, **io)
    ds, dq, dkv = Out(N, heads, Tq, Tk), padded(N, Tq, ldq, used=E), padded(N, Tk, ldkv, used=2 * E)
    launch(L.AttnDesc, dout=dev(R.pitched(dout, ldo, SENT)), ds=ds, dq=dq, dk=dkv, dv=dkv.t.data_ptr() + 4 * E, lddq=ldq, lddk=ldkv,
           lddv=ldkv, backward=1, **io)
    ds.done()
    dkdv = split(dkv, 2 * E)
    return split(out, E), p.done(), split(dq, E), dkdv[..., :E], dkdv[..., E:]


ATTN_CASES = [(16, 3, 257, 1.0), (48, 1, 300, 1.0), (80, 3, 5, 1.0), (112, 1, 257, 1.0), (112, 3, 300, 1.0), (128, 3, 300, 1.0),
              (128, 1, 5, 1.0), (80, 3, 300, 30.0)]


@pytest.mark.parametrize('dh,heads,Tk,qscale', ATTN_CASES)
def test_attn(dh, heads, Tk, qscale):
    """N = 2 rows, forward and backward.  Paths: dh = 48, 80, 112 leave 256 - G * dh / 4 = 4, 16, 4 threads of attn_weighted_rows
    idle (G = 21, 12, 9 key groups) and stride its LDS buffer by a dh that is no power of two; Tk = 257 and 300 give thread 0 (0 ..
    43) a second key; Tk = 5 leaves all but 5 threads without a key and most key groups empty; heads = 1 and 3; every pitch wider
    than E.  (80, 3, 300, 30.0) scales q by 30: the scores spread over more than 30 and pass 89, so expf overflows without the
    max subtraction.  Yardstick: out and dq add their keys in the kernel's group order, the rest is the plain formula.
    fp32-CPU err / bound / kernel err: (16, 3, 257) out 2.1e-7 / 8.2e-7 / 1.5e-7, dq 1.7e-7 / 6.6e-7 / 1.5e-7;
    (112, 3, 300) out 3.0e-7 / 1.2e-6 / 1.4e-7, p 9.8e-8 / 3.9e-7 / 3.2e-8, dq 2.5e-7 / 1.0e-6 / 1.4e-7, dk 2.3e-7 / 9.1e-7 / 1.0e-7, dv 3.0e-7 /
    1.2e-6 / 1.6e-7; (128, 1, 5) out 4.1e-7 / 1.6e-6 / 6.1e-7, dk 4.8e-7 / 1.9e-6 / 7.6e-7; q x 30: out 2.5e-5 / 1.0e-4 / 1.1e-5, p 6.0e-6 /
    2.4e-5 / 3.4e-6, dq 1.4e-5 / 5.4e-5 / 2.4e-5, dv 1.7e-5 / 6.6e-5 / 9.3e-6 and, the least margin of the 40 comparisons, dk 2.4e-4 /
    9.6e-4 / 6.0e-4 (of 1.1e2)."""
    q, k, v, dout = _attn_inputs(dh, heads, Tk, qscale)
    scale = float(torch.tensor(dh ** -0.5))
    out, p, dq, dk, dv = _attn_run(q, k, v, dout, heads, dh, scale)
    a64, a32 = R.f64(q, k, v), f32(q, k, v)
    o64, p64 = R.attn(*a64, heads, scale)
    o32, p32 = R.attn(*a32, heads, scale, rows=R.weighted_rows_in_groups)
    what = f'attn dh={dh} heads={heads} Tk={Tk} x{qscale:g}'
    near(f'{what} out', out, o64, o32)
    near(f'{what} p', p, p64, p32)
    b64 = R.attn_bwd(*a64, heads, scale, R.f64(dout))
    b32 = R.attn_bwd(*a32, heads, scale, dout, rows=R.weighted_rows_in_groups)
    for name, got, r64, r32 in zip(('dq', 'dk', 'dv'), (dq, dk, dv), b64, b32):
        near(f'{what} {name}', got, r64, r32)


@pytest.mark.parametrize('dh,heads', [(48, 3), (128, 1)])
def test_attn_single_key(dh, heads):
    """Tk = 1: p is exactly 1, out is a copy of the key's v, dq and dk are exactly 0, dv is the column sum of dout over the 16
    queries.  fp32-CPU err / bound / kernel err of dv: dh = 48 1.4e-6 / 5.5e-6 / 1.4e-6, dh = 128 1.5e-6 / 6.1e-6 / 1.5e-6"""
    q, k, v, dout = _attn_inputs(dh, heads, 1)
    out, p, dq, dk, dv = _attn_run(q, k, v, dout, heads, dh, float(torch.tensor(dh ** -0.5)))
    assert bool((p == 1).all())
    exact('attn Tk = 1 out', out, R.f64(v).expand_as(out))
    assert bool((dq == 0).all()) and bool((dk == 0).all())
    near(f'attn Tk = 1 dh={dh} dv', dv, R.f64(dout).sum(dim=1, keepdim=True), dout.sum(dim=1, keepdim=True))


@pytest.mark.parametrize('why', ['Tq', 'dh144', 'dh24', 'pitch', 'E>ldq'])
def test_attn_refusals(why):
    """Tq != 16, dh = 144, dh = 24, a pitch that is no multiple of 4 and E > ldq are refused, forward and backward: nothing is
    launched, every output keeps its NaN"""
    heads, dh, Tq, Tk = {'dh144': (1, 144, 16, 5), 'dh24': (2, 24, 16, 5), 'Tq': (2, 32, 15, 5)}.get(why, (2, 32, 16, 5))
    N, E = 2, heads * dh
    ld = {'pitch': E + 2, 'E>ldq': E - 4}.get(why, E + 4)
    wide = max(ld, E) + 4
    q, kv, dout = dev(g(N, 16, wide, seed=1)), dev(g(N, Tk, 2 * wide, seed=2)), dev(g(N, 16, wide, seed=3))
    out, p, ds, dq, dkv = Out(N, 16, wide), Out(N, heads, 16, Tk), Out(N, heads, 16, Tk), Out(N, 16, wide), Out(N, Tk, 2 * wide)
    io = dict(q=q, k=kv, v=kv.data_ptr() + 4 * wide, p=p, ldq=ld, ldk=2 * wide, ldv=2 * wide, ldo=wide, N=N, Tq=Tq, Tk=Tk, heads=heads,
              dh=dh, scale=dh ** -0.5)
    with pytest.raises(L.GaError):
        launch(L.AttnDesc, out=out, **io)
    with pytest.raises(L.GaError):
        launch(L.AttnDesc, dout=dout, ds=ds, dq=dq, dk=dkv, dv=dkv.t.data_ptr() + 4 * wide, lddq=wide, lddk=2 * wide, lddv=2 * wide,
               backward=1, **io)
    untouched(out, p, ds, dq, dkv)


# =====================================================================================================================
# ga_layernorm
# =====================================================================================================================
LN_C = [4, 100, 260, 512, 1028]
LN_ROWS, LN_EPS = 7, float(torch.tensor(1e-5))


def _ln_inputs(C, with_b, offset=0.0):
    a, b = g(LN_ROWS, C, seed=1), (g(LN_ROWS, C, seed=2, scale=0.5) if with_b else None)
    if offset:                      # a constant of `offset` standard deviations on every token, alternating sign
        std = (1.25 if with_b else 1.0) ** 0.5
        a = a + offset * std * ((1 - 2 * (torch.arange(LN_ROWS) % 2)).float() * (1 + 0.1 * CS.u(LN_ROWS, seed=9)))[:, None]
    return a, b, 1 + 0.2 * g(C, seed=3), g(C, seed=4), g(LN_ROWS, C, seed=5), g(LN_ROWS, C, seed=6)


@pytest.mark.parametrize('C', LN_C)
@pytest.mark.parametrize('with_b', [True, False])
def test_layernorm(C, with_b):
    """7 tokens, one wavefront each, four per workgroup: the second workgroup is partial.  C = 4 (one lane), 100 (25 lanes), 260
    (one full trip of 64 lanes x 4 and a second one of a single lane) and 1028 (four trips and a lane) are the partial trips, 512
    the two full ones; with b and with b = NULL; y and stats; backward with accumulate = 0 into a NaN dx and with accumulate = 1.
    fp32-CPU err / bound / kernel err: over the 40 comparisons the fp32 CPU error is 6.1e-8 .. 8.5e-7 and the kernel's
    4.6e-8 .. 6.6e-7; the least margin: C = 1028 with b, dx accumulated 5.2e-7 / 2.1e-6 / 6.3e-7."""
    a, b, gamma, beta, dy, dx0 = _ln_inputs(C, with_b)
    io = dict(a=dev(a), b=dev(b), gamma=dev(gamma), rows=LN_ROWS, C=C, eps=LN_EPS)
    y, st = Out(LN_ROWS, C), Out(LN_ROWS, 2)
    launch(L.LayernormDesc, beta=dev(beta), y=y, stats=st, **io)
    r64, r32 = R.layernorm(*R.f64(a, b, gamma, beta), LN_EPS), R.layernorm(a, b, gamma, beta, LN_EPS)
    what = f'layernorm C={C} b={with_b}'
    near(f'{what} y', y.done(), r64[0], r32[0])
    near(f'{what} stats', st.done(), r64[1], r32[1])
    dx, dxa = Out(LN_ROWS, C), Out.of(dev(dx0))
    launch(L.LayernormDesc, stats=st, dy=dev(dy), dx=dx, backward=1, accumulate=0, **io)
    launch(L.LayernormDesc, stats=st, dy=dev(dy), dx=dxa, backward=1, accumulate=1, **io)
    d64, d32 = R.layernorm_bwd(*R.f64(a, b, gamma), LN_EPS, R.f64(dy)), R.layernorm_bwd(a, b, gamma, LN_EPS, dy)
    near(f'{what} dx over NaN', dx.done(), d64, d32)
    near(f'{what} dx accumulated', dxa.done(), R.f64(dx0) + d64, dx0 + d32)


@pytest.mark.parametrize('C', LN_C)
def test_layernorm_offset_tokens(C):
    """every token carries a constant of 100 standard deviations: mean^2 is 10^4 x the variance.  The kernel's error against
    float64 may be at most 4 x that of torch.nn.functional.layer_norm in fp32 on the CPU on the same a + b.
    layer_norm fp32 err / bound / kernel err (kernel rstd relative err): C = 4 1.1e-5 / 4.2e-5 / 1.0e-5 (2.9e-6), 100 1.3e-5 /
    5.1e-5 / 1.8e-5 (4.1e-7), 260 1.8e-5 / 7.2e-5 / 9.1e-6 (2.3e-7), 512 1.3e-5 / 5.2e-5 / 1.2e-5 (1.6e-7), 1028 1.3e-5 / 5.0e-5 / 1.2e-5
    (1.5e-7): the two-pass variance holds, no defect."""
    a, b, gamma, beta, _, _ = _ln_inputs(C, True, offset=100.0)
    y, st = Out(LN_ROWS, C), Out(LN_ROWS, 2)
    launch(L.LayernormDesc, a=dev(a), b=dev(b), gamma=dev(gamma), beta=dev(beta), y=y, stats=st, rows=LN_ROWS, C=C, eps=LN_EPS)
    out, stats = y.done(), st.done()
    r64 = R.layernorm(*R.f64(a, b, gamma, beta), LN_EPS)
    cpu = torch.nn.functional.layer_norm(a + b, (C,), gamma, beta, LN_EPS)
    e_cpu, e_k = R.max_err(cpu, r64[0]), R.max_err(out, r64[0])
    bd = max(4 * e_cpu, 2.0 ** -22 * r64[0].abs().max().item())
    e_rstd = ((stats[:, 1].double() - r64[1][:, 1]).abs() / r64[1][:, 1]).max().item()
    print(f'layernorm offset C={C}: layer_norm fp32 err {e_cpu:.3e}, bound {bd:.3e}, kernel err {e_k:.3e}, kernel rstd rel err {e_rstd:.3e}')
    assert torch.isfinite(out).all() and e_k <= bd, f'kernel err {e_k:.3e} > 4 x layer_norm fp32 err {e_cpu:.3e}'


# =====================================================================================================================
# ga_resize2_crop
# =====================================================================================================================
@pytest.mark.parametrize('H,W,crop', [(1, 1, 0), (5, 7, 0), (5, 7, 1), (6, 10, 3), (8, 8, 0)])
@pytest.mark.parametrize('C', [4, 12])
def test_resize2_crop(H, W, crop, C):
    """N = 3.  (1, 1): both neighbours of every output clamp onto the one pixel; (5, 7): odd sizes; crop = 1 and 3: an odd crop
    starts the kept rows on an odd output row, so the row phase of output 0 is 3/4 | 1/4 and the adjoint's first and last input
    rows lose outputs to the crop; forward, adjoint with accumulate = 0 over NaN, adjoint with accumulate = 1.
    fp32-CPU err / bound / kernel err: over the 30 comparisons fp32 CPU 0 .. 9.2e-7, kernel 0 .. 7.8e-7 ((1, 1) is exact); the
    least margin: (6, 10, 3) C = 4 adjoint over NaN 3.4e-7 / 1.4e-6 / 6.5e-7."""
    N, Ho, Wo = 3, 2 * H - 2 * crop, 2 * W
    x, dy, dx0 = g(N, H, W, C, seed=1), g(N, Ho, Wo, C, seed=2), g(N, H, W, C, seed=3)
    what = f'resize2_crop {H}x{W} crop {crop} C={C}'
    y = Out(N, Ho, Wo, C)
    launch(L.Resize2CropDesc, x=dev(x), y=y, N=N, H=H, W=W, C=C, crop=crop)
    near(f'{what} forward', y.done(), R.resize2_crop(R.f64(x), crop), R.resize2_crop(x, crop))
    dx, dxa = Out(N, H, W, C), Out.of(dev(dx0))
    launch(L.Resize2CropDesc, dy=dev(dy), dx=dx, N=N, H=H, W=W, C=C, crop=crop, backward=1, accumulate=0)
    launch(L.Resize2CropDesc, dy=dev(dy), dx=dxa, N=N, H=H, W=W, C=C, crop=crop, backward=1, accumulate=1)
    a64, a32 = R.resize2_crop_adjoint(R.f64(dy), crop), R.resize2_crop_adjoint(dy, crop)
    near(f'{what} adjoint over NaN', dx.done(), a64, a32)
    near(f'{what} adjoint accumulated', dxa.done(), R.f64(dx0) + a64, dx0 + a32)


# =====================================================================================================================
# ga_gconv
# =====================================================================================================================
def _gconv(x, w, bias, cg, KH, KW, stride, pad, Ho, Wo, pro_act=0, dact_x=None, dact_act=0, dact_rep=0):
    N, Hi, Wi, C = x.shape
    y = Out(N, Ho, Wo, C)
    launch(L.GconvDesc, x=dev(x), w=dev(w), bias=dev(bias), dact_x=dev(dact_x), y=y, N=N, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=C, cg=cg, KH=KH,
           KW=KW, stride=stride, pad=pad, pro_act=pro_act, dact_act=dact_act, dact_rep=dact_rep)
    return y.done()


@pytest.mark.parametrize('cg,with_bias,act', [(4, True, R.RELU), (8, False, R.RELU), (16, True, R.NONE), (32, True, R.RELU), (12, True, R.RELU)])
@pytest.mark.parametrize('stride', [1, 2])
def test_gconv_non_square(cg, with_bias, act, stride):
    """3 x 3, pad 1, G = 3 groups, N = 3 images of 9 x 11.  Stride 1: 297 output pixels, so the LDS-weights kernel (cg = 4, 8, 16,
    32) starts a second workgroup and that one is ragged (41 pixels); stride 2 on the odd input: Ho = 5, Wo = 6, the first and
    the last window of both axes hang over the border by one tap.  cg = 12 is the generic kernel.  cg = 8
    runs with bias NULL, cg = 16 with pro_act NONE.
    fp32-CPU err / bound / kernel err: stride 1 (stride 2 within 10 %): cg = 4 3.9e-7 / 1.6e-6 / 3.9e-7,
    8 3.1e-7 / 1.2e-6 / 3.7e-7, 16 7.9e-7 / 3.2e-6 / 1.3e-6, 32 7.3e-7 / 2.9e-6 / 2.0e-6, 12 5.0e-7 / 2.0e-6 / 8.4e-7."""
    N, G, H, W = 3, 3, 9, 11
    C = G * cg
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    assert (Ho, Wo) == ((9, 11) if stride == 1 else (5, 6))
    x, w, b = g(N, H, W, C, seed=1), g(C, 9 * cg, seed=2, scale=(9 * cg) ** -0.5), (g(C, seed=3) if with_bias else None)
    out = _gconv(x, w, b, cg, 3, 3, stride, 1, Ho, Wo, pro_act=act)
    near(f'gconv cg={cg} stride {stride}', out, R.gconv(*R.f64(x, w, b), cg, 3, 3, stride, 1, Ho, Wo, pro_act=act),
         R.gconv(x, w, b, cg, 3, 3, stride, 1, Ho, Wo, pro_act=act))


@pytest.mark.parametrize('cg', CS.GCONV_ANCHORED_CG)
@pytest.mark.parametrize('KH,KW', CS.GCONV_WINDOWS)
def test_gconv_anchored_windows(cg, KH, KW):
    """the sub-kernels of a stride-2 transpose: 1 x 1, 1 x 2, 2 x 1 and 2 x 2 windows anchored at the output pixel (pad 0, Ho = Hi,
    Wo = Wi: the last row / column has its second tap outside the image), with ReLU' of a saved activation and dact_rep = 3 (6
    cotangent rows on 2 forward rows), on the LDS-weights kernel (cg = 4) and the generic one (cg = 12).  The elements whose act'
    source lies on the kink are left out.
    fp32-CPU err / bound / kernel err: over the 8 cases fp32 CPU 2.5e-7 .. 6.3e-7, kernel 2.5e-7 .. 5.8e-7; the least margin: 1 x 2 cg = 4 2.6e-7 / 1.0e-6 / 2.6e-7."""
    c = CS.gconv_anchored_case(cg, KH, KW)
    K, H, W = c['K'], c['H'], c['W']
    x, w, u = c['x'], c['w'], c['dact_x']
    out = _gconv(x, w, None, cg, KH, KW, 1, 0, H, W, dact_x=u, dact_act=L.GA_ACT_RELU, dact_rep=K)
    kw = dict(dact_act=R.RELU, dact_rep=K)
    near(f'gconv anchored {KH}x{KW} cg={cg}', out, R.gconv(*R.f64(x, w), None, cg, KH, KW, 1, 0, H, W, dact_x=R.f64(u), **kw),
         R.gconv(x, w, None, cg, KH, KW, 1, 0, H, W, dact_x=u, **kw), skip=R.rep_rows(R.near_kink(R.f64(u)), K))


# =====================================================================================================================
# ga_gauss_blur
# =====================================================================================================================
def _taps(k):
    t = torch.exp(-(torch.arange(k, dtype=torch.float32) - k // 2) ** 2 / 2)
    return t / t.sum()


@pytest.mark.parametrize('H,W,k,radius', [(8, 12, 15, 0), (12, 8, 15, 0), (5, 90, 9, 0), (12, 700, 23, 0), (12, 700, 23, 4)])
def test_gauss_blur_edges(H, W, k, radius):
    """3 planes, forward and adjoint.  Single-kernel path: (8, 12, 15) and (12, 8, 15) are non-square with k/2 = 7 = min(H, W) - 1,
    the widest reflection the entry point accepts, on the rows and on the columns; (5, 90, 9) has k/2 = H - 1 on a wide plane.
    Two-pass path: (12, 700, 23) has k/2 = 11 = H - 1, a second row tile of 4 of 8 rows and a last column strip of 28 of 32
    columns; tmp starts as NaN and tmp = NULL is still refused.  radius = 4 skips the taps beyond 4 of the centre in the kernel
    and in the reference alike.  The reference adds its taps in tap order.  fp32-CPU err / bound / kernel err: forward, adjoint:
    (8, 12) 1.2e-7 / 5.0e-7 / 1.5e-7, 1.3e-7 / 5.1e-7 / 1.3e-7; (12, 8) 1.7e-7 / 6.7e-7 / 1.1e-7, 1.3e-7 / 5.3e-7 / 1.2e-7; (5, 90) 1.8e-7 /
    7.1e-7 / 1.4e-7, 1.2e-7 / 4.7e-7 / 1.3e-7; (12, 700) 2.2e-7 / 8.7e-7 / 1.9e-7, 2.8e-7 / 1.1e-6 / 2.2e-7; radius 4 1.6e-7 / 6.3e-7 /
    1.7e-7, 2.6e-7 / 1.0e-6 / 2.4e-7."""
    planes = 3
    x, dy, taps = g(planes, H, W, seed=1), g(planes, H, W, seed=2), _taps(k)
    two_pass = (2 * H * W + k) * 4 > 64 * 1024
    assert two_pass == (W == 700)
    io = dict(taps=dev(taps), planes=planes, H=H, W=W, k=k, radius=radius)
    what = f'blur {H}x{W} k={k} radius {radius}'
    for backward, src, ref in ((0, x, R.gauss_blur), (1, dy, R.gauss_blur_adjoint)):
        y, tmp = Out(planes, H, W), (Out(planes, H, W) if two_pass else None)
        launch(L.BlurDesc, x=dev(src), y=y, tmp=tmp, backward=backward, **io)
        near(f'{what} {"adjoint" if backward else "forward"}', y.done(), ref(*R.f64(src, taps), radius), ref(src, taps, radius))
        if two_pass:
            tmp.done()
            y = Out(planes, H, W)
            with pytest.raises(L.GaError):
                launch(L.BlurDesc, x=dev(src), y=y, backward=backward, **io)
            untouched(y)


# =====================================================================================================================
# ga_rowchan_reduce
# =====================================================================================================================
_reduce_order, _order_sum = R.reduce_order, R.order_sum        # the launch's summation order: tests/opref.py holds it


def _reduce(N, P, C, a=None, b=None, ws=None, ws_floats=0, scale=0.5, **kw):
    out = Out(N, C)
    launch(L.ReduceDesc, a=dev(a), b=dev(b), out=out, N=N, P=P, C=C, scale=scale, ws=ws, ws_floats=ws_floats, **kw)
    return out.done()


@pytest.mark.parametrize('C', [12, 20, 40, 100])
@pytest.mark.parametrize('with_b', [True, False])
def test_rowchan_reduce_two_stage_narrow(C, with_b):
    """N = 2, P = 4100, five segments of 820 pixels.  C = 12, 20, 40 have C / 4 = 3, 5, 10 channel quads on ql = 4, 8, 16 quad
    lanes: the surplus lanes must add zeros to the tree; C = 100 has a partial second 64-channel chunk.  The workspace starts
    as NaN; two launches give the same bits.  Yardstick: the fp32 CPU sum in segment / lane / tree order.
    fp32-CPU err / bound / kernel err: with b: C = 12 9.6e-6 / 3.9e-5 / 9.6e-6, 20 1.1e-5 / 4.3e-5 / 1.1e-5, 40 1.4e-5 /
    5.5e-5 / 1.4e-5, 100 1.5e-5 / 6.1e-5 / 1.5e-5; without: 8.2e-6 / 3.3e-5 / 8.2e-6, 6.6e-6 / 2.6e-5 / 6.6e-6, 1.1e-5 / 4.6e-5 / 1.1e-5,
    1.5e-5 / 5.9e-5 / 1.5e-5 (the kernel's error equals the yardstick's: the documented order is the order it adds in)."""
    N, P = 2, 4100
    a, b = g(N, P, C, seed=1), (g(N, P, C, seed=2) if with_b else None)
    S, lanes = _reduce_order(N, P, C, 64 * N * C)
    assert (S, lanes) == (5, {12: 64, 20: 32, 40: 16, 100: 16}[C])
    ws = Out(64 * N, C)
    out = _reduce(N, P, C, a, b, ws, 64 * N * C)
    near(f'rowchan_reduce C={C} b={with_b}', out, R.rowchan_reduce(*R.f64(a, b), 0.5)[0], R.rowchan_reduce(a, b, 0.5, total=_order_sum(S, lanes))[0])
    assert torch.equal(out, _reduce(N, P, C, a, b, ws, 64 * N * C)), 'two launches differ'
    ws.done()


def test_rowchan_reduce_formed_operand_two_stage():
    """C = 20 (ql = 8 > C / 4), a formed from a_src [N,P,4] and a_w [C][4], b given, scaled = a * gate + skip with scaled aliasing
    skip.  fp32-CPU err / bound / kernel err: out 2.4e-5 / 9.8e-5 / 2.6e-5, scaled 1.3e-6 / 5.3e-6 / 1.2e-6"""
    N, P, C = 2, 4100, 20
    src, aw, b, gate, skip = g(N, P, 4, seed=1), g(C, 4, seed=2, scale=0.5), g(N, P, C, seed=3), g(N, C, seed=4), g(N, P, C, seed=5)
    S, lanes = _reduce_order(N, P, C, 64 * N * C)
    ws, scaled = Out(64 * N, C), Out.of(dev(skip))
    out = _reduce(N, P, C, None, b, ws, 64 * N * C, scale=1.0, a_src=dev(src), a_w=dev(aw), gate=dev(gate), skip=scaled.t, scaled=scaled)
    r64 = R.rowchan_reduce(None, R.f64(b), 1.0, *R.f64(gate, skip, src, aw))
    r32 = R.rowchan_reduce(None, b, 1.0, gate, skip, src, aw, total=_order_sum(S, lanes))
    near('rowchan_reduce a_src out', out, r64[0], r32[0])
    near('rowchan_reduce a_src scaled', scaled.done(), r64[1], r32[1])


def test_rowchan_reduce_workspace_sizes():
    """C = 20, N = 2.  ws_floats = 2 N C, the documented minimum: two segments, and the row behind the workspace keeps its
    sentinel.  ws_floats = N C leaves S = 1: the single-stage result bit for bit.  P = 4095, just under the two-stage threshold,
    with a workspace supplied: single stage as well, the workspace stays NaN.  Yardstick: the fp32 CPU sum in the kernel's
    order (two segments with the tree; 16 lanes in lane order).
    fp32-CPU err / bound / kernel err: ws = 2NC 1.2e-5 / 5.0e-5 / 1.2e-5, single stage 2.8e-5 / 1.1e-4 / 2.8e-5, P = 4095 2.9e-5 / 1.2e-4 /
    2.9e-5"""
    N, P, C = 2, 4100, 20
    a, b = g(N, P, C, seed=1), g(N, P, C, seed=2)
    r64 = R.rowchan_reduce(*R.f64(a, b), 0.5)[0]
    ws = Out(2 * N, C)
    assert _reduce_order(N, P, C, 2 * N * C) == (2, 32)
    near('rowchan_reduce ws = 2NC', _reduce(N, P, C, a, b, ws, 2 * N * C), r64, R.rowchan_reduce(a, b, 0.5, total=_order_sum(2, 32))[0])
    assert torch.isfinite(ws.done()).all()
    single = _reduce(N, P, C, a, b)
    near('rowchan_reduce single stage', single, r64, R.rowchan_reduce(a, b, 0.5, total=_order_sum(1, 16))[0])
    ws = Out(N, C)
    assert torch.equal(_reduce(N, P, C, a, b, ws, N * C), single), 'ws_floats = N C is not the single-stage result'
    assert bool(torch.isnan(ws.done()).all())
    a, b = a[:, :4095].contiguous(), b[:, :4095].contiguous()
    ws = Out(64 * N, C)
    out = _reduce(N, 4095, C, a, b, ws, 64 * N * C)
    near('rowchan_reduce P = 4095', out, R.rowchan_reduce(*R.f64(a, b), 0.5)[0], R.rowchan_reduce(a, b, 0.5, total=_order_sum(1, 16))[0])
    assert torch.equal(out, _reduce(N, 4095, C, a, b)) and bool(torch.isnan(ws.done()).all())


# =====================================================================================================================
# ga_avgpool_act
# =====================================================================================================================
@pytest.mark.parametrize('P,C', CS.AVGPOOL_SHAPES)
@pytest.mark.parametrize('act', [R.NONE, R.RELU, R.SILU])
def test_avgpool_act_edges(P, C, act):
    """N = 3.  P = 1: fifteen of the sixteen pixel lanes add nothing; P = 15: one lane short; P = 49 (the 7 x 7 map) with C = 132:
    a third 64-channel chunk of one quad.  Backward over a NaN dx; with ReLU the elements on the kink are left out.
    fp32-CPU err / bound / kernel err: over the 18 comparisons fp32 CPU 0 .. 1.4e-7, kernel 0 .. 1.4e-7 (P = 1 with
    NONE and RELU is exact); the least margin: P = 49 C = 132 RELU forward 6.6e-8 / 2.7e-7 / 1.3e-7."""
    c = CS.avgpool_case(P, C)
    x, dy = c['x'], c['dy']
    N = x.shape[0]
    y, dx = Out(N, C), Out(N, P, C)
    launch(L.AvgpoolActDesc, x=dev(x), y=y, N=N, P=P, C=C, act=act)
    launch(L.AvgpoolActDesc, x=dev(x), dy=dev(dy), dx=dx, N=N, P=P, C=C, act=act, backward=1)
    what = f'avgpool_act P={P} C={C} act {act}'
    near(f'{what} forward', y.done(), R.avgpool_act(R.f64(x), act), R.avgpool_act(x, act))
    near(f'{what} backward', dx.done(), R.avgpool_act_bwd(R.f64(x), act, R.f64(dy)), R.avgpool_act_bwd(x, act, dy),
         skip=R.near_kink(R.f64(x)) if act == R.RELU else None)
