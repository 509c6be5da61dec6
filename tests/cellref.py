"""
Float64 reference, fp32 yardstick and seeded inputs for the fused decoder cells ga_dec_cell / ga_dec_cell_halo, written from the
formulas of include/ga_ops.h (not from the kernels, no autograd).  No GPU, no library: CPU tensors in, CPU tensors out.

Layout: activations dense NHWC; w1 [Hd][C], wd [25][Hd] (tap-major, tap (kh, kw) reads pixel (h + kh - 2, w + kw - 2)),
w2 [C][Hd]; pro_scale / pro_shift [N][C].

  cell_forward / cell_backward / halo_backward   the header's formulas in the dtype of their inputs (float64 = the reference)
  emulate_forward / emulate_backward / emulate_halo_backward
        the same three results in plain fp32 PyTorch with every 1x1 contraction done the way csrc/conv_split.h does it
        (split4 / mfma3): both operands split as ga_split_bf16 splits them, hi = bf16(v), lo = bf16(v - hi); the products
        lo.hi, hi.lo and hi.hi kept (fp32 matmuls of bf16-valued tensors: every product is exact, the sums are fp32), lo.lo
        dropped; dt3 and (halo) dt1 formed in fp32 before they are split; depthwise part, SiLU and SiLU' plain fp32.
        `zero_lo` names weight matrices whose lo part is zeroed for hidden chunk 0 (32 channels): the defect the bound must see.
  row_bound   opref.bound applied per image row n: max(4 max|emu[n] - ref[n]|, 2^-22 max|ref[n]|), so that a workgroup holding
              images of different magnitude cannot hide an error in the small ones under the large ones' maximum.
  inputs      the seeded case of the GPU tests (weights as tests/test_dec_cell_gpu._cell, image i scaled by 4 ** (i % 3 - 1));
              tests/test_cellref_cpu.py checks the yardstick on exactly these.
"""
import types

import numpy as np
import torch

import opref as R

CH = 32                                      # hidden channels per chunk (DC_CH)


# ---------------------------------------------------------------------------------------------------- formulas
def flip_taps(wd):
    """[25][Hd] forward taps -> the taps of the transposed depthwise conv (wd_bwd)"""
    return wd.flip(0)


def _per_row(v):
    return v[:, None, None, :]


def cell_forward(x, w1, b1, wd, bd, w2, b2, mm=torch.matmul):
    """-> t1 [N,H,W,Hd] = W1 x + b1, t2 = dw5(silu(t1)) + bd, t3 [N,H,W,C] = W2 silu(t2) + b2"""
    t1 = mm(x, w1.t()) + b1
    t2 = R.dwconv5(t1, wd, bd, pro_act=R.SILU)
    t3 = mm(R.act(t2, R.SILU), w2.t()) + b2
    return t1, t2, t3


def cell_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, act_rep=1, mm=torch.matmul, mm1=None):
    """-> dt1 [N,H,W,Hd] = silu'(t1) * dw5^T(silu'(t2) * (W2^T (dout * ps[n] + pb[n]))); cotangent row n reads x row n // act_rep.
    mm1: the contraction of the recomputed expand conv when it differs from mm (the emulation's defects)"""
    t1, t2, _ = cell_forward(R.rep_rows(x, act_rep), w1, b1, wd, bd, w2, b2, mm=mm1 or mm)
    dt3 = dout * _per_row(pro_scale) + _per_row(pro_shift)
    dt2 = mm(dt3, w2) * R.dact(t2, R.SILU)
    return R.dwconv5(dt2, flip_taps(wd), dact_x=t1, dact_act=R.SILU)


def halo_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, addend=None, addend2=None, mm=torch.matmul, mm1=None,
                  mm3=None):
    """-> dx [N,H,W,C] = addend + addend2 + W1^T dt1"""
    dt1 = cell_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, mm=mm, mm1=mm1)
    return with_addends((mm3 or mm)(dt1, w1), addend, addend2)


def with_addends(dx, addend=None, addend2=None):
    """the last step of halo_backward, for a test that wants several addend variants of one W1^T dt1"""
    if addend is not None:
        dx = dx + addend
    if addend2 is not None:
        dx = dx + addend2
    return dx


# ---------------------------------------------------------------------------------------------------- emulation
def split_bf16(v):
    """ga_split_bf16 / split4: hi = bf16(v), lo = bf16(v - hi), both returned as fp32 tensors holding bf16 values"""
    hi = v.to(torch.bfloat16).float()
    return hi, (v - hi).to(torch.bfloat16).float()


def _mm_split(zero_lo_rows=None):
    """a [..., K] @ b [K, M] as mfma3 sums it: a_lo b_hi + a_hi b_lo + a_hi b_hi.  zero_lo_rows = (axis, stop): the lo part of
    b is zeroed on [0, stop) of that axis (a chunk of the weight matrix missing from the w*_lo buffer)"""
    def mm(a, b):
        assert a.dtype == torch.float32 and b.dtype == torch.float32
        ah, al = split_bf16(a)
        bh, bl = split_bf16(b)
        if zero_lo_rows is not None:
            axis, stop = zero_lo_rows
            bl = bl.clone()
            bl.narrow(axis, 0, stop).zero_()
        return (al @ bh + ah @ bl) + ah @ bh
    return mm


def _w1_mm(zero_lo):
    # the expand conv contracts x [.., C] with w1.t() [C][Hd]: chunk 0 = columns 0 .. 31
    return _mm_split((1, CH) if 'w1' in zero_lo else None)


def emulate_forward(x, w1, b1, wd, bd, w2, b2, zero_lo=()):
    """zero_lo: 'w1' (rows 0 .. 31 of w1_lo) and / or 'w2' (columns 0 .. 31 of w2_lo)"""
    mm1, mm2 = _w1_mm(zero_lo), _mm_split((0, CH) if 'w2' in zero_lo else None)
    t1 = mm1(x, w1.t().contiguous()) + b1
    t2 = R.dwconv5(t1, wd, bd, pro_act=R.SILU)
    t3 = mm2(R.act(t2, R.SILU), w2.t().contiguous()) + b2
    return t1, t2, t3


def emulate_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, act_rep=1, zero_lo=()):
    """zero_lo: 'w1' and / or 'w2t' (rows 0 .. 31 of the W2^T lo buffer)"""
    mmg = _mm_split((1, CH) if 'w2t' in zero_lo else None)            # dt3 [.., C] @ w2 [C][Hd]: chunk 0 = columns 0 .. 31
    return cell_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, act_rep=act_rep, mm=mmg, mm1=_w1_mm(zero_lo))


def emulate_halo_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, addend=None, addend2=None, zero_lo=()):
    mmg = _mm_split((1, CH) if 'w2t' in zero_lo else None)
    return halo_backward(x, w1, b1, wd, bd, w2, b2, dout, pro_scale, pro_shift, addend, addend2, mm=mmg, mm1=_w1_mm(zero_lo),
                         mm3=_mm_split())


# ---------------------------------------------------------------------------------------------------- the yardstick
def row_err(a, ref):
    """[N]: max |a[n] - ref[n]| over everything but the image row index"""
    return (a.detach().double() - ref.double()).abs().flatten(1).max(dim=1).values


def row_bound(emu, ref):
    """[N]: opref.bound row by row"""
    return torch.maximum(4.0 * row_err(emu, ref), 2.0 ** -22 * ref.double().abs().flatten(1).max(dim=1).values)


def row_floor_decides(emu, ref):
    """True when some row's bound is its 2^-22 floor and not its 4 x emulation term"""
    return bool((4.0 * row_err(emu, ref) <= 2.0 ** -22 * ref.double().abs().flatten(1).max(dim=1).values).any())


def worst(out, ref, bound):
    """(ratio, row, index inside the row) of the element with the largest err / bound[row]"""
    e = (out.detach().double() - ref.double()).abs().flatten(1) / bound[:, None]
    flat = int(e.argmax())
    n, i = divmod(flat, e.shape[1])
    return e[n, i].item(), n, np.unravel_index(i, tuple(out.shape[1:]))


def check_rows(what, out, emu, ref):
    """assert |out - ref| <= row_bound(emu, ref) in every row; prints and returns (emulation err, bound, kernel err, ratio) over
    the whole tensor, ratio = kernel err / emulation err of the worst row"""
    assert torch.isfinite(out).all(), f'{what}: not every element was written'
    b, ee, ke = row_bound(emu, ref), row_err(emu, ref), row_err(out, ref)
    ratio, n, idx = worst(out, ref, b)
    fig = (ee.max().item(), b.max().item(), ke.max().item(), (ke / ee).max().item())
    print(f'{what}: emulation err {fig[0]:.3e}, bound {fig[1]:.3e}, kernel err {fig[2]:.3e}, kernel / emulation {fig[3]:.2f} '
          f'(worst row {n}: {ke[n].item():.3e} of bound {b[n].item():.3e})')
    assert ratio <= 1.0, (f'{what}: row {n} element {tuple(int(i) for i in idx)} is {ratio:.2f} x its bound '
                          f'(kernel err {ke[n].item():.3e}, bound {b[n].item():.3e}, emulation err {ee[n].item():.3e})')
    return fig


# ---------------------------------------------------------------------------------------------------- inputs
def g(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def image_scale(n):
    """[n]: 4 ** (i % 3 - 1): neighbouring images differ by a factor of 4 or 16"""
    return torch.tensor([4.0 ** (i % 3 - 1) for i in range(n)])


def inputs(N, H, W, C, Hd, act_rep=1, seed=11):
    """fp32 case: x [N / act_rep, H, W, C] and dout [N, H, W, C] scaled per image, weights as tests/test_dec_cell_gpu._cell,
    prologue and addends as that file's backward"""
    Nx = N // act_rep
    c = types.SimpleNamespace(N=N, H=H, W=W, C=C, Hd=Hd, act_rep=act_rep)
    c.x = (g(Nx, C, H, W, seed=seed).permute(0, 2, 3, 1) * image_scale(Nx).view(Nx, 1, 1, 1)).contiguous()
    c.w1 = g(Hd, C, seed=seed + 1, scale=1.0 / np.sqrt(C))
    c.b1 = g(Hd, seed=seed + 2, scale=0.3)
    c.wd = g(Hd, 25, seed=seed + 3, scale=0.2).t().contiguous()
    c.bd = g(Hd, seed=seed + 4, scale=0.3)
    c.w2 = g(C, Hd, seed=seed + 5, scale=1.0 / np.sqrt(Hd))
    c.b2 = g(C, seed=seed + 6, scale=0.3)
    c.dout = (g(N, C, H, W, seed=21).permute(0, 2, 3, 1) * image_scale(N).view(N, 1, 1, 1)).contiguous()
    c.ps = g(N, C, seed=22).abs() * 0.1 + 0.05
    c.pb = g(N, C, seed=23) * 0.01
    # the addends are gradients of the tensor dx is one of: the image's scale, and a tenth of dout's magnitude like dx itself
    # (unit-normal addends would put every row's 2^-22 floor above its emulation term)
    c.add = (g(N, C, H, W, seed=24).permute(0, 2, 3, 1) * (0.1 * image_scale(N)).view(N, 1, 1, 1)).contiguous()
    c.add2 = (g(N, C, H, W, seed=25).permute(0, 2, 3, 1) * (0.1 * image_scale(N)).view(N, 1, 1, 1)).contiguous()
    c.weights = (c.w1, c.b1, c.wd, c.bd, c.w2, c.b2)
    c.cot = (c.dout, c.ps, c.pb)
    return c


# ---------------------------------------------------------------------------------------------------- cases
TILE_PIXELS = {128: 256, 256: 128}           # pixels per ga_dec_cell workgroup

# what ga_dec_cell_supported is expected to accept among the power-of-two images up to 128 x 128 (read off dc_lds_bytes;
# 2 x 64 x 256 fits the forward LDS budget by 128 bytes).  tests/test_cellref_cpu.py asserts that the library reports this set.
GEOMS = {128: [(8, 16), (8, 32), (16, 8), (16, 16), (32, 8)],
         256: [(2, 64), (4, 8), (4, 16), (4, 32), (8, 4), (8, 8), (8, 16), (16, 4), (16, 8), (32, 4)]}


def accepted_geometries(supported):
    """{C: [(H, W), ...]} over H, W in 1, 2, .. 128, asking the library with two workgroups' worth of rows"""
    out = {}
    for C, M in TILE_PIXELS.items():
        out[C] = []
        for H in (1 << i for i in range(8)):
            for W in (1 << i for i in range(8)):
                if H * W <= 2 * M and (2 * M) % (H * W) == 0 and supported(2 * M // (H * W), H, W, C, 32) == 1:
                    out[C].append((H, W))
    return out


def geometry_cases(geoms=None):
    """(N, H, W, C, Hd): every accepted geometry with N H W = 2 M, at one chunk and at three"""
    geoms = GEOMS if geoms is None else geoms
    return [(2 * TILE_PIXELS[C] // (H * W), H, W, C, Hd) for C in sorted(geoms) for (H, W) in geoms[C] for Hd in (32, 96)]


PIPELINE_CASES = [(2, 16, 16, 128, 64), (4, 8, 8, 256, 64)]                   # Hd 32 and 96 are in geometry_cases
SHIPPED_CASES = [(2, 16, 16, 128, 768), (2, 8, 8, 256, 1536)]                 # the second: the smallest N the shape accepts
ACT_REP_CASES = [(6, 8, 8, 256, 64, 0), (6, 16, 16, 128, 32, 1), (6, 8, 16, 128, 96, 0)]       # N, H, W, C, Hd, variant
HALO_CASES = [(N, H, W, C, Hd) for (H, W) in ((8, 16), (16, 16), (8, 32), (16, 32), (24, 48)) for C in (32, 64) for Hd in (32, 96)
              for N in (1, 3)]
HALO_DEFECT_CASES = [(3, 16, 32, 32, 96), (3, 16, 32, 64, 96)]
