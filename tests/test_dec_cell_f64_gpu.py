"""
ga_dec_cell against the float64 cell of tests/cellref.py, row by row: every image row n may differ from float64 by at most
cellref.row_bound = 4 x the error of the split-bf16 emulation in plain fp32 on the CPU in that row (floor 2^-22 of the row's
max |ref|; tests/test_cellref_cpu.py shows that the floor decides no row and that one missing lo chunk leaves the bound by 9 x
or more on these inputs).  Image i is scaled by 4 ** (i % 3 - 1): the images that share one framed LDS plane differ by a factor of 4
or 16, so a leak across a frame or an error in a small image is not hidden under the largest image's maximum.  Outputs start as
NaN with a sentinel row behind them (Out / launch of tests/test_ops_edges_gpu.py).

  geometry   every (H, W, C) ga_dec_cell_supported accepts among the power-of-two images up to 128 x 128, two workgroups each,
             Hd 32 (one chunk: every "next chunk" index is clamped) and 96, forward and backward; variant 1 = variant 0 bitwise
  pipeline   Hd 64 at the square shapes, the shipped Hd 768 / 1536 once each
  defect     the shipped shapes with the lo rows of chunk 0 zeroed in the w1_lo (forward) / W2^T lo (backward) buffer: out of bound
  act_rep    3 cotangents per forward row: within the bound and bitwise an act_rep = 1 launch on x.repeat_interleave(3, 0)
  unfused    the fused result equals the three launches it replaces bit for bit (csrc/dec_cell.hip), every geometry
  refusals   GA_E_ALIGN / GA_E_BADARG leave the output's NaN fill alone

Measured on an MI355X (whole tensor: emulation err / bound / kernel err; kernel err / emulation err of the worst row; the last
three lines are the act_rep cases N x H x W x C x Hd x variant).  The largest kernel err / bound of any row is 0.36.  Fused and unfused
were bitwise equal at all 15 geometries, both hidden widths, forward and backward (60 comparisons).  With the lo chunk zeroed:
2x16x16x128x768 forward 6.6e-4 against a bound of 4.5e-5 (14.6 x the bound in row 1), backward 2.3e-4 against 4.9e-6 (66 x);
2x8x8x256x1536 forward 3.6e-4 against 3.6e-5 (10 x), backward 2.4e-4 against 4.0e-6 (67 x).
  4x8x16x128x32     fwd 7.807e-5 / 3.123e-4 / 7.783e-5; 1.01   bwd 3.529e-5 / 1.412e-4 / 3.577e-5; 1.20
  4x8x16x128x96     fwd 7.139e-5 / 2.856e-4 / 7.127e-5; 1.01   bwd 3.088e-5 / 1.235e-4 / 3.104e-5; 1.06
  2x8x32x128x32     fwd 1.778e-5 / 7.111e-5 / 1.778e-5; 1.00   bwd 4.592e-6 / 1.837e-5 / 4.651e-6; 1.01
  2x8x32x128x96     fwd 1.131e-5 / 4.524e-5 / 1.118e-5; 1.00   bwd 2.629e-6 / 1.052e-5 / 2.990e-6; 1.14
  4x16x8x128x32     fwd 8.862e-5 / 3.545e-4 / 8.815e-5; 1.03   bwd 3.533e-5 / 1.413e-4 / 3.569e-5; 1.04
  4x16x8x128x96     fwd 5.518e-5 / 2.207e-4 / 5.506e-5; 1.01   bwd 2.247e-5 / 8.987e-5 / 2.271e-5; 1.06
  2x16x16x128x32    fwd 1.960e-5 / 7.840e-5 / 1.957e-5; 1.00   bwd 3.769e-6 / 1.507e-5 / 3.888e-6; 1.03
  2x16x16x128x96    fwd 1.285e-5 / 5.139e-5 / 1.285e-5; 1.00   bwd 2.737e-6 / 1.095e-5 / 2.737e-6; 1.01
  2x32x8x128x32     fwd 1.332e-5 / 5.328e-5 / 1.297e-5; 1.00   bwd 3.571e-6 / 1.428e-5 / 3.639e-6; 1.02
  2x32x8x128x96     fwd 1.178e-5 / 4.712e-5 / 1.193e-5; 1.01   bwd 2.579e-6 / 1.031e-5 / 2.571e-6; 1.00
  2x2x64x256x32     fwd 9.316e-6 / 3.726e-5 / 9.316e-6; 1.01   bwd 3.426e-6 / 1.371e-5 / 3.426e-6; 1.04
  2x2x64x256x96     fwd 1.511e-5 / 6.044e-5 / 1.505e-5; 1.03   bwd 2.491e-6 / 9.966e-6 / 2.447e-6; 1.02
  8x4x8x256x32      fwd 7.142e-5 / 2.857e-4 / 7.046e-5; 1.00   bwd 6.736e-5 / 2.694e-4 / 6.712e-5; 1.00
  8x4x8x256x96      fwd 4.628e-5 / 1.851e-4 / 4.652e-5; 1.43   bwd 4.027e-5 / 1.611e-4 / 3.991e-5; 1.11
  4x4x16x256x32     fwd 6.603e-5 / 2.641e-4 / 6.555e-5; 1.01   bwd 3.154e-5 / 1.262e-4 / 3.142e-5; 1.01
  4x4x16x256x96     fwd 4.399e-5 / 1.760e-4 / 4.447e-5; 1.01   bwd 3.788e-5 / 1.515e-4 / 3.818e-5; 1.02
  2x4x32x256x32     fwd 1.397e-5 / 5.588e-5 / 1.433e-5; 1.03   bwd 5.364e-6 / 2.146e-5 / 5.215e-6; 1.02
  2x4x32x256x96     fwd 1.298e-5 / 5.194e-5 / 1.304e-5; 1.00   bwd 2.888e-6 / 1.155e-5 / 3.074e-6; 1.06
  8x8x4x256x32      fwd 5.401e-5 / 2.161e-4 / 5.592e-5; 1.22   bwd 3.473e-5 / 1.389e-4 / 3.401e-5; 1.03
  8x8x4x256x96      fwd 4.390e-5 / 1.756e-4 / 4.477e-5; 1.04   bwd 2.463e-5 / 9.854e-5 / 2.422e-5; 1.08
  4x8x8x256x32      fwd 6.319e-5 / 2.528e-4 / 6.319e-5; 1.03   bwd 2.958e-5 / 1.183e-4 / 2.985e-5; 1.01
  4x8x8x256x96      fwd 5.542e-5 / 2.217e-4 / 5.495e-5; 1.00   bwd 3.379e-5 / 1.352e-4 / 3.355e-5; 1.03
  2x8x16x256x32     fwd 1.488e-5 / 5.951e-5 / 1.482e-5; 1.00   bwd 3.462e-6 / 1.385e-5 / 3.704e-6; 1.07
  2x8x16x256x96     fwd 1.426e-5 / 5.702e-5 / 1.432e-5; 1.00   bwd 3.220e-6 / 1.288e-5 / 3.175e-6; 1.01
  4x16x4x256x32     fwd 6.307e-5 / 2.523e-4 / 6.307e-5; 1.00   bwd 3.832e-5 / 1.533e-4 / 3.903e-5; 1.02
  4x16x4x256x96     fwd 4.266e-5 / 1.706e-4 / 4.206e-5; 1.02   bwd 2.490e-5 / 9.960e-5 / 2.490e-5; 1.01
  2x16x8x256x32     fwd 1.456e-5 / 5.823e-5 / 1.459e-5; 1.01   bwd 6.140e-6 / 2.456e-5 / 6.169e-6; 1.00
  2x16x8x256x96     fwd 1.072e-5 / 4.287e-5 / 1.048e-5; 1.00   bwd 4.109e-6 / 1.644e-5 / 3.826e-6; 0.96
  2x32x4x256x32     fwd 1.255e-5 / 5.019e-5 / 1.255e-5; 1.00   bwd 4.401e-6 / 1.761e-5 / 4.312e-6; 0.98
  2x32x4x256x96     fwd 1.000e-5 / 4.001e-5 / 1.048e-5; 1.05   bwd 2.694e-6 / 1.078e-5 / 2.694e-6; 1.03
  2x16x16x128x64    fwd 1.462e-5 / 5.847e-5 / 1.497e-5; 1.02   bwd 2.801e-6 / 1.121e-5 / 2.816e-6; 1.01
  4x8x8x256x64      fwd 7.250e-5 / 2.900e-4 / 7.369e-5; 1.02   bwd 3.725e-5 / 1.490e-4 / 3.713e-5; 1.01
  2x16x16x128x768   fwd 1.132e-5 / 4.529e-5 / 1.105e-5; 0.98   bwd 1.235e-6 / 4.939e-6 / 1.235e-6; 1.01
  2x8x8x256x1536    fwd 8.886e-6 / 3.554e-5 / 9.467e-6; 1.07   bwd 9.988e-7 / 3.995e-6 / 1.029e-6; 1.03
  6x8x8x256x64x0    bwd 2.238e-5 / 8.954e-5 / 2.203e-5; 1.04
  6x16x16x128x32x1  bwd 1.725e-5 / 6.900e-5 / 1.695e-5; 1.01
  6x8x16x128x96x0   bwd 1.082e-5 / 4.330e-5 / 1.142e-5; 1.07
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

import cellref as CR   # noqa: E402
import opref as R   # noqa: E402
from gen_adversarial_amd import _lib as L   # noqa: E402
from test_ops_gpu import DEV, run_conv   # noqa: E402
from test_ops_edges_gpu import Out, dev, launch   # noqa: E402

GEOMS = CR.accepted_geometries(L.lib.ga_dec_cell_supported)          # the library is the record
GEOMETRY_CASES = CR.geometry_cases(GEOMS)
NOT_BIT_EQUAL = set()        # (H, W, C) whose fused result differs from the unfused launches in the last bits: none


def ident(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def split(w):
    hi = w.to(torch.bfloat16)
    return hi.contiguous(), (w - hi.float()).to(torch.bfloat16).contiguous()


class Cell:
    """the device side of one cellref.inputs case"""

    def __init__(self, c):
        self.c = c
        self.x, self.dout, self.ps, self.pb = dev(c.x), dev(c.dout), dev(c.ps), dev(c.pb)
        self.w1f, self.w2f, self.w2t = dev(c.w1), dev(c.w2), dev(c.w2.t())
        self.w1, self.w2, self.w2ts = split(self.w1f), split(self.w2f), split(self.w2t)
        self.wd, self.wdb = dev(c.wd), dev(CR.flip_taps(c.wd))
        self.b1, self.bd, self.b2 = dev(c.b1), dev(c.bd), dev(c.b2)

    def desc(self, backward, **over):
        c = self.c
        kw = dict(x=self.x, w1_hi=self.w1[0], w1_lo=self.w1[1], b1=self.b1, wd=self.wd, wd_bwd=self.wdb, bd=self.bd,
                  N=c.N, H=c.H, W=c.W, C=c.C, Hd=c.Hd, backward=backward)
        if backward:
            kw.update(w2_hi=self.w2ts[0], w2_lo=self.w2ts[1], dout=self.dout, pro_scale=self.ps, pro_shift=self.pb, act_rep=c.act_rep)
        else:
            kw.update(w2_hi=self.w2[0], w2_lo=self.w2[1], b2=self.b2)
        kw.update(over)
        return kw

    def run(self, backward, **over):
        c = self.c
        y = Out(c.N, c.H, c.W, c.Hd if backward else c.C)
        launch(L.DecCellDesc, y=y, **self.desc(backward, **over))
        return y.done()

    def unfused(self):
        """-> t3, dt1 of the three launches per direction that ga_dec_cell replaces (test_dec_cell_gpu.py)"""
        c = self.c
        hid = (c.N, c.H, c.W, c.Hd)
        u1, u2, u3 = torch.empty(hid, device=DEV), torch.empty(hid, device=DEV), torch.empty(c.N, c.H, c.W, c.C, device=DEV)
        run_conv(self.x, self.w1f, u1, 1, bias=self.b1, w_hi=self.w1[0], w_lo=self.w1[1])
        launch(L.DwDesc, x=u1, w=self.wd, bias=self.bd, y=u2, N=c.N, H=c.H, W=c.W, C=c.Hd, pro_act=L.GA_ACT_SILU)
        run_conv(u2, self.w2f, u3, 1, bias=self.b2, pro_act=L.GA_ACT_SILU, w_hi=self.w2[0], w_lo=self.w2[1])
        v2, v1 = torch.empty(hid, device=DEV), torch.empty(hid, device=DEV)
        run_conv(self.dout, self.w2t, v2, 1, pro_scale=self.ps, pro_shift=self.pb, pro_per_row=1, dact_x=u2,
                 dact_act=L.GA_ACT_SILU, lddact=c.Hd, w_hi=self.w2ts[0], w_lo=self.w2ts[1])
        launch(L.DwDesc, x=v2, w=self.wdb, dact_x=u1, y=v1, N=c.N, H=c.H, W=c.W, C=c.Hd, dact_act=L.GA_ACT_SILU)
        torch.cuda.synchronize()
        return u3.cpu(), v1.cpu()


@functools.lru_cache(maxsize=None)
def refs(case, K=1):
    """computed once per case and left unchanged: (inputs, float64 t3, emulated t3, float64 dt1, emulated dt1)"""
    c = CR.inputs(*case, act_rep=K)
    x64, w64, cot64 = R.f64(c.x), R.f64(*c.weights), R.f64(*c.cot)
    fwd = (CR.cell_forward(x64, *w64)[2], CR.emulate_forward(c.x, *c.weights)[2]) if K == 1 else (None, None)
    return (c, *fwd, CR.cell_backward(x64, *w64, *cot64, act_rep=K), CR.emulate_backward(c.x, *c.weights, *c.cot, act_rep=K))


@functools.lru_cache(maxsize=None)
def fused(case):
    c = refs(case)[0]
    cell = Cell(c)
    return cell, cell.run(0), cell.run(1)


def both_directions(case):
    c, t3, t3e, dt1, dt1e = refs(case)
    cell, y, g1 = fused(case)
    CR.check_rows(f'dec_cell {ident(case)} forward', y, t3e, t3)
    CR.check_rows(f'dec_cell {ident(case)} backward', g1, dt1e, dt1)
    return cell, y, g1


def test_the_accepted_geometries_are_the_expected_ones():
    assert GEOMS == CR.GEOMS


@pytest.mark.parametrize('case', GEOMETRY_CASES, ids=ident)
def test_every_accepted_geometry(case):
    cell, y, g1 = both_directions(case)
    if case[3] == 128:
        assert torch.equal(cell.run(0, variant=1), y), 'variant 1 (forward) differs from variant 0'
        assert torch.equal(cell.run(1, variant=1), g1), 'variant 1 (backward) differs from variant 0'


@pytest.mark.parametrize('case', CR.PIPELINE_CASES + CR.SHIPPED_CASES, ids=ident)
def test_chunk_pipeline(case):
    both_directions(case)


@pytest.mark.parametrize('case', CR.SHIPPED_CASES, ids=ident)
def test_the_bound_sees_a_missing_lo_chunk(case):
    c, t3, t3e, dt1, dt1e = refs(case)
    cell, y, g1 = both_directions(case)                                  # the intact launch passes
    for backward, (hi, lo), out_ok, emu, ref in ((0, cell.w1, y, t3e, t3), (1, cell.w2ts, g1, dt1e, dt1)):
        broken = lo.clone()
        broken[:CR.CH] = 0                                               # rows 0 .. 31 = hidden chunk 0 of [Hd][C]
        out = cell.run(backward, **{'w2_lo' if backward else 'w1_lo': broken})
        assert torch.isfinite(out).all()
        ratio, n, idx = CR.worst(out, ref, CR.row_bound(emu, ref))
        print(f'dec_cell {ident(case)} {"backward" if backward else "forward"}, lo rows of chunk 0 zeroed: row {n} element '
              f'{tuple(int(i) for i in idx)} is {ratio:.1f} x its bound (err {CR.row_err(out, ref).max().item():.3e}, bound '
              f'{CR.row_bound(emu, ref).max().item():.3e}; intact err {CR.row_err(out_ok, ref).max().item():.3e})')
        with pytest.raises(AssertionError, match='x its bound'):
            CR.check_rows('zeroed lo chunk', out, emu, ref)


@pytest.mark.parametrize('case', CR.ACT_REP_CASES, ids=ident)
def test_act_rep(case):
    K, variant = 3, case[5]
    c, _, _, dt1, dt1e = refs(case[:5], K)
    cell = Cell(c)
    out = cell.run(1, variant=variant)
    CR.check_rows(f'dec_cell {ident(case)} backward, act_rep = 3', out, dt1e, dt1)
    rep = cell.run(1, variant=variant, act_rep=1, x=cell.x.repeat_interleave(K, dim=0).contiguous())
    assert torch.equal(out, rep), 'act_rep = 3 differs from act_rep = 1 on the repeated rows'


@pytest.mark.parametrize('case', GEOMETRY_CASES, ids=ident)
def test_fused_equals_the_three_unfused_launches(case):
    cell, y, g1 = fused(case)
    u3, v1 = cell.unfused()
    for what, a, b in (('forward', y, u3), ('backward', g1, v1)):
        scale, diff = b.abs().max().item(), (a - b).abs().max().item()
        print(f'dec_cell {ident(case)} fused vs unfused {what}: max |diff| {diff:.3e} of {scale:.3e}, bitwise equal: {torch.equal(a, b)}')
        if case[1:4] in NOT_BIT_EQUAL:
            assert diff <= 2e-6 * scale
        else:
            assert torch.equal(a, b), f'{what}: fused and unfused differ by {diff:.3e} of {scale:.3e}'


def test_refusals_leave_the_output_alone():
    case = (2, 16, 16, 128, 32)
    cell = Cell(refs(case)[0])
    c = cell.c

    def refused(backward, want, **over):
        y = Out(c.N, c.H, c.W, c.Hd if backward else c.C)
        d, keep = L.DecCellDesc(), []
        for k, v in dict(cell.desc(backward, **over), y=y.t).items():
            if torch.is_tensor(v):
                keep.append(v)
                v = v.data_ptr()
            setattr(d, k, v)
        assert L.lib.ga_dec_cell(ctypes.byref(d), 0) == want
        assert torch.isnan(y.done()).all(), 'a refused launch wrote its output'

    off = torch.zeros(cell.x.numel() + 4, device=DEV)[1:]               # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    refused(0, L.GA_E_ALIGN, x=off)
    refused(1, L.GA_E_ALIGN, dout=off)
    refused(0, L.GA_E_BADARG, act_rep=3)                                 # replicas are a backward field
    refused(1, L.GA_E_BADARG, act_rep=3)                                 # N = 2 cotangent rows are no multiple of 3
