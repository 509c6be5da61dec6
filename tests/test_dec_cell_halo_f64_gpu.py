"""
ga_dec_cell_halo against the float64 cell of tests/cellref.py, row by row (cellref.row_bound: 4 x the error of the split-bf16
emulation in plain fp32 on the CPU in that image row, floor 2^-22 of the row's max |ref|), image i scaled by 4 ** (i % 3 - 1),
outputs NaN-filled with a sentinel row behind them.

  shapes     8 x 16 (one tile: every side is a border), 16 x 16 and 8 x 32 (two tiles: the recomputed 4-pixel halo crosses one
             seam), 16 x 32, 24 x 48 (an interior tile); C 32 and 64; Hd 32 and 96; N 1 and 3
  forward    t3;  backward  dx with no addend, addend, addend + addend2, and with addend / addend2 ALIASING y (the header allows
             it and the engine uses it): the aliased results equal the others bitwise
  defect     once per C: lo rows of chunk 0 zeroed in the w1_lo (forward) / W2^T lo (backward) buffer: out of bound
  unfused    forward against the three launches it replaces at 2e-6 of max |t3| (the header promises no bits; the outcome is printed)

Measured on an MI355X (whole tensor: emulation err / bound / kernel err; kernel err / emulation err of the worst row).  The
backward figures are those without an addend; with one or both they agree to within 1 % (the addends are a tenth of dout).  The
forward was bitwise equal to the unfused launches in all 40 cases.  With the lo chunk zeroed: 3x16x32x32x96 forward 7.7e-3 against
a bound of 2.1e-4 (36 x the bound in row 2), backward 1.3e-3 against 4.9e-5 (33 x); 3x16x32x64x96 47 x and 33 x.
  1x8x16x32x32      fwd 3.780e-6 / 1.512e-5 / 3.750e-6; 0.99   bwd 2.473e-7 / 9.894e-7 / 2.464e-7; 1.00
  3x8x16x32x32      fwd 5.070e-5 / 2.028e-4 / 5.040e-5; 1.00   bwd 1.190e-5 / 4.759e-5 / 1.181e-5; 1.03
  1x8x16x32x96      fwd 5.280e-6 / 2.112e-5 / 5.280e-6; 1.00   bwd 2.582e-7 / 1.033e-6 / 2.531e-7; 0.98
  3x8x16x32x96      fwd 5.674e-5 / 2.270e-4 / 5.662e-5; 1.00   bwd 1.117e-5 / 4.469e-5 / 1.060e-5; 1.00
  1x8x16x64x32      fwd 4.774e-6 / 1.909e-5 / 4.774e-6; 1.00   bwd 3.075e-7 / 1.230e-6 / 3.094e-7; 1.01
  3x8x16x64x32      fwd 6.183e-5 / 2.473e-4 / 6.183e-5; 1.00   bwd 1.309e-5 / 5.235e-5 / 1.310e-5; 1.01
  1x8x16x64x96      fwd 4.555e-6 / 1.822e-5 / 4.645e-6; 1.02   bwd 2.668e-7 / 1.067e-6 / 2.701e-7; 1.01
  3x8x16x64x96      fwd 4.415e-5 / 1.766e-4 / 4.463e-5; 1.02   bwd 9.625e-6 / 3.850e-5 / 9.476e-6; 1.06
  1x16x16x32x32     fwd 4.245e-6 / 1.698e-5 / 4.305e-6; 1.01   bwd 3.181e-7 / 1.273e-6 / 3.138e-7; 0.99
  3x16x16x32x32     fwd 6.230e-5 / 2.492e-4 / 6.230e-5; 1.05   bwd 1.712e-5 / 6.846e-5 / 1.715e-5; 1.04
  1x16x16x32x96     fwd 4.246e-6 / 1.698e-5 / 4.186e-6; 0.99   bwd 2.670e-7 / 1.068e-6 / 2.613e-7; 0.98
  3x16x16x32x96     fwd 5.664e-5 / 2.266e-4 / 5.616e-5; 1.05   bwd 1.160e-5 / 4.638e-5 / 1.124e-5; 0.99
  1x16x16x64x32     fwd 5.581e-6 / 2.232e-5 / 5.566e-6; 1.00   bwd 3.747e-7 / 1.499e-6 / 3.747e-7; 1.00
  3x16x16x64x32     fwd 6.393e-5 / 2.557e-4 / 6.965e-5; 1.09   bwd 1.350e-5 / 5.400e-5 / 1.362e-5; 1.01
  1x16x16x64x96     fwd 6.166e-6 / 2.466e-5 / 6.166e-6; 1.00   bwd 5.012e-7 / 2.005e-6 / 5.012e-7; 1.00
  3x16x16x64x96     fwd 6.120e-5 / 2.448e-4 / 5.882e-5; 1.01   bwd 1.048e-5 / 4.191e-5 / 9.821e-6; 1.00
  1x8x32x32x32      fwd 4.840e-6 / 1.936e-5 / 4.104e-6; 0.85   bwd 3.561e-7 / 1.425e-6 / 3.580e-7; 1.01
  3x8x32x32x32      fwd 7.105e-5 / 2.842e-4 / 7.129e-5; 1.02   bwd 1.562e-5 / 6.248e-5 / 1.904e-5; 1.22
  1x8x32x32x96      fwd 4.670e-6 / 1.868e-5 / 4.726e-6; 1.01   bwd 2.945e-7 / 1.178e-6 / 2.926e-7; 0.99
  3x8x32x32x96      fwd 4.757e-5 / 1.903e-4 / 4.828e-5; 1.02   bwd 1.021e-5 / 4.084e-5 / 1.095e-5; 1.07
  1x8x32x64x32      fwd 5.774e-6 / 2.310e-5 / 5.774e-6; 1.00   bwd 4.131e-7 / 1.653e-6 / 4.094e-7; 0.99
  3x8x32x64x32      fwd 6.881e-5 / 2.752e-4 / 6.833e-5; 1.00   bwd 1.226e-5 / 4.905e-5 / 1.238e-5; 1.01
  1x8x32x64x96      fwd 5.436e-6 / 2.174e-5 / 5.347e-6; 0.98   bwd 3.415e-7 / 1.366e-6 / 3.396e-7; 0.99
  3x8x32x64x96      fwd 6.422e-5 / 2.569e-4 / 6.469e-5; 1.02   bwd 1.062e-5 / 4.249e-5 / 1.093e-5; 1.03
  1x16x32x32x32     fwd 4.786e-6 / 1.914e-5 / 4.786e-6; 1.00   bwd 4.001e-7 / 1.600e-6 / 3.963e-7; 0.99
  3x16x32x32x32     fwd 7.203e-5 / 2.881e-4 / 7.227e-5; 1.00   bwd 2.061e-5 / 8.244e-5 / 2.067e-5; 1.00
  1x16x32x32x96     fwd 5.069e-6 / 2.028e-5 / 5.039e-6; 0.99   bwd 2.885e-7 / 1.154e-6 / 2.867e-7; 0.99
  3x16x32x32x96     fwd 5.301e-5 / 2.120e-4 / 5.683e-5; 1.07   bwd 1.225e-5 / 4.901e-5 / 1.179e-5; 1.02
  1x16x32x64x32     fwd 5.895e-6 / 2.358e-5 / 5.850e-6; 0.99   bwd 4.351e-7 / 1.740e-6 / 4.406e-7; 1.01
  3x16x32x64x32     fwd 9.192e-5 / 3.677e-4 / 9.144e-5; 1.00   bwd 1.324e-5 / 5.295e-5 / 1.324e-5; 1.01
  1x16x32x64x96     fwd 6.192e-6 / 2.477e-5 / 6.252e-6; 1.01   bwd 3.961e-7 / 1.585e-6 / 4.045e-7; 1.02
  3x16x32x64x96     fwd 6.029e-5 / 2.412e-4 / 5.981e-5; 1.01   bwd 1.176e-5 / 4.702e-5 / 1.177e-5; 1.02
  1x24x48x32x32     fwd 4.766e-6 / 1.906e-5 / 4.736e-6; 0.99   bwd 3.418e-7 / 1.367e-6 / 3.418e-7; 1.00
  3x24x48x32x32     fwd 8.061e-5 / 3.225e-4 / 7.584e-5; 1.00   bwd 2.405e-5 / 9.619e-5 / 2.393e-5; 1.01
  1x24x48x32x96     fwd 5.188e-6 / 2.075e-5 / 5.188e-6; 1.00   bwd 4.163e-7 / 1.665e-6 / 4.079e-7; 0.98
  3x24x48x32x96     fwd 6.449e-5 / 2.580e-4 / 6.544e-5; 1.01   bwd 1.324e-5 / 5.296e-5 / 1.333e-5; 1.02
  1x24x48x64x32     fwd 6.788e-6 / 2.715e-5 / 6.907e-6; 1.02   bwd 5.270e-7 / 2.108e-6 / 5.233e-7; 0.99
  3x24x48x64x32     fwd 8.137e-5 / 3.255e-4 / 8.113e-5; 1.02   bwd 1.725e-5 / 6.899e-5 / 1.659e-5; 1.02
  1x24x48x64x96     fwd 6.465e-6 / 2.586e-5 / 6.525e-6; 1.01   bwd 3.801e-7 / 1.521e-6 / 3.773e-7; 0.99
  3x24x48x64x96     fwd 5.636e-5 / 2.255e-4 / 5.708e-5; 1.01   bwd 1.217e-5 / 4.869e-5 / 1.195e-5; 0.99
"""
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
from test_dec_cell_f64_gpu import ident, split   # noqa: E402


class Halo:
    """the device side of one cellref.inputs case"""

    def __init__(self, c):
        self.c = c
        self.x, self.dout, self.ps, self.pb = dev(c.x), dev(c.dout), dev(c.ps), dev(c.pb)
        self.add, self.add2 = dev(c.add), dev(c.add2)
        self.w1f, self.w2f = dev(c.w1), dev(c.w2)
        self.w1, self.w2 = split(self.w1f), split(self.w2f)
        self.w2ts, self.w1ts = split(dev(c.w2.t())), split(dev(c.w1.t()))
        self.wd, self.wdb = dev(c.wd), dev(CR.flip_taps(c.wd))
        self.b1, self.bd, self.b2 = dev(c.b1), dev(c.bd), dev(c.b2)

    def run(self, backward, y=None, **over):
        c = self.c
        y = Out(c.N, c.H, c.W, c.C) if y is None else y
        kw = dict(x=self.x, w1_hi=self.w1[0], w1_lo=self.w1[1], b1=self.b1, wd=self.wd, wd_bwd=self.wdb, bd=self.bd, b2=self.b2,
                  w1t_hi=self.w1ts[0], w1t_lo=self.w1ts[1], N=c.N, H=c.H, W=c.W, Cin=c.C, Cout=c.C, Hd=c.Hd, backward=backward, up=0)
        if backward:
            kw.update(w2_hi=self.w2ts[0], w2_lo=self.w2ts[1], dout=self.dout, pro_scale=self.ps, pro_shift=self.pb)
        else:
            kw.update(w2_hi=self.w2[0], w2_lo=self.w2[1])
        kw.update(over)
        launch(L.DecCellHaloDesc, y=y, **kw)
        return y.done()

    def unfused_forward(self):
        c = self.c
        hid = (c.N, c.H, c.W, c.Hd)
        u1, u2, u3 = torch.empty(hid, device=DEV), torch.empty(hid, device=DEV), torch.empty(c.N, c.H, c.W, c.C, device=DEV)
        run_conv(self.x, self.w1f, u1, 1, bias=self.b1, w_hi=self.w1[0], w_lo=self.w1[1])
        launch(L.DwDesc, x=u1, w=self.wd, bias=self.bd, y=u2, N=c.N, H=c.H, W=c.W, C=c.Hd, pro_act=L.GA_ACT_SILU)
        run_conv(u2, self.w2f, u3, 1, bias=self.b2, pro_act=L.GA_ACT_SILU, w_hi=self.w2[0], w_lo=self.w2[1])
        torch.cuda.synchronize()
        return u3.cpu()


@functools.lru_cache(maxsize=None)
def refs(case):
    """computed once per case and left unchanged: (inputs, float64 t3, emulated t3, float64 W1^T dt1, emulated W1^T dt1)"""
    c = CR.inputs(*case)
    x64, w64, cot64 = R.f64(c.x), R.f64(*c.weights), R.f64(*c.cot)
    return (c, CR.cell_forward(x64, *w64)[2], CR.emulate_forward(c.x, *c.weights)[2],
            CR.halo_backward(x64, *w64, *cot64), CR.emulate_halo_backward(c.x, *c.weights, *c.cot))


@pytest.mark.parametrize('case', CR.HALO_CASES, ids=ident)
def test_halo_forward_and_backward(case):
    c, t3, t3e, dx, dxe = refs(case)
    h = Halo(c)
    what = f'dec_cell_halo {ident(case)}'
    y = h.run(0)
    CR.check_rows(f'{what} forward', y, t3e, t3)
    u3 = h.unfused_forward()
    scale, diff = u3.abs().max().item(), (y - u3).abs().max().item()
    print(f'{what} fused vs unfused forward: max |diff| {diff:.3e} of {scale:.3e}, bitwise equal: {torch.equal(y, u3)}')
    assert diff <= 2e-6 * scale

    add64, add264 = R.f64(c.add, c.add2)
    plain = h.run(1)
    CR.check_rows(f'{what} backward', plain, dxe, dx)
    one = h.run(1, addend=h.add)
    CR.check_rows(f'{what} backward + addend', one, CR.with_addends(dxe, c.add), CR.with_addends(dx, add64))
    two = h.run(1, addend=h.add, addend2=h.add2)
    CR.check_rows(f'{what} backward + addend + addend2', two, CR.with_addends(dxe, c.add, c.add2), CR.with_addends(dx, add64, add264))
    # in-place accumulation into an already written gradient
    buf = Out.of(h.add)
    assert torch.equal(h.run(1, y=buf, addend=buf.t), one), 'addend aliasing y differs from a separate addend'
    buf = Out.of(h.add2)
    assert torch.equal(h.run(1, y=buf, addend=h.add, addend2=buf.t), two), 'addend2 aliasing y differs from a separate addend2'


@pytest.mark.parametrize('case', CR.HALO_DEFECT_CASES, ids=ident)
def test_the_bound_sees_a_missing_lo_chunk(case):
    c, t3, t3e, dx, dxe = refs(case)
    h = Halo(c)
    for backward, (hi, lo), emu, ref in ((0, h.w1, t3e, t3), (1, h.w2ts, dxe, dx)):
        what = f'dec_cell_halo {ident(case)} {"backward" if backward else "forward"}'
        ok = h.run(backward)
        CR.check_rows(what, ok, emu, ref)                                # the intact launch passes
        broken = lo.clone()
        broken[:CR.CH] = 0                                               # rows 0 .. 31 = hidden chunk 0 of [Hd][C]
        out = h.run(backward, **{'w2_lo' if backward else 'w1_lo': broken})
        assert torch.isfinite(out).all()
        ratio, n, idx = CR.worst(out, ref, CR.row_bound(emu, ref))
        print(f'{what}, lo rows of chunk 0 zeroed: row {n} element {tuple(int(i) for i in idx)} is {ratio:.1f} x its bound '
              f'(err {CR.row_err(out, ref).max().item():.3e}, bound {CR.row_bound(emu, ref).max().item():.3e}; intact err '
              f'{CR.row_err(ok, ref).max().item():.3e})')
        with pytest.raises(AssertionError, match='x its bound'):
            CR.check_rows('zeroed lo chunk', out, emu, ref)
