"""
tests/cellref.py validated without a GPU:
  * cell_backward and halo_backward (explicit formulas) equal float64 autograd through F.conv2d (grouped for the depthwise part)
    to 1e-12 relative, with act_rep = 3 and both addends;
  * the case lists: ga_dec_cell_supported (host code) reports exactly cellref.GEOMS;
  * detection power, on the exact inputs of every GPU case of tests/test_dec_cell_f64_gpu.py and
    tests/test_dec_cell_halo_f64_gpu.py: the emulation with ONE injected defect - the lo part of hidden chunk 0 missing from w1
    (forward) or from W2^T (backward) - leaves row_bound by a factor of 3 or more in at least one row, and the 2^-22 floor
    decides no row's bound (4 x the emulation error is larger in every row).
Measured over the whole tensor (emulation err / bound / defect err; defect err / bound in the worst row):
  2 x 16 x 16 x 128, Hd 768    forward 1.1e-5 / 4.5e-5 / 6.6e-4; 14.6     backward 1.2e-6 / 4.9e-6 / 2.3e-4; 65.6
  2 x 8 x 8 x 256, Hd 1536     forward 9.2e-6 / 3.7e-5 / 3.6e-4; 9.6      backward 1.0e-6 / 4.1e-6 / 2.4e-4; 66.4
9.6 is the smallest factor of all cases (the kernel with the same rows zeroed in its buffer: 6.59e-4 and 14.6 at Hd 768).
"""
import pytest
import torch
import torch.nn.functional as F

import cellref as CR
import opref as R

TOL = 1e-12
POWER = 3.0


def same(a, b, what=''):
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), f'{what}: {err:.3e}'


def _autograd_cell(x, w1, b1, wd, bd, w2, b2):
    """NHWC in, (x leaf, t1 leaf-free, t3) through aten's convolutions in NCHW"""
    Hd = w1.shape[0]
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    t1 = F.conv2d(xn, w1[:, :, None, None], b1)
    t2 = F.conv2d(F.silu(t1), wd.t().reshape(Hd, 1, 5, 5), bd, padding=2, groups=Hd)
    t3 = F.conv2d(F.silu(t2), w2[:, :, None, None], b2)
    return xn, t1, t2, t3


@pytest.mark.parametrize('N,H,W,C,Hd,K', [(2, 5, 7, 8, 32, 1), (6, 4, 8, 16, 64, 3), (3, 8, 16, 32, 32, 1)])
def test_backward_formulas_equal_autograd(N, H, W, C, Hd, K):
    c = CR.inputs(N, H, W, C, Hd, act_rep=K)
    x, w1, b1, wd, bd, w2, b2, dout, ps, pb, add, add2 = R.f64(c.x, *c.weights, *c.cot, c.add, c.add2)
    xr = R.rep_rows(x, K)
    xn, t1, t2, t3 = _autograd_cell(xr, w1, b1, wd, bd, w2, b2)
    f1, f2, f3 = CR.cell_forward(xr, w1, b1, wd, bd, w2, b2)
    for a, b, what in ((f1, t1, 't1'), (f2, t2, 't2'), (f3, t3, 't3')):
        same(a, b.permute(0, 2, 3, 1), what)
    dt3 = (dout * ps[:, None, None, :] + pb[:, None, None, :]).permute(0, 3, 1, 2)
    gt1, gx = torch.autograd.grad((t3 * dt3).sum(), [t1, xn])
    same(CR.cell_backward(x, w1, b1, wd, bd, w2, b2, dout, ps, pb, act_rep=K), gt1.permute(0, 2, 3, 1), 'dt1')
    if K == 1:
        gx = gx.permute(0, 2, 3, 1)
        same(CR.halo_backward(x, w1, b1, wd, bd, w2, b2, dout, ps, pb), gx, 'dx')
        same(CR.halo_backward(x, w1, b1, wd, bd, w2, b2, dout, ps, pb, addend=add), gx + add, 'dx + addend')
        same(CR.halo_backward(x, w1, b1, wd, bd, w2, b2, dout, ps, pb, add, add2), gx + add + add2, 'dx + both addends')


def test_split_is_ga_split_bf16_and_the_emulation_drops_only_lo_lo():
    v = CR.g(64, 48, seed=3)
    hi, lo = CR.split_bf16(v)
    assert torch.equal(hi, v.bfloat16().float()) and torch.equal(lo, (v - hi).bfloat16().float())
    assert (v - hi - lo).abs().max().item() <= 2.0 ** -16 * v.abs().max().item()
    w = CR.g(48, 32, seed=4)
    wh, wl = CR.split_bf16(w)
    want = (lo.double() @ wh.double() + hi.double() @ wl.double()) + hi.double() @ wh.double()
    got = CR._mm_split()(v, w)
    assert (got.double() - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    dropped = CR._mm_split((1, 32))(v, w)
    assert torch.equal(dropped, (lo @ wh) + hi @ wh)            # every column is in chunk 0: the hi.lo product is gone


def test_the_library_accepts_the_expected_geometries():
    from gen_adversarial_amd import _lib as L
    assert CR.accepted_geometries(L.lib.ga_dec_cell_supported) == CR.GEOMS
    for (N, H, W, C, Hd) in CR.geometry_cases() + CR.PIPELINE_CASES + CR.SHIPPED_CASES + [c[:5] for c in CR.ACT_REP_CASES]:
        assert L.lib.ga_dec_cell_supported(N, H, W, C, Hd) == 1, (N, H, W, C, Hd)
    for (N, H, W, C, Hd) in CR.HALO_CASES + CR.HALO_DEFECT_CASES:
        assert L.lib.ga_dec_cell_halo_supported(N, H, W, C, Hd) == 1, (N, H, W, C, Hd)


def _power(what, broken, emu, ref):
    assert not CR.row_floor_decides(emu, ref), f'{what}: the 2^-22 floor decides a row'
    ratio, n, _ = CR.worst(broken, ref, CR.row_bound(emu, ref))
    print(f'{what}: emulation err {CR.row_err(emu, ref).max().item():.3e}, bound {CR.row_bound(emu, ref).max().item():.3e}, '
          f'defect err {CR.row_err(broken, ref).max().item():.3e}, defect / bound {ratio:.1f} in row {n}')
    assert ratio >= POWER, f'{what}: the injected defect reaches only {ratio:.2f} x the bound'


CELL_CASES = [(c, 1) for c in CR.geometry_cases() + CR.PIPELINE_CASES + CR.SHIPPED_CASES] + [(c[:5], 3) for c in CR.ACT_REP_CASES]


@pytest.mark.parametrize('case,K', CELL_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f'K{v}')
def test_row_bound_sees_a_missing_lo_chunk_dec_cell(case, K):
    c = CR.inputs(*case, act_rep=K)
    x64, w64, cot64 = R.f64(c.x), R.f64(*c.weights), R.f64(*c.cot)
    if K == 1:
        ref = CR.cell_forward(x64, *w64)[2]
        _power('forward', CR.emulate_forward(c.x, *c.weights, zero_lo=('w1',))[2], CR.emulate_forward(c.x, *c.weights)[2], ref)
    ref = CR.cell_backward(x64, *w64, *cot64, act_rep=K)
    _power('backward', CR.emulate_backward(c.x, *c.weights, *c.cot, act_rep=K, zero_lo=('w2t',)),
           CR.emulate_backward(c.x, *c.weights, *c.cot, act_rep=K), ref)


@pytest.mark.parametrize('case', CR.HALO_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_row_bound_sees_a_missing_lo_chunk_halo(case):
    c = CR.inputs(*case)
    x64, w64, cot64 = R.f64(c.x), R.f64(*c.weights), R.f64(*c.cot)
    _power('forward', CR.emulate_forward(c.x, *c.weights, zero_lo=('w1',))[2], CR.emulate_forward(c.x, *c.weights)[2],
           CR.cell_forward(x64, *w64)[2])
    for add, add2 in ((None, None), (c.add, c.add2)):
        ref = CR.halo_backward(x64, *w64, *cot64, R.f64(add), R.f64(add2))
        _power('backward', CR.emulate_halo_backward(c.x, *c.weights, *c.cot, add, add2, zero_lo=('w2t',)),
               CR.emulate_halo_backward(c.x, *c.weights, *c.cot, add, add2), ref)
