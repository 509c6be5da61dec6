"""CPU: the float64 descriptor interpreter of tests/convref.py against the same operation composed from F.conv2d /
F.conv_transpose2d and explicit activations, one test per form of ga_conv_desc (include/ga_ops.h)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import convref as R

ACTS = {0: lambda u: u, 1: F.silu, 2: F.elu, 3: F.relu, 4: lambda u: F.leaky_relu(u, 0.01)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pitched(t, ld):
    """NCHW float64 -> NHWC with channel pitch ld; the pitch padding is NaN so that reading it poisons the result"""
    n, c, h, w = t.shape
    out = torch.full((n, h, w, ld), float('nan'), dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def _desc(**kw):
    base = dict(C2=0, sn=1, sd=1, pad=0, pro_act=0, pro_per_row=0, dact_act=0, addend_bcast_n=0, dact_rep=0, addend_rep=0,
                flags=0, ldx2=0, ldadd=0, ldadd2=0, lddact=0)
    base.update(kw)
    return SimpleNamespace(**base)


def _wflat(w):
    """[Cout, C, KH, KW] -> the library layout [Cout][(kh * KW + kw) * C + c]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def _check(d, t, want):
    ref, scale, slack = R.conv_ref(d, t)
    want = want.permute(0, 2, 3, 1)
    assert ref.shape == want.shape, (tuple(ref.shape), tuple(want.shape))
    assert torch.isfinite(ref).all() and torch.isfinite(scale).all() and (slack >= 0).all()
    err = (ref - want).abs().max().item()
    assert err <= 1e-12 * max(1.0, want.abs().max().item()), err
    assert (ref.abs() <= scale * (1 + 1e-12)).all()            # the error scale dominates the result it bounds
    return ref, scale


@pytest.mark.parametrize('act', [0, 1, 2, 3, 4])
def test_strided_forward_with_affine_prologue(act):
    g = _gen(act)
    N, C1, H, W, Cout, K = 2, 5, 9, 7, 6, 3
    x = torch.randn(N, C1, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C1, K, K, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    s, sh = torch.rand(C1, generator=g, dtype=torch.float64) + 0.5, torch.randn(C1, generator=g, dtype=torch.float64)
    want = F.conv2d(ACTS[act](x * s.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), w, b, stride=2, padding=1)
    d = _desc(N=N, Hi=H, Wi=W, C1=C1, Cout=Cout, Ho=want.shape[2], Wo=want.shape[3], KH=K, KW=K, sn=2, pad=1, ldx=8, pro_act=act)
    _check(d, dict(x=_pitched(x, 8), w=_wflat(w), bias=b, pro_scale=s, pro_shift=sh), want)


def test_plain_conv_error_scale_is_the_absolute_contraction():
    g = _gen(1)
    x = torch.randn(1, 4, 6, 6, generator=g, dtype=torch.float64)
    w = torch.randn(3, 4, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(3, generator=g, dtype=torch.float64)
    d = _desc(N=1, Hi=6, Wi=6, C1=4, Cout=3, Ho=6, Wo=6, KH=3, KW=3, pad=1, ldx=4)
    _, scale = _check(d, dict(x=_pitched(x, 4), w=_wflat(w), bias=b), F.conv2d(x, w, b, padding=1))
    want = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(scale, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize('k,pad_f,out_pad', [(3, 1, 1), (4, 1, 0), (1, 0, 1)])
def test_transposed_conv_with_flipped_weights(k, pad_f, out_pad):
    """sn = 1, sd = 2: the backward-to-input of a stride-2 conv (weights flipped and transposed, pad = K - 1 - pad_f)"""
    g = _gen(k)
    N, Cf_in, Cf_out, h = 2, 5, 7, 4
    wf = torch.randn(Cf_out, Cf_in, k, k, generator=g, dtype=torch.float64)
    cot = torch.randn(N, Cf_out, h, h + 1, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(cot, wf, stride=2, padding=pad_f, output_padding=out_pad)
    wd = wf.flip(2, 3).permute(1, 0, 2, 3)          # [Cf_in][Cf_out][kh][kw]
    d = _desc(N=N, Hi=h, Wi=h + 1, C1=Cf_out, Cout=Cf_in, Ho=want.shape[2], Wo=want.shape[3], KH=k, KW=k, sd=2,
              pad=k - 1 - pad_f, ldx=Cf_out + 1)
    _check(d, dict(x=_pitched(cot, Cf_out + 1), w=_wflat(wd)), want)


def test_dual_source_prologue_on_source_one_only():
    g = _gen(3)
    N, C1, C2, H, Cout = 2, 4, 6, 5, 3
    x = torch.randn(N, C1, H, H, generator=g, dtype=torch.float64)
    x2 = torch.randn(N, C2, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C1 + C2, 3, 3, generator=g, dtype=torch.float64)
    s, sh = torch.rand(C1, generator=g, dtype=torch.float64) + 0.5, torch.randn(C1, generator=g, dtype=torch.float64)
    want = F.conv2d(torch.cat([F.silu(x * s.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), x2], 1), w, padding=1)
    d = _desc(N=N, Hi=H, Wi=H, C1=C1, C2=C2, Cout=Cout, Ho=H, Wo=H, KH=3, KW=3, pad=1, ldx=C1, ldx2=C2 + 2, pro_act=1)
    _check(d, dict(x=_pitched(x, C1), x2=_pitched(x2, C2 + 2), w=_wflat(w), pro_scale=s, pro_shift=sh), want)


def test_per_row_prologue():
    g = _gen(4)
    N, C1, H, Cout = 3, 4, 4, 5
    x = torch.randn(N, C1, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C1, 1, 1, generator=g, dtype=torch.float64)
    s, sh = torch.rand(N, C1, generator=g, dtype=torch.float64) + 0.5, torch.randn(N, C1, generator=g, dtype=torch.float64)
    want = F.conv2d(F.elu(x * s.view(N, C1, 1, 1) + sh.view(N, C1, 1, 1)), w)
    d = _desc(N=N, Hi=H, Wi=H, C1=C1, Cout=Cout, Ho=H, Wo=H, KH=1, KW=1, ldx=C1, pro_act=2, pro_per_row=1)
    _check(d, dict(x=_pitched(x, C1), w=_wflat(w), pro_scale=s, pro_shift=sh), want)


def test_prelu_prologue_and_prelu_derivative_epilogue():
    g = _gen(5)
    N, C, H, Cout = 2, 6, 5, 4
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64)
    slope = torch.rand(C, generator=g, dtype=torch.float64) - 0.3
    want = F.conv2d(F.prelu(x, slope), w, padding=1)
    d = _desc(N=N, Hi=H, Wi=H, C1=C, Cout=Cout, Ho=H, Wo=H, KH=3, KW=3, pad=1, ldx=C, flags=R.GA_CONV_PRO_PRELU)
    _check(d, dict(x=_pitched(x, C), w=_wflat(w), pro_scale=slope, pro_shift=slope), want)
    # epilogue: the cotangent of PReLU's input, y = conv(cot) * (u > 0 ? 1 : slope)
    cot = torch.randn(N, Cout, H, H, generator=g, dtype=torch.float64)
    u = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    ur = u.clone().requires_grad_(True)
    (fac,) = torch.autograd.grad(F.prelu(ur, slope).sum(), [ur])
    wb = w.flip(2, 3).permute(1, 0, 2, 3)
    want = F.conv2d(cot, wb, padding=1) * fac
    d = _desc(N=N, Hi=H, Wi=H, C1=Cout, Cout=C, Ho=H, Wo=H, KH=3, KW=3, pad=1, ldx=Cout, lddact=C + 3, flags=R.GA_CONV_DACT_PRELU)
    _check(d, dict(x=_pitched(cot, Cout), w=_wflat(wb), dact_x=_pitched(u, C + 3), dact_scale=slope, dact_shift=slope), want)


@pytest.mark.parametrize('act', [1, 2, 3, 4])
@pytest.mark.parametrize('affine', [False, True])
def test_act_derivative_epilogue(act, affine):
    """y = conv * act'(dact_scale * u + dact_shift) * dact_scale: d/du act(dact_scale * u + dact_shift), by autograd"""
    g = _gen(10 * act + affine)
    N, C, H, Cout = 2, 5, 4, 6
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    u = torch.randn(N, Cout, H, H, generator=g, dtype=torch.float64)
    ds, db = torch.rand(Cout, generator=g, dtype=torch.float64) + 0.5, torch.randn(Cout, generator=g, dtype=torch.float64)
    ur = u.clone().requires_grad_(True)
    arg = ur * ds.view(1, -1, 1, 1) + db.view(1, -1, 1, 1) if affine else ur
    (fac,) = torch.autograd.grad(ACTS[act](arg).sum(), [ur])
    want = F.conv2d(x, w, b, padding=1) * fac
    d = _desc(N=N, Hi=H, Wi=H, C1=C, Cout=Cout, Ho=H, Wo=H, KH=3, KW=3, pad=1, ldx=C, lddact=Cout, dact_act=act)
    t = dict(x=_pitched(x, C), w=_wflat(w), bias=b, dact_x=_pitched(u, Cout))
    if affine:
        t.update(dact_scale=ds, dact_shift=db)
    _check(d, t, want)


def test_residual_flags():
    """GA_CONV_ADDEND_RELU: y = conv + relu(addend); GA_CONV_ADDEND_PRE_DACT: y = (conv + addend) * act'(u) + addend2"""
    g = _gen(6)
    N, C, H, Cout = 2, 8, 4, 5
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C, 1, 1, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    a = torch.randn(N, Cout, H, H, generator=g, dtype=torch.float64)
    a2 = torch.randn(N, Cout, H, H, generator=g, dtype=torch.float64)
    u = torch.randn(N, Cout, H, H, generator=g, dtype=torch.float64)
    conv = F.conv2d(x, w, b)
    base = dict(N=N, Hi=H, Wi=H, C1=C, Cout=Cout, Ho=H, Wo=H, KH=1, KW=1, ldx=C, ldadd=Cout + 1)
    _check(_desc(**base, flags=R.GA_CONV_ADDEND_RELU), dict(x=_pitched(x, C), w=_wflat(w), bias=b, addend=_pitched(a, Cout + 1)),
           conv + F.relu(a))
    d = _desc(**base, flags=R.GA_CONV_ADDEND_PRE_DACT, dact_act=3, lddact=Cout, ldadd2=Cout + 2)
    _check(d, dict(x=_pitched(x, C), w=_wflat(w), bias=b, addend=_pitched(a, Cout + 1), dact_x=_pitched(u, Cout),
                   addend2=_pitched(a2, Cout + 2)), (conv + a) * (u > 0).double() + a2)


def test_broadcast_addend_addend_rep_and_dact_rep():
    g = _gen(7)
    N, rep, C, H, Cout = 6, 3, 4, 4, 5
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, C, 3, 3, generator=g, dtype=torch.float64)
    conv = F.conv2d(x, w, padding=1)
    base = dict(N=N, Hi=H, Wi=H, C1=C, Cout=Cout, Ho=H, Wo=H, KH=3, KW=3, pad=1, ldx=C)
    t = dict(x=_pitched(x, C), w=_wflat(w))
    ab = torch.randn(1, Cout, H, H, generator=g, dtype=torch.float64)           # one [Ho, Wo, ldadd] map for every row
    _check(_desc(**base, addend_bcast_n=1, ldadd=Cout), dict(t, addend=_pitched(ab, Cout)), conv + ab)
    ar = torch.randn(N // rep, Cout, H, H, generator=g, dtype=torch.float64)    # row n reads addend row n / rep
    _check(_desc(**base, addend_rep=rep, ldadd=Cout + 4), dict(t, addend=_pitched(ar, Cout + 4)), conv + ar.repeat_interleave(rep, 0))
    u = torch.randn(N // rep, Cout, H, H, generator=g, dtype=torch.float64)     # row n reads dact_x row n / rep
    want = conv * (u.repeat_interleave(rep, 0) > 0).double() + ar.repeat_interleave(rep, 0)
    _check(_desc(**base, dact_rep=rep, dact_act=3, lddact=Cout, addend_rep=rep, ldadd=Cout + 4),
           dict(t, dact_x=_pitched(u, Cout), addend=_pitched(ar, Cout + 4)), want)


def test_bound_ratio_flags_nan_and_errors_beyond_tau():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    scale = torch.tensor([4.0, 2.0, 1.0], dtype=torch.float64)
    slack = torch.zeros(3, dtype=torch.float64)
    r, _ = R.bound_ratio(ref.float(), ref, scale, slack, R.TAU_FP32)
    assert r == 0.0
    bad = ref.clone()
    bad[1] += 3 * R.TAU_BF3 * 2.0
    r, e = R.bound_ratio(bad, ref, scale, slack, R.TAU_BF3)
    assert r > 2.5 and e > 2.5 * R.TAU_BF3
    assert R.bound_ratio(bad, ref, scale, slack + 6 * R.TAU_BF3, R.TAU_BF3)[0] < 1
    assert R.bound_ratio(torch.tensor([1.0, float('nan'), 0.0]), ref, scale, slack, R.TAU_BF3)[0] == float('inf')


def test_silu_derivative_zero_is_covered_by_the_slack_not_by_tau():
    """near u = -1.2785 SiLU' is ~0: the fp32 factor's absolute error times |v| is absorbed by the slack, and a lost lo term
    elsewhere still breaks the bound"""
    u0 = -1.2784645427610738
    d = _desc(N=1, Hi=1, Wi=1, C1=4, Cout=2, Ho=1, Wo=1, KH=1, KW=1, ldx=4, lddact=2, dact_act=1)
    x = torch.tensor([[[[3.0]], [[-2.0]], [[1.0]], [[0.5]]]], dtype=torch.float64)
    w = torch.ones(2, 4, dtype=torch.float64)
    u = torch.tensor([[[[u0]], [[0.3]]]], dtype=torch.float64)
    ref, scale, slack = R.conv_ref(d, dict(x=_pitched(x, 4), w=w, dact_x=_pitched(u, 2)))
    assert abs(ref[0, 0, 0, 0].item()) < 1e-12 and slack[0, 0, 0, 0] > 1e-7 * 2.5
    y = ref.clone()
    y[0, 0, 0, 0] += 2.5 * 1e-7                                    # |v| = 2.5, factor off by 1e-7
    assert R.bound_ratio(y, ref, scale, slack, R.TAU_FP32)[0] <= 1
    y[0, 0, 0, 1] += 2.0 ** -9 * scale[0, 0, 0, 1]
    assert R.bound_ratio(y, ref, scale, slack, R.TAU_BF3)[0] > 1
