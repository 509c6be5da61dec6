"""A float64 interpreter of `ga_conv_desc` (include/ga_ops.h) and the element-wise error bound the conv tests assert.

conv_ref(d, t) computes what the comment above `ga_conv_desc` defines, in float64 on the device the tensors live on:

    y[n,ho,wo,co] = epi( bias[co] + sum_{kh,kw,c} w[co][(kh*KW+kw)*(C1+C2)+c] * in(n, hi, wi, c) )
    hi = (ho*sn - pad + kh) / sd            (tap skipped unless the division is exact and 0 <= hi < Hi; same for wi)
    in(.,c) = act_pro(pro_scale*x + pro_shift) for c < C1 (per channel, or per row with pro_per_row; PReLU with
              GA_CONV_PRO_PRELU), x2[., c-C1] for c >= C1
    epi(v)  = v * act'(dact_scale*dact_x + dact_shift) * dact_scale     (dact_x; GA_CONV_DACT_PRELU: v * (u > 0 ? 1 : slope))
              + addend (broadcast over n, or shared by addend_rep rows; relu'd with GA_CONV_ADDEND_RELU, added before the
              act' factor with GA_CONV_ADDEND_PRE_DACT) + addend2

`d` is anything with the descriptor's integer fields as attributes (a ctypes ConvDesc, a SimpleNamespace); the pointer
fields are ignored: `t` maps the operand names (x, x2, w, bias, pro_scale, pro_shift, addend, addend2, dact_x, dact_scale,
dact_shift) to tensors in the library's memory layout with the descriptor's pitches (ldx, ldx2, ldadd, ldadd2, lddact).
The result is [N, Ho, Wo, Cout]: channel co of pixel m is what the kernel writes at y[m * ldy + co].

Alongside it come two per-element allowances.  The ERROR SCALE is the same contraction on absolute values, sum |w| |in| +
|bias| (+ |addend| for GA_CONV_ADDEND_PRE_DACT), times the largest |act' factor| within the rounding of its argument, plus
|addend| + |addend2|.  The SLACK is what the kernel's fp32 prologue and act' evaluation may add on their own, independent of
how the contraction is done (see below).  Tests assert, element by element,

    |y - ref| <= tau * scale + slack + 2^-22 * |ref|

Derivation of tau (u = 2^-24, the fp32 unit roundoff; u_b = 2^-8, bf16's):

  split-bf16 (w_hi / w_lo given; conv_bf3, the halo tiles 5-8, tile 11).  Both operands are split, a = a_hi + a_lo + da with
  a_hi = bf16(a), a_lo = bf16(a - a_hi), so |a_lo| <= u_b |a| and |da| <= u_b^2 |a|; likewise w.  The kernel forms
  a_hi w_hi + a_lo w_hi + a_hi w_lo (each product of two bf16 is exact in fp32) and drops a_lo w_lo.  Per product the error is
  |a_lo w_lo| + |da w| + |a dw| <= 3 u_b^2 |a w| = 3 * 2^-16 |a w|: summed over K, at most 3 * 2^-16 * scale.
  Accumulation in fp32 adds at most u |S_k| per partial sum S_k.  The worst case, K u scale (1.6e-3 at K = 27648), says
  nothing; with independent rounding errors (Higham & Mary 2019) the sum is ~ u sqrt(sum_k S_k^2) / sqrt(3), and for
  zero-mean operands |S_k| ~ sqrt(k) rms(a w) while scale ~ K mean|a w|: about u of the scale at every K, a few u at the
  tail of 10^8 elements.  Budget 32 u = 2^-19.
      tau_bf3  = 3 * 2^-16 + 2^-19 = 4.77e-5
  With w_lo dropped the per-product error is |a dw_hi| <= u_b |a w| = 2^-8 |a w| with dw_hi of random sign: the max over
  a plan-sized output of a short contraction (K = 288) lands near 4e-4 of the scale, far outside tau_bf3.

  exact fp32 (conv_mfma: v_mfma_f32_32x32x2_f32).  Each product rounds at most once (u |a w|), the rest is accumulation:
      tau_fp32 = 2^-19 + 2^-24 = 1.97e-6

The slack: each input in(c) of the prologue carries 4 u (|pro_scale x| + |pro_shift|) from the fp32 affine (x 1.1, the
largest |act'|) and, for SiLU, a relative (1.5 |u| + 6) u from the fast exp (v_exp_f32 of u log2 e) and reciprocal; summed with
|w| through the contraction.  The act' factor f of the epilogue is off by df: its spread within 2^-20 of an fp32-rounded
argument (a ReLU kink), 8 u (1 + |u|) for the fast SiLU' and 4 u |f| for ELU' (expf), times |v| = |bias + sum|.  Near SiLU's
zero of act' (u = -1.2785) f is ~1e-6 while df stays ~1e-7: there |v| df is most of the error, and no multiple of the scale
would cover it.  The 2^-22 |ref| term covers the epilogue's few roundings relative to the result.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

GA_ACT_NONE, GA_ACT_SILU, GA_ACT_ELU, GA_ACT_RELU, GA_ACT_LRELU = 0, 1, 2, 3, 4
GA_CONV_ADDEND_RELU, GA_CONV_ADDEND_PRE_DACT, GA_CONV_PRO_PRELU, GA_CONV_DACT_PRELU = 1, 2, 4, 8

TAU_BF3 = 3 * 2.0 ** -16 + 2.0 ** -19
TAU_FP32 = 2.0 ** -19 + 2.0 ** -24
REL_EPI = 2.0 ** -22
ARG_EPS = 2.0 ** -20        # relative rounding of an act' argument u = dact_scale * dact_x + dact_shift computed in fp32

__all__ = ['conv_ref', 'act', 'act_grad', 'bound_ratio', 'TAU_BF3', 'TAU_FP32', 'REL_EPI']


def act(u: torch.Tensor, a: int) -> torch.Tensor:
    if a == GA_ACT_SILU:
        return u * torch.sigmoid(u)
    if a == GA_ACT_ELU:
        return torch.where(u > 0, u, torch.expm1(u))
    if a == GA_ACT_RELU:
        return u.clamp_min(0)
    if a == GA_ACT_LRELU:
        return torch.where(u > 0, u, 0.01 * u)
    assert a == GA_ACT_NONE, a
    return u


def act_grad(u: torch.Tensor, a: int) -> torch.Tensor:
    if a == GA_ACT_SILU:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if a == GA_ACT_ELU:
        return torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    if a == GA_ACT_RELU:
        return (u > 0).to(u.dtype)
    if a == GA_ACT_LRELU:
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.01))
    assert a == GA_ACT_NONE, a
    return torch.ones_like(u)


def _rows(t: torch.Tensor, rows: int, ld: int, c: int) -> torch.Tensor:
    """the first c channels of `rows` pixels stored with pitch ld, as float64 [rows, c]"""
    flat = t.reshape(-1)
    need = rows * ld
    if flat.numel() < need:                 # the last pixel needs only its first c channels
        flat = torch.cat([flat, flat.new_zeros(need - flat.numel())])
    return flat[:need].view(rows, ld)[:, :c].double()


def _conv(inp: torch.Tensor, w4: torch.Tensor, d) -> torch.Tensor:
    """inp [N, C, Hi, Wi], w4 [Cout, C, KH, KW] -> [N, Cout, Ho, Wo] with the tap rule hi = (ho*sn - pad + kh) / sd"""
    sd, sn, pad = d.sd, d.sn, d.pad
    if sd > 1:          # zero-insertion: position j of the dilated input is in[j / sd] when sd | j, else 0
        n, c, h, w = inp.shape
        up = inp.new_zeros(n, c, h * sd, w * sd)
        up[:, :, ::sd, ::sd] = inp
        inp = up
    hu, wu = inp.shape[2], inp.shape[3]
    # dilated-input rows read: ho*sn - pad + kh for ho < Ho, kh < KH; out-of-range rows are zero
    need_h, need_w = (d.Ho - 1) * sn + d.KH - pad, (d.Wo - 1) * sn + d.KW - pad
    inp = F.pad(inp, (pad, max(0, need_w - wu), pad, max(0, need_h - hu)))
    inp = inp[:, :, :pad + need_h, :pad + need_w]
    return F.conv2d(inp, w4, stride=sn)[:, :, :d.Ho, :d.Wo]


def conv_ref(d, t: dict):
    """(ref, scale, slack), float64 [N, Ho, Wo, Cout] on the device of t['x']"""
    N, Hi, Wi, C1, C2, Cout = d.N, d.Hi, d.Wi, d.C1, d.C2, d.Cout
    Ho, Wo, KH, KW = d.Ho, d.Wo, d.KH, d.KW
    flags = d.flags
    P_in, P_out = N * Hi * Wi, N * Ho * Wo
    x = _rows(t['x'], P_in, d.ldx, C1).view(N, Hi * Wi, C1)
    err_in = torch.zeros_like(x)                    # absolute rounding allowance of the prologue's fp32 affine
    if t.get('pro_scale') is not None:
        s = t['pro_scale'].double().reshape(-1)
        b = t['pro_shift'].double().reshape(-1)
        if flags & GA_CONV_PRO_PRELU:
            x = torch.where(x > 0, x, x * s[:C1])
        else:
            s, b = (s[:N * C1].view(N, 1, C1), b[:N * C1].view(N, 1, C1)) if d.pro_per_row else (s[:C1], b[:C1])
            err_in = 2.0 ** -22 * ((x * s).abs() + b.abs())
            x = x * s + b
    a = act(x, d.pro_act)
    err_in = err_in * 1.1                           # |act'| <= 1.1
    if d.pro_act == GA_ACT_SILU:
        err_in = err_in + 2.0 ** -24 * (1.5 * x.abs() + 6) * a.abs()
    parts, parts_abs, parts_err = [a], [a.abs()], [err_in]
    if C2 > 0:
        x2 = _rows(t['x2'], P_in, d.ldx2, C2).view(N, Hi * Wi, C2)
        parts.append(x2)
        parts_abs.append(x2.abs())
        parts_err.append(torch.zeros_like(x2))

    def nchw(p):
        return torch.cat(p, 2).view(N, Hi, Wi, C1 + C2).permute(0, 3, 1, 2)
    w4 = t['w'].double().reshape(Cout, KH, KW, C1 + C2).permute(0, 3, 1, 2)
    v = _conv(nchw(parts), w4, d).permute(0, 2, 3, 1).reshape(P_out, Cout)
    sc = _conv(nchw(parts_abs), w4.abs(), d).permute(0, 2, 3, 1).reshape(P_out, Cout)
    # the prologue's own rounding, carried through the contraction: an absolute allowance, not a multiple of tau
    slack = _conv(nchw(parts_err), w4.abs(), d).permute(0, 2, 3, 1).reshape(P_out, Cout) if bool(err_in.any()) else torch.zeros_like(v)
    if t.get('bias') is not None:
        bias = t['bias'].double().reshape(-1)[:Cout]
        v = v + bias
        sc = sc + bias.abs()

    HoWo = Ho * Wo
    addend = None
    if t.get('addend') is not None:
        if d.addend_bcast_n:
            addend = _rows(t['addend'], HoWo, d.ldadd, Cout).repeat(N, 1)
        else:
            rep = d.addend_rep if d.addend_rep > 1 else 1
            addend = _rows(t['addend'], P_out // rep, d.ldadd, Cout).view(N // rep, HoWo, Cout)
            addend = addend.repeat_interleave(rep, 0).reshape(P_out, Cout)
        if flags & GA_CONV_ADDEND_RELU:
            addend = addend.clamp_min(0)
    pre = bool(flags & GA_CONV_ADDEND_PRE_DACT) and addend is not None
    if pre:
        v = v + addend
        sc = sc + addend.abs()
    if t.get('dact_x') is not None:
        rep = d.dact_rep if d.dact_rep > 1 else 1
        u = _rows(t['dact_x'], P_out // rep, d.lddact, Cout).view(N // rep, HoWo, Cout)
        u = u.repeat_interleave(rep, 0).reshape(P_out, Cout)
        ds = t['dact_scale'].double().reshape(-1)[:Cout] if t.get('dact_scale') is not None else None
        if flags & GA_CONV_DACT_PRELU:          # the sign test on the stored dact_x is exact
            f = torch.where(u > 0, torch.ones_like(u), ds.expand_as(u))
            f_abs, df = f.abs(), torch.zeros_like(u)
        else:
            if ds is not None:                  # u = dact_scale * dact_x + dact_shift is rounded to fp32 in the kernel
                db = t['dact_shift'].double().reshape(-1)[:Cout]
                eps = ARG_EPS * ((u * ds).abs() + db.abs())
                u = u * ds + db
            else:
                ds, eps = torch.ones(Cout, dtype=u.dtype, device=u.device), torch.zeros_like(u)
            g0, gm, gp = (act_grad(u, d.dact_act), act_grad(u - eps, d.dact_act), act_grad(u + eps, d.dact_act))
            f = g0 * ds
            # the scale takes the largest |act'| within the rounding of its argument; the factor's own error (a ReLU kink
            # crossed under an fp32 argument, the fast sigmoid of SiLU', expf of ELU') is an absolute allowance |v| df
            f_abs = torch.maximum(torch.maximum(gm.abs(), gp.abs()), g0.abs()) * ds.abs()
            df = torch.maximum(torch.maximum(gm, gp), g0) - torch.minimum(torch.minimum(gm, gp), g0)
            if d.dact_act == GA_ACT_SILU:
                df = df + 2.0 ** -21 * (1 + u.abs())
            elif d.dact_act == GA_ACT_ELU:
                df = df + 2.0 ** -22 * g0.abs()
            df = df * ds.abs()
        slack = slack * f_abs + (v.abs() + 2 * TAU_BF3 * sc) * df
        v = v * f
        sc = sc * f_abs
    if addend is not None and not pre:
        v = v + addend
        sc = sc + addend.abs()
    if t.get('addend2') is not None:
        a2 = _rows(t['addend2'], P_out, d.ldadd2, Cout)
        v = v + a2
        sc = sc + a2.abs()
    shape = (N, Ho, Wo, Cout)
    return v.view(shape), sc.view(shape), slack.view(shape)


def bound_ratio(y: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, slack: torch.Tensor, tau: float):
    """(max over elements of |y - ref| / (tau * scale + slack + 2^-22 |ref|), max of (|y - ref| - slack - 2^-22 |ref|) / scale):
    the first is <= 1 when the bound holds everywhere, the second is the part of tau the contraction used; NaN / inf in y count
    as unbounded"""
    y = y.double()
    err = (y - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    fixed = slack + REL_EPI * ref.abs()
    r = (err / (tau * scale + fixed).clamp_min(1e-300)).max().item()
    e = ((err - fixed).clamp_min(0) / scale.clamp_min(1e-300)).max().item()
    return r, e
