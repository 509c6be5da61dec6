"""
Plain references of the element-wise / reduction entry points of include/ga_ops.h, written from the header's formulas (not
from the kernels).  No GPU, no library: CPU tensors in, CPU tensors out.

Every function computes in the dtype of its inputs: float64 inputs give the reference, float32 inputs give "the same formula
in plain fp32 PyTorch", whose distance to the float64 result is what the GPU tests derive their bounds from (bound()).
Activations are dense NHWC ([N,H,W,C] or [N,P,C]); pitches (ld, ldz, lds, ld_planes, ld_img) and the space-to-depth layouts
are the business of the pack / unpack helpers at the end, so that a test can hand the kernel pitched buffers and the
reference dense ones.  Replica fields are literal: `rep_rows(t, K)` makes cotangent row n read forward row n // K.
"""
import torch
import torch.nn.functional as F

SQRT2 = 2.0 ** 0.5
NONE, SILU, ELU, RELU, LRELU, FLRELU = range(6)


def f64(*ts):
    out = tuple(None if t is None else t.detach().double() for t in ts)
    return out[0] if len(out) == 1 else out


def rep_rows(t, K):
    """[N/K, ...] -> [N, ...]: row n is forward row n // K"""
    return t if K <= 1 else t.repeat_interleave(K, dim=0)


def act(u, a):
    if a == SILU:
        return u * torch.sigmoid(u)
    if a == ELU:
        return torch.where(u > 0, u, torch.expm1(u))
    if a == RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if a == LRELU:
        return torch.where(u > 0, u, 0.01 * u)
    if a == FLRELU:
        return torch.where(u > 0, u, 0.2 * u) * SQRT2
    return u


def dact(u, a):
    """d act / du; at the kink the slope branch is taken (u > 0 ? 1 : slope)"""
    one = torch.ones_like(u)
    if a == SILU:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if a == ELU:
        return torch.where(u > 0, one, torch.exp(u))
    if a == RELU:
        return torch.where(u > 0, one, 0 * one)
    if a == LRELU:
        return torch.where(u > 0, one, 0.01 * one)
    if a == FLRELU:
        return torch.where(u > 0, one, 0.2 * one) * SQRT2
    return one


# ---------------------------------------------------------------------------------------------------- ga_dwconv5
def up2_nearest(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def pool2_sum(y):
    N, H, W, C = y.shape
    return y.reshape(N, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))


def dwconv5(x, w, bias=None, dact_x=None, pro_act=NONE, dact_act=NONE, up2=False, pool2=False, act_rep=1):
    """y = [pool2] (bias + dw5(up2(act(x)))) * act'(dact_x row n // act_rep); w: [25][C] tap-major, tap (kh, kw) reads pixel
    (h + kh - 2, w + kw - 2), zero outside the image"""
    a = act(x, pro_act)
    if up2:
        a = up2_nearest(a)
    N, H, W, C = a.shape
    ap = F.pad(a, (0, 0, 2, 2, 2, 2))
    y = torch.zeros_like(a)
    for kh in range(5):
        for kw in range(5):
            y = y + w[kh * 5 + kw] * ap[:, kh:kh + H, kw:kw + W]
    if pool2:
        assert bias is None
        y = pool2_sum(y)
    if bias is not None:
        y = y + bias
    if dact_x is not None:
        y = y * dact(rep_rows(dact_x, act_rep), dact_act)
    return y


# ---------------------------------------------------------------------------------------------------- squeeze and excite
def se_excite_fwd(m, w1, b1, w2, b2):
    hid = m @ w1.t() + b1
    return hid, torch.sigmoid(act(hid, RELU) @ w2.t() + b2)


def se_excite_bwd(dgate, hid, gate, w1, w2, res_scale, P):
    """the unfused backward: dgate [N,C] (already d / d gate) -> pro_scale = res_scale * gate, pro_shift = d m / P"""
    ds = dgate * gate * (1 - gate)
    dh = (ds @ w2) * (hid > 0).to(ds.dtype)
    return res_scale * gate, (dh @ w1) / P


def se_excite_bwd_fused(t, dout, hid, gate, w1, w2, res_scale, act_rep=1):
    """t [N/K,P,C], dout [N,P,C] -> pro_scale, pro_shift [N,C]: d t = dout * pro_scale + pro_shift"""
    tr, hr, gr = rep_rows(t, act_rep), rep_rows(hid, act_rep), rep_rows(gate, act_rep)
    P = t.shape[1]
    dgate = res_scale * (dout * tr).sum(dim=1)
    ds = dgate * gr * (1 - gr)
    dh = (ds @ w2) * (hr > 0).to(ds.dtype)
    return res_scale * gr, (dh @ w1) / P


def bilinear_up2(x):
    """[N,h,w,C] -> [N,2h,2w,C], align_corners=True"""
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1)


def bilinear_up2_adjoint(dhigh):
    N, H, W, C = dhigh.shape
    lo = torch.zeros(N, H // 2, W // 2, C, dtype=dhigh.dtype, requires_grad=True)
    (g,) = torch.autograd.grad((bilinear_up2(lo) * dhigh).sum(), [lo])
    return g


def se_apply(skip, t, gate, res_scale, skip_mode=0):
    N, H, W, C = t.shape
    if skip is None:
        s = torch.zeros_like(t)
    elif skip_mode == 0:
        s = skip
    elif skip_mode == 1:
        s = bilinear_up2(skip)
    else:
        s = skip[:, ::2, ::2]
    return s + res_scale * gate.view(N, 1, 1, C) * t


# ---------------------------------------------------------------------------------------------------- ga_sampler_mix, mode 1
def _sc5(v):
    return 5 * torch.tanh(v / 5)


def sampler_nd(mu_q, p, eps):
    """mu_q, p: [N,h,w,2NL] = (mu | logsig); eps [N,h,w,NL] (NHWC)"""
    NL = eps.shape[-1]
    return _sc5(mu_q[..., :NL] + p[..., :NL]) + (torch.exp(_sc5(mu_q[..., NL:] + p[..., NL:])) + 0.01) * eps


def sampler_nd_bwd(mu_q, p, eps, dz, act_rep=1):
    """-> d (mu | logsig) [N,h,w,2NL], the same for mu_q and p"""
    NL = eps.shape[-1]
    mu_q, p, eps = rep_rows(mu_q, act_rep), rep_rows(p, act_rep), rep_rows(eps, act_rep)
    ms, ls = mu_q[..., :NL] + p[..., :NL], mu_q[..., NL:] + p[..., NL:]
    dmu = dz * (1 - torch.tanh(ms / 5) ** 2)
    dls = dz * eps * torch.exp(_sc5(ls)) * (1 - torch.tanh(ls / 5) ** 2)
    return torch.cat([dmu, dls], dim=-1)


# ---------------------------------------------------------------------------------------------------- ga_sampler_mix, mode 0
def sampler_mix(mu_q, mu_p, logsig_p, eps, alpha, one_minus_alpha, temp):
    """z = (1 - alpha) enc_mu + alpha (eps * sigma + dec_mu); all [N,h,w,NL], rows already expanded; mu_p None: the prior N(0, 1)
    of the first group (logsig_p is then zeros).  alpha / one_minus_alpha: floats or [N,1,1,1]"""
    mp = torch.zeros_like(mu_q) if mu_p is None else mu_p
    sigma = temp * torch.exp(_sc5(logsig_p))
    return one_minus_alpha * _sc5(mp + mu_q) + alpha * (eps * sigma + _sc5(mp))


def sampler_mix_bwd(mu_q, mu_p, logsig_p, eps, dz, alpha, one_minus_alpha, temp):
    """-> d mu_q, d mu_p, d logsig_p, each [N,h,w,NL] per (cotangent) row; mu_p None as in sampler_mix"""
    mp = torch.zeros_like(mu_q) if mu_p is None else mu_p
    sech2 = lambda v: 1 - torch.tanh(v / 5) ** 2
    denc = one_minus_alpha * dz * sech2(mp + mu_q)
    dmp = denc + alpha * dz * sech2(mp)
    dls = alpha * dz * eps * temp * torch.exp(_sc5(logsig_p)) * sech2(logsig_p)
    return denc, dmp, dls


# ---------------------------------------------------------------------------------------------------- ga_sampler_mix, mode 2
def sampler_alpha_terms(mu_q, mu_p, logsig_p, eps, dz, temp):
    """the terms of d loss / d alpha: dz * (eps * sigma + dec_mu - enc_mu), [N,h,w,NL], operands as in sampler_mix; row n's
    cotangent of alpha is their sum"""
    mp = torch.zeros_like(mu_q) if mu_p is None else mu_p
    return dz * (eps * (temp * torch.exp(_sc5(logsig_p))) + _sc5(mp) - _sc5(mp + mu_q))


# ---------------------------------------------------------------------------------------------------- ga_dml_mean
def _dml_parts(l, nmix):
    p = torch.softmax(l[..., :nmix], dim=-1)
    q = l[..., nmix:10 * nmix].reshape(*l.shape[:-1], nmix, 9)
    mu = (q[..., 0:3] * p[..., None]).sum(dim=-2)
    th = torch.tanh(q[..., 6:9])
    K = (th * p[..., None]).sum(dim=-2)
    r = mu[..., 0].clamp(-1, 1)
    gpre = mu[..., 1] + K[..., 0] * r
    g = gpre.clamp(-1, 1)
    bpre = mu[..., 2] + K[..., 1] * r + K[..., 2] * g
    return p, q, th, mu, K, r, gpre, g, bpre


def dml_mean(logits, nmix):
    """logits [N,H,W,ld] -> image [N,H,W,3] in [0, 1]"""
    *_, r, _, g, bpre = _dml_parts(logits, nmix)
    return torch.stack([r, g, bpre.clamp(-1, 1)], dim=-1) * 0.5 + 0.5


def dml_pre(logits, nmix):
    """the three clamp inputs (kink sites at -1 and 1)"""
    _, _, _, mu, _, _, gpre, _, bpre = _dml_parts(logits, nmix)
    return torch.stack([mu[..., 0], gpre, bpre], dim=-1)


def dml_mean_bwd(logits, nmix, dimg, act_rep=1):
    """dimg [N,H,W,3] (the sum of the NHWC and NCHW cotangents) -> dlogits [N,H,W,ld], all ld channels (pad ones zero)"""
    l = rep_rows(logits, act_rep)
    p, q, th, mu, K, r, gpre, g, bpre = _dml_parts(l, nmix)
    inside = lambda v: ((v >= -1) & (v <= 1)).to(l.dtype)
    d = 0.5 * dimg
    dbp = d[..., 2] * inside(bpre)
    dr = d[..., 0] + dbp * K[..., 1]
    dg = d[..., 1] + dbp * K[..., 2]
    dgp = dg * inside(gpre)
    dr = dr + dgp * K[..., 0]
    dmu = torch.stack([dr * inside(mu[..., 0]), dgp, dbp], dim=-1)
    dK = torch.stack([dgp * r, dbp * r, dbp * g], dim=-1)
    dpk = (q[..., 0:3] * dmu[..., None, :]).sum(-1) + (th * dK[..., None, :]).sum(-1)
    dot = (p * dpk).sum(-1, keepdim=True)
    dq = torch.zeros_like(q)
    dq[..., 0:3] = p[..., None] * dmu[..., None, :]
    dq[..., 6:9] = p[..., None] * dK[..., None, :] * (1 - th * th)
    out = torch.zeros_like(l)
    out[..., :nmix] = p * (dpk - dot)
    out[..., nmix:10 * nmix] = dq.reshape(*l.shape[:-1], 9 * nmix)
    return out


# ---------------------------------------------------------------------------------------------------- max pools
def _win2(x):
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def maxpool2(x):
    a, b, c, e = _win2(x)
    return torch.maximum(torch.maximum(a, b), torch.maximum(c, e))


def maxpool2_bwd(x, dy, act_rep=1):
    """dy goes to the first maximal element in (h, w) scan order of the forward row n // act_rep"""
    a, b, c, e = _win2(rep_rows(x, act_rep))
    m, w = a, torch.zeros_like(a, dtype=torch.long)
    for k, v in ((1, b), (2, c), (3, e)):
        take = v > m
        m, w = torch.where(take, v, m), torch.where(take, torch.full_like(w, k), w)
    N, Ho, Wo, C = dy.shape
    dx = torch.zeros(N, 2 * Ho, 2 * Wo, C, dtype=dy.dtype)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, i::2, j::2] = torch.where(w == k, dy, torch.zeros_like(dy))
    return dx


def maxpool2_gap(x):
    """largest minus second largest element of every window (a gradient routing decision is a near-tie when this is small)"""
    s = torch.stack(_win2(x), dim=-1).sort(dim=-1).values
    return s[..., 3] - s[..., 2]


def maxpool3s2(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------- ga_interleave2
def interleave2(s, N, H, W, C, dact_x=None, dact_scale=None, dact_shift=None, addend=None, addend2=None, dact_act=NONE,
                dact_prelu=False, dact_rep=1, dtype=torch.float64):
    """s: four planes [N,H/2,W/2,C] or None, index 2a + b for output parity (a, b)"""
    y = torch.zeros(N, H, W, C, dtype=dtype)
    for a in (0, 1):
        for b in (0, 1):
            if s[2 * a + b] is not None:
                y[:, a::2, b::2] = s[2 * a + b]
    if dact_x is not None:
        u = rep_rows(dact_x, dact_rep)
        if dact_prelu:
            y = y * torch.where(u > 0, torch.ones_like(u), dact_scale.expand_as(u))
        elif dact_scale is not None:
            y = y * dact(u * dact_scale + dact_shift, dact_act) * dact_scale
        else:
            y = y * dact(u, dact_act)
    if addend is not None:
        y = y + addend
    if addend2 is not None:
        y = y + addend2
    return y


# ---------------------------------------------------------------------------------------------------- ga_image_io
def image_pre(x_nchw, noise, coef, rep):
    """[N,C,H,W]: x[n // rep] + noise[n] * coef[n] before the clamp"""
    v = rep_rows(x_nchw, rep)
    if noise is not None:
        v = v + noise * coef.view(-1, 1, 1, 1)
    return v


def image_io(x_nchw, noise, coef, rep):
    """-> dense NHWC [N,H,W,C]"""
    return image_pre(x_nchw, noise, coef, rep).clamp(0, 1).permute(0, 2, 3, 1)


def image_io_bwd(x_nchw, noise, coef, rep, dy, cot_rep=1):
    """dy dense NHWC [N,H,W,C], N = images * rep * K -> dx [images * K, C, H, W]:
    dx[image*K + k] = sum_j dy[(image*rep + j)*K + k] * 1[0 <= pre(image, j) <= 1]"""
    K = max(cot_rep, 1)
    pre = image_pre(x_nchw, noise, coef, rep)                      # [images*rep, C, H, W]
    B, Cc, H, W = x_nchw.shape
    mask = ((pre >= 0) & (pre <= 1)).to(dy.dtype).view(B, rep, 1, Cc, H, W)
    g = dy.permute(0, 3, 1, 2).reshape(B, rep, K, Cc, H, W)
    return (g * mask).sum(dim=1).reshape(B * K, Cc, H, W)


# ---------------------------------------------------------------------------------------------------- ga_avae
def _lrelu02(v):
    return torch.where(v > 0, v, 0.2 * v)


def avae_adain_pre(x, noise, wn):
    return x if noise is None else x + wn * noise[..., None]


def avae_adain(x, noise, wn, style):
    """x [N,P,C], noise [N,P] or None, wn [C], style [N,2C] = (gamma | beta) -> y [N,P,C], stats [N,C,2] = (mean, rstd);
    InstanceNorm: biased variance over the pixels, eps 1e-5"""
    C = x.shape[-1]
    u = _lrelu02(avae_adain_pre(x, noise, wn))
    mean = u.mean(dim=1, keepdim=True)
    var = ((u - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-5)
    y = style[:, None, :C] * (u - mean) * rstd + style[:, None, C:]
    return y, torch.stack([mean[:, 0], rstd[:, 0]], dim=-1)


def avae_adain_bwd(x, noise, wn, style, dy):
    """-> dx [N,P,C], (dgamma | dbeta) [N,2C]"""
    C, P = x.shape[-1], x.shape[1]
    pre = avae_adain_pre(x, noise, wn)
    u = _lrelu02(pre)
    mean = u.mean(dim=1, keepdim=True)
    rstd = 1 / torch.sqrt(((u - mean) ** 2).mean(dim=1, keepdim=True) + 1e-5)
    xhat = (u - mean) * rstd
    dbeta, dgamma = dy.sum(dim=1), (dy * xhat).sum(dim=1)
    du = style[:, None, :C] * rstd * (dy - dbeta[:, None] / P - xhat * dgamma[:, None] / P)
    return du * torch.where(pre > 0, torch.ones_like(pre), 0.2 * torch.ones_like(pre)), torch.cat([dgamma, dbeta], dim=1)


def avgpool(x, k):
    N, H, W, C = x.shape
    return x.reshape(N, H // k, k, W // k, k, C).mean(dim=(2, 4))


def avgpool_bwd(dy, k):
    return dy.repeat_interleave(k, dim=1).repeat_interleave(k, dim=2) / (k * k)


def pixelnorm(x):
    return x / torch.sqrt((x * x).mean(dim=-1, keepdim=True) + 1e-8)


def pixelnorm_bwd(x, dy):
    C = x.shape[-1]
    r = 1 / torch.sqrt((x * x).mean(dim=-1, keepdim=True) + 1e-8)
    return r * dy - x * r ** 3 * (dy * x).sum(dim=-1, keepdim=True) / C


def avae_sample(t, eps_nchw, f0):
    """t [N,P,2C], eps [N,C,P] -> z [N,P,C]"""
    C = t.shape[-1] // 2
    return _lrelu02(t[..., :C]) + eps_nchw.transpose(1, 2) * torch.exp(0.5 * _lrelu02(t[..., C:])) * f0


def avae_sample_bwd(t, eps_nchw, f0, dz):
    C = t.shape[-1] // 2
    sl = lambda v: torch.where(v > 0, torch.ones_like(v), 0.2 * torch.ones_like(v))
    dm = dz * sl(t[..., :C])
    dv = dz * eps_nchw.transpose(1, 2) * torch.exp(0.5 * _lrelu02(t[..., C:])) * f0 * 0.5 * sl(t[..., C:])
    return torch.cat([dm, dv], dim=-1)


# ---------------------------------------------------------------------------------------------------- small maps
def unary(x, g, mode, eps=0.0):
    if mode == 0:
        return x * x
    if mode == 1:
        return 2 * x * g
    if mode == 2:
        return 1 / torch.sqrt(x + eps)
    return -0.5 * g * x * x


def prelu(x, slope):
    return torch.where(x > 0, x, slope * x)


def prelu_bwd(x, slope, dy):
    return dy * torch.where(x > 0, torch.ones_like(x), slope.expand_as(x))


def axpby(x, y, alpha, beta):
    return alpha * x + beta * y


def rep_sum(x, rep):
    """fixed order: ((x0 + x1) + x2) + ..."""
    v = x.reshape(x.shape[0] // rep, rep, -1)
    acc = v[:, 0].clone()
    for r in range(1, rep):
        acc = acc + v[:, r]
    return acc


# ---------------------------------------------------------------------------------------------------- ga_pool_denorm
def _band_mask(H, band, dtype):
    m = torch.ones(H, dtype=dtype)
    if band > 0:
        m[:band] = 0
        m[H - band:] = 0
    return m.view(1, H, 1, 1)


def pool_denorm(x, k, band=0):
    """x [N,kH,kW,4] (lanes 0..2 used) -> pooled image [N,H,W,3] = 0.5 * mean + 0.5, band rows = 0"""
    y = 0.5 * avgpool(x[..., :3], k) + 0.5
    return y * _band_mask(y.shape[1], band, x.dtype)


def pool_denorm_bwd(dy, dy_nchw, k, band=0):
    """dy [N,H,W,3] (+ dy_nchw [N,3,H,W]) -> dx [N,kH,kW,3]"""
    g = dy if dy_nchw is None else dy + dy_nchw.permute(0, 2, 3, 1)
    g = g * _band_mask(g.shape[1], band, g.dtype)
    return 0.5 * avgpool_bwd(g, k)


# ---------------------------------------------------------------------------------------------------- ga_modout / ga_up2_blur
def modout_u(t, scale, add):
    u = t if scale is None else scale[:, None, :] * t
    return u if add is None else u + add[None]


def modout(t, scale, add, a):
    return act(modout_u(t, scale, add), a)


def modout_bwd(t, scale, add, a, dout):
    """-> dt [N,P,C], red [N,C] = sum_p dt * t"""
    dt = dout * dact(modout_u(t, scale, add), a)
    if scale is not None:
        dt = dt * scale[:, None, :]
    return dt, (dt * t).sum(dim=1)


def up2_blur(lo):
    """per axis out[2U] = 1/4 s[U-1] + 3/4 s[U], out[2U+1] = 3/4 s[U] + 1/4 s[U+1], zero beyond the border"""
    def axis(s, dim):
        n = s.shape[dim]
        z = torch.zeros_like(s.narrow(dim, 0, 1))
        prev, nxt = torch.cat([z, s.narrow(dim, 0, n - 1)], dim), torch.cat([s.narrow(dim, 1, n - 1), z], dim)
        ev, od = 0.25 * prev + 0.75 * s, 0.75 * s + 0.25 * nxt
        return torch.stack([ev, od], dim=dim + 1).flatten(dim, dim + 1)
    return axis(axis(lo, 1), 2)


# ---------------------------------------------------------------------------------------------------- ga_latent_mix
def latent_mix(codes, avg, styles, alpha, rep=1):
    """codes [R/rep,J,D], styles [R,J,D], alpha [J]"""
    c = rep_rows(codes, rep)
    if avg is not None:
        c = c + avg
    a = alpha.view(1, -1, 1)
    return (1 - a) * c + a * styles


def latent_mix_bwd(dout, alpha, rep=1):
    R, J, D = dout.shape
    rep = max(rep, 1)
    v = dout.reshape(R // rep, rep, J, D)
    acc = v[:, 0].clone()
    for r in range(1, rep):
        acc = acc + v[:, r]
    return (1 - alpha.view(1, -1, 1)) * acc


def latent_mix_rows(codes, avg, styles, alpha, rep=1):
    """the alpha_ld form: alpha [R,J], row r mixes with its own alpha[r]"""
    c = rep_rows(codes, rep)
    if avg is not None:
        c = c + avg
    a = alpha[:, :, None]
    return (1 - a) * c + a * styles


def latent_mix_rows_bwd(dout, alpha, rep=1):
    """dcodes sums the replicas' cotangents in row order, each scaled by its own (1 - alpha)"""
    R, J, D = dout.shape
    rep = max(rep, 1)
    v = ((1 - alpha[:, :, None]) * dout).reshape(R // rep, rep, J, D)
    acc = v[:, 0].clone()
    for r in range(1, rep):
        acc = acc + v[:, r]
    return acc


def latent_alpha_terms(codes, avg, styles, dout, rep=1):
    """backward 2: the terms of d loss / d alpha, dout * (styles - (codes + avg)), [R,J,D]; out[r][j] is their sum over D"""
    c = rep_rows(codes, rep)
    return dout * (styles - (c if avg is None else c + avg))


def sampler_alpha_c(T):
    """ga_sampler_mix mode 2: additions on the longest path of the kernel's summation tree over T terms -- ceil(T / 256) into a
    thread's strided partial sum, 6 steps of the wave-64 butterfly, 3 for the four waves' partials added in wave order -- plus 16
    for the rounding of one term (two tanhf, one expf, the products): |err| <= c * 2^-24 * sum |term|"""
    return -(-T // 256) + 6 + 3 + 16


def latent_alpha_c(D):
    """ga_latent_mix backward 2: a lane adds 4 per quad it owns (three inside the quad, one into its sum), ceil(D / 4 / 64) quads,
    then 6 butterfly steps; plus 3 for the rounding of one term (codes + avg, styles - that, the product)"""
    return 4 * -(-(D // 4) // 64) + 6 + 3


# ---------------------------------------------------------------------------------------------------- ga_attn
def split_heads(t, heads):
    """[N,T,E] -> [N,heads,T,dh]: head h = channels [h*dh, (h+1)*dh)"""
    N, T, E = t.shape
    return t.reshape(N, T, heads, E // heads).permute(0, 2, 1, 3)


def merge_heads(t):
    N, h, T, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(N, T, h * dh)


def weighted_rows(w, m):
    """[.., Tq, Tk] x [.., Tk, dh] -> [.., Tq, dh] = sum_key w[q][key] * m[key]"""
    return w @ m


def weighted_rows_in_groups(w, m):
    """the same sum in the order csrc/attention.hip documents for P V and dS K: G = 256 / (dh / 4) key groups, group g adds its
    keys g, g + G, ... one after the other, then the groups' partial sums are added in group order.  A yardstick for the long
    sums only (the dtype is still the caller's)."""
    Tk, dh = m.shape[-2], m.shape[-1]
    G = 256 // (dh // 4)
    steps = -(-Tk // G)
    wp, mp = F.pad(w, (0, steps * G - Tk)), F.pad(m, (0, 0, 0, steps * G - Tk))
    part = torch.zeros(*w.shape[:-1], G, dh, dtype=w.dtype)
    for s in range(steps):
        part = part + wp[..., s * G:(s + 1) * G, None] * mp[..., None, s * G:(s + 1) * G, :]
    acc = part[..., 0, :]
    for gg in range(1, G):
        acc = acc + part[..., gg, :]
    return acc


def attn(q, k, v, heads, scale, rows=weighted_rows):
    """q [N,Tq,E], k, v [N,Tk,E] -> out [N,Tq,E], p [N,heads,Tq,Tk] = softmax over the keys of scale * q_h k_h^T"""
    qh, kh, vh = split_heads(q, heads), split_heads(k, heads), split_heads(v, heads)
    s = scale * (qh @ kh.transpose(-1, -2))
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)
    return merge_heads(rows(p, vh)), p


def attn_bwd(q, k, v, heads, scale, dout, rows=weighted_rows):
    """-> dq [N,Tq,E], dk, dv [N,Tk,E]:  dV = P^T dO, dP = dO V^T, dS = P (dP - sum_key dP P), dK = scale dS^T Q, dQ = scale dS K"""
    qh, kh, vh, do = split_heads(q, heads), split_heads(k, heads), split_heads(v, heads), split_heads(dout, heads)
    p = attn(q, k, v, heads, scale)[1]
    dv = p.transpose(-1, -2) @ do
    dp = do @ vh.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(dim=-1, keepdim=True))
    dk = scale * (ds.transpose(-1, -2) @ qh)
    dq = scale * rows(ds, kh)
    return merge_heads(dq), merge_heads(dk), merge_heads(dv)


# ---------------------------------------------------------------------------------------------------- ga_layernorm
def layernorm(a, b, gamma, beta, eps):
    """x = a (+ b), [rows, C] -> y, stats [rows, 2] = (mean, rstd); biased variance, eps inside the root"""
    x = a if b is None else a + b
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    return (x - mean) * rstd * gamma + beta, torch.cat([mean, rstd], dim=-1)


def layernorm_bwd(a, b, gamma, eps, dy):
    """d loss / d x, the same for both summands"""
    x = a if b is None else a + b
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    xhat, gy = (x - mean) * rstd, dy * gamma
    return rstd * (gy - gy.mean(dim=-1, keepdim=True) - xhat * (gy * xhat).mean(dim=-1, keepdim=True))


# ---------------------------------------------------------------------------------------------------- ga_resize2_crop
def _up2_axis(x, dim):
    """bilinear x2, align_corners=False, along one axis: out[2j] = 1/4 x[j-1] + 3/4 x[j], out[2j+1] = 3/4 x[j] + 1/4 x[j+1],
    indices clamped to the image"""
    n = x.shape[dim]
    j = torch.arange(n)
    prev, nxt = x.index_select(dim, (j - 1).clamp(min=0)), x.index_select(dim, (j + 1).clamp(max=n - 1))
    return torch.stack([0.25 * prev + 0.75 * x, 0.75 * x + 0.25 * nxt], dim=dim + 1).flatten(dim, dim + 1)


def _up2_axis_adjoint(dy, dim):
    n = dy.shape[dim] // 2
    j = torch.arange(n)
    ev, od = dy.index_select(dim, 2 * j), dy.index_select(dim, 2 * j + 1)
    dx = 0.75 * ev + 0.75 * od
    dx = dx.index_add(dim, (j - 1).clamp(min=0), 0.25 * ev)
    return dx.index_add(dim, (j + 1).clamp(max=n - 1), 0.25 * od)


def resize2_crop(x, crop):
    """x [N,H,W,C] -> [N, 2H - 2 crop, 2W, C]: rows [crop, 2H - crop) of the x2 image"""
    y = _up2_axis(_up2_axis(x, 1), 2)
    return y[:, crop:y.shape[1] - crop]


def resize2_crop_adjoint(dy, crop):
    """dy [N, 2H - 2 crop, 2W, C] -> dx [N,H,W,C]"""
    full = F.pad(dy, (0, 0, 0, 0, crop, crop))
    return _up2_axis_adjoint(_up2_axis_adjoint(full, 2), 1)


# ---------------------------------------------------------------------------------------------------- ga_gconv
def _taps_range(n_out, n_in, stride, pad, k):
    """the outputs o whose tap k lies inside the image (0 <= o * stride - pad + k < n_in): a range, and its first input"""
    o = [i for i in range(n_out) if 0 <= i * stride - pad + k < n_in]
    return (o[0], o[-1] + 1, o[0] * stride - pad + k) if o else (0, 0, 0)


def gconv(x, w, bias, cg, KH, KW, stride, pad, Ho, Wo, pro_act=NONE, dact_x=None, dact_act=NONE, dact_rep=1):
    """x [N,Hi,Wi,C], w [C][KH*KW*cg] with k = (kh*KW + kw)*cg + ci (row co of group g reads input channels g*cg + ci)
    -> y [N,Ho,Wo,C] = (bias + sum over the taps inside the image) * act'(dact_x row n // dact_rep)"""
    N, Hi, Wi, C = x.shape
    G = C // cg
    a = act(x, pro_act)
    wv = w.reshape(G, cg, KH * KW, cg)                                   # [group][co][tap][ci]
    y = torch.zeros(N, Ho, Wo, C, dtype=x.dtype)
    if bias is not None:
        y = y + bias
    for kh in range(KH):
        h0, h1, hi = _taps_range(Ho, Hi, stride, pad, kh)
        for kw in range(KW):
            w0, w1, wi = _taps_range(Wo, Wi, stride, pad, kw)
            if h1 == h0 or w1 == w0:
                continue
            src = a[:, hi:hi + (h1 - h0 - 1) * stride + 1:stride, wi:wi + (w1 - w0 - 1) * stride + 1:stride]
            src = src.reshape(N, h1 - h0, w1 - w0, G, 1, cg)
            y[:, h0:h1, w0:w1] += (src * wv[:, :, kh * KW + kw]).sum(dim=-1).reshape(N, h1 - h0, w1 - w0, C)
    if dact_x is not None:
        y = y * dact(rep_rows(dact_x, dact_rep), dact_act)
    return y


# ---------------------------------------------------------------------------------------------------- ga_gauss_blur
def _reflect(t, n):
    """'reflect' border (no edge repeat): -1 -> 1, n -> n - 2"""
    t = t.abs()
    return torch.where(t >= n, 2 * (n - 1) - t, t)


def _blur_radius(k, radius):
    return radius if 0 < radius < k // 2 else k // 2


def _blur_axis(x, taps, dim, radius):
    """out[i] = sum_q taps[q] * x[reflect(i + q - k/2)], the taps within `radius` of the centre, in tap order"""
    k, n = taps.numel(), x.shape[dim]
    p, r, i = k // 2, _blur_radius(k, radius), torch.arange(n)
    acc = torch.zeros_like(x)
    for q in range(p - r, p + r + 1):
        acc = acc + taps[q] * x.index_select(dim, _reflect(i + q - p, n))
    return acc


def _blur_axis_adjoint(dy, taps, dim, radius):
    k, n = taps.numel(), dy.shape[dim]
    p, r, i = k // 2, _blur_radius(k, radius), torch.arange(n)
    acc = torch.zeros_like(dy)
    for q in range(p - r, p + r + 1):
        acc = acc.index_add(dim, _reflect(i + q - p, n), taps[q] * dy)
    return acc


def gauss_blur(x, taps, radius=0):
    """x [planes,H,W]: along x, then along y (kornia's separable order)"""
    return _blur_axis(_blur_axis(x, taps, 2, radius), taps, 1, radius)


def gauss_blur_adjoint(dy, taps, radius=0):
    return _blur_axis_adjoint(_blur_axis_adjoint(dy, taps, 1, radius), taps, 2, radius)


# ---------------------------------------------------------------------------------------------------- ga_rowchan_reduce
def pixel_sum(v):
    return v.sum(dim=1)


def lane_sum(v, lanes, tree):
    """sum over dim 1 of [N,P,C] in the order csrc/elementwise.hip documents: `lanes` pixel lanes, lane l adds its pixels l,
    l + lanes, ... one after the other; then the lanes are added as a halving tree (two-stage kernel) or in lane order (single
    stage).  A yardstick for the long sums only."""
    N, P, C = v.shape
    steps = -(-P // lanes)
    vp = F.pad(v, (0, 0, 0, steps * lanes - P)).reshape(N, steps, lanes, C)
    part = torch.zeros(N, lanes, C, dtype=v.dtype)
    for s in range(steps):
        part = part + vp[:, s]
    if tree:
        while lanes > 1:
            lanes //= 2
            part = part[:, :lanes] + part[:, lanes:2 * lanes]
        return part[:, 0]
    acc = part[:, 0]
    for l in range(1, lanes):
        acc = acc + part[:, l]
    return acc


def segment_sum(v, S, lanes):
    """two-stage order: S segments of ceil(P / S) pixels, each by lane_sum with the tree, then added in segment order"""
    P = v.shape[1]
    seg = -(-P // S)
    acc = torch.zeros(v.shape[0], v.shape[2], dtype=v.dtype)
    for s in range(S):
        acc = acc + lane_sum(v[:, s * seg:min(P, (s + 1) * seg)], lanes, True)
    return acc


def reduce_order(N, P, C, ws_floats):
    """(segments S, pixel lanes) of a ga_rowchan_reduce launch as include/ga_ops.h and the kernels' comments give them: two
    stages when a workspace is given and P >= 4096, S = ws_floats / (N C) capped at 2048 workgroups and at 1024 pixels per
    segment, ql = the power of two >= min(16, C / 4) channel-quad lanes x 256 / ql pixel lanes; S < 2: one stage, 16 pixel lanes"""
    nchunks = (C + 63) // 64
    S = min(ws_floats // (N * C), 2048 // (N * nchunks), (P + 1023) // 1024) if ws_floats and P >= 4096 else 1
    if S < 2:
        return 1, 16
    ql = 1
    while ql < min(16, C // 4):
        ql *= 2
    return S, 256 // ql


def order_sum(S, lanes):
    """the `total` of rowchan_reduce in that order"""
    return (lambda v: segment_sum(v, S, lanes)) if S > 1 else (lambda v: lane_sum(v, lanes, False))


def rowchan_reduce(a, b, scale, gate=None, skip=None, a_src=None, a_w=None, total=pixel_sum):
    """out[n,c] = scale * sum_p a[n,p,c] * (b or 1); scaled[n,p,c] = a * gate[n,c] (+ skip) when gate is given, else None.
    a None: a[n,p,c] = sum_{k<4} a_w[c][k] * a_src[n,p,k]"""
    if a is None:
        a = (a_src[:, :, None, :] * a_w).sum(dim=-1)
    out = total(a if b is None else a * b) * scale
    if gate is None:
        return out, None
    scaled = a * gate[:, None, :]
    return out, scaled if skip is None else scaled + skip


# ---------------------------------------------------------------------------------------------------- ga_avgpool_act
def avgpool_act(x, a):
    """x [N,P,C] -> [N,C] = mean_p act(x)"""
    return act(x, a).mean(dim=1)


def avgpool_act_bwd(x, a, dy, act_rep=1):
    P = x.shape[1]
    return dy[:, None, :] / P * dact(rep_rows(x, act_rep), a)


# ---------------------------------------------------------------------------------------------------- layouts
def pitched(t, ld, fill):
    """dense [..., C] -> [..., ld] with the pad channels set to `fill`"""
    out = torch.full((*t.shape[:-1], ld), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def s2d_pack(img, ld, fill):
    """dense NHWC [N,H,W,C] -> space-to-depth [N,H/2,W/2,4*ld]: pixel (h, w) channel c at phase (h&1)*2 + (w&1), lane c"""
    N, H, W, C = img.shape
    v = pitched(img, ld, fill).reshape(N, H // 2, 2, W // 2, 2, ld).permute(0, 1, 3, 2, 4, 5)
    return v.reshape(N, H // 2, W // 2, 4 * ld).contiguous()


def s2d_unpack(t, ld):
    """space-to-depth [N,H/2,W/2,4*ld] -> [N,H,W,ld]"""
    N, h, w, _ = t.shape
    return t.reshape(N, h, w, 2, 2, ld).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * h, 2 * w, ld)


# ---------------------------------------------------------------------------------------------------- bounds and kinks
def max_err(a, ref):
    return (a.detach().double() - ref.double()).abs().max().item()


def bound(fp32_result, ref):
    """what a kernel may differ from `ref` by: 4 x the error of the same formula in plain fp32 on the CPU (another summation
    order, rsqrtf / expf / fast sigmoid against libm), at least 2^-22 of max |ref|"""
    return max(4.0 * max_err(fp32_result, ref), 2.0 ** -22 * ref.abs().max().item())


KINK_REL = 1e-6      # a decision within this of its tie (relative to max |pre|) has no defined derivative
KINK_CAP = 1e-3      # at most this share of a case's elements may be excluded


def near_kink(pre, kinks=(0.0,)):
    """mask of the elements whose pre-activation lies within KINK_REL * max|pre| of a kink"""
    tol = KINK_REL * pre.abs().max()
    m = torch.zeros_like(pre, dtype=torch.bool)
    for k in kinks:
        m |= (pre - k).abs() <= tol
    return m
