"""
tests/opref.py validated without a GPU: every backward reference equals torch.autograd.grad of its forward reference in
float64 to 1e-12 (replicas written as repeat_interleave), the adjoint ops satisfy <A x, y> = <x, A^T y>, the layout helpers
round-trip, and the seeded inputs of tests/test_ops_edges_gpu.py and tests/test_ops_edges2_gpu.py keep the share of near-tie
decisions under the cap those tests are allowed to exclude.  The references of the second sweep are checked against an
independent formulation each: attention against autograd through torch.softmax, LayerNorm against F.layer_norm, the resize
against F.interpolate(align_corners=False), the grouped conv against F.conv2d(groups=...) and, as its own backward, against
autograd through it (stride 1: folding.grouped_bwd_weights; stride 2: the four anchored windows of
folding.grouped_subpixel_weights), the blur against F.pad(mode='reflect') + F.conv2d, the reductions against .sum; adjoints
come from autograd.
"""
import pytest
import torch

import opref as R
import opref_cases as CS

TOL = 1e-12


def d(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def same(a, b, what=''):
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), f'{what}: {err:.3e}'


def grad(out, cot, *wrt):
    return torch.autograd.grad((out * cot).sum(), list(wrt))


@pytest.mark.parametrize('H,W,up', [(5, 7, False), (6, 4, False), (2, 2, False), (12, 20, True), (4, 4, False)])
def test_dwconv5_backward_is_the_adjoint_with_act_prime(H, W, up):
    N, K, C = 2, 3, 8
    hs, ws = (H // 2, W // 2) if up else (H, W)
    x = d(N, hs, ws, C, seed=1).requires_grad_(True)
    w, b = d(25, C, seed=2, scale=0.2), d(C, seed=3)
    cot = d(N * K, H, W, C, seed=4)
    y = R.dwconv5(R.rep_rows(x, K), w, b, pro_act=R.SILU, up2=up)
    xr = R.rep_rows(x, K).detach().requires_grad_(True)
    (gx,) = grad(R.dwconv5(xr, w, b, pro_act=R.SILU, up2=up), cot, xr)
    assert y.shape == cot.shape
    w_flip = w.view(5, 5, C).flip(0, 1).reshape(25, C)
    same(R.dwconv5(cot, w_flip, dact_x=x.detach(), dact_act=R.SILU, pool2=up, act_rep=K), gx, 'dwconv5 bwd')
    # against aten's grouped convolution
    ref = torch.nn.functional.conv2d(R.act(x.detach(), R.SILU).permute(0, 3, 1, 2) if not up else
                                     R.up2_nearest(R.act(x.detach(), R.SILU)).permute(0, 3, 1, 2),
                                     w.t().reshape(C, 1, 5, 5), b, padding=2, groups=C).permute(0, 2, 3, 1)
    same(R.dwconv5(x.detach(), w, b, pro_act=R.SILU, up2=up), ref, 'dwconv5 fwd')


def test_se_excite_fused_backward():
    s = CS.se_case()
    t, dout, w1, b1, w2, b2 = R.f64(s['t'], s['dout'], s['w1'], s['b1'], s['w2'], s['b2'])
    K, rs = s['K'], s['res_scale']
    tr = R.rep_rows(t, K).requires_grad_(True)
    hid, gate = R.se_excite_fwd(tr.mean(dim=1), w1, b1, w2, b2)
    out = rs * gate[:, None, :] * tr
    (gt,) = grad(out, dout, tr)
    hid0, gate0 = R.se_excite_fwd(t.mean(dim=1), w1, b1, w2, b2)
    ps, pb = R.se_excite_bwd_fused(t, dout, hid0, gate0, w1, w2, rs, act_rep=K)
    same(dout * ps[:, None, :] + pb[:, None, :], gt, 'se backward')


def test_se_apply_and_bilinear_adjoint():
    N, H, W, C = 2, 6, 10, 8
    t, gate = d(N, H, W, C, seed=1), d(N, C, seed=2)
    low = d(N, H // 2, W // 2, C, seed=3).requires_grad_(True)
    cot = d(N, H, W, C, seed=4)
    (gl,) = grad(R.se_apply(low, t, gate, 0.1, skip_mode=1), cot, low)
    same(R.bilinear_up2_adjoint(cot), gl, 'bilinear adjoint')
    lhs = (R.bilinear_up2(low.detach()) * cot).sum()
    rhs = (low.detach() * R.bilinear_up2_adjoint(cot)).sum()
    assert abs(lhs - rhs) <= TOL * abs(lhs)
    big = d(N, 2 * H, 2 * W, C, seed=5)
    same(R.se_apply(big, t, gate, 0.1, skip_mode=2), big[:, ::2, ::2] + 0.1 * gate.view(N, 1, 1, C) * t)


def test_sampler_mode1_backward():
    N, K, h, w, NL = 6, 3, 4, 6, 6
    mq, p = d(N // K, h, w, 2 * NL, seed=1, scale=3), d(N // K, h, w, 2 * NL, seed=2, scale=3)
    eps, dz = d(N // K, h, w, NL, seed=3), d(N, h, w, NL, seed=4)
    mr, pr = R.rep_rows(mq, K).requires_grad_(True), R.rep_rows(p, K).requires_grad_(True)
    gq, gp = grad(R.sampler_nd(mr, pr, R.rep_rows(eps, K)), dz, mr, pr)
    ref = R.sampler_nd_bwd(mq, p, eps, dz, act_rep=K)
    same(ref, gq, 'd mu_q')
    same(ref, gp, 'd p')


@pytest.mark.parametrize('first', [False, True])
def test_sampler_mode0_backward_and_alpha_terms(first):
    """per-row alphas; `first`: the prior N(0, 1) of the first group (mu_p None, logsig_p zeros).  The alpha cotangent of mode 2
    is d / d alpha of the forward with one_minus_alpha = 1 - alpha"""
    N, h, w, NL, temp = 4, 3, 5, 6, 0.6
    mq, eps, dz = d(N, h, w, NL, seed=1, scale=3).requires_grad_(True), d(N, h, w, NL, seed=2), d(N, h, w, NL, seed=3)
    mp = None if first else d(N, h, w, NL, seed=4, scale=3).requires_grad_(True)
    ls = torch.zeros(N, h, w, NL, dtype=torch.float64) if first else d(N, h, w, NL, seed=5).requires_grad_(True)
    a = torch.rand(N, 1, 1, 1, generator=torch.Generator().manual_seed(6), dtype=torch.float64).requires_grad_(True)
    leaves = [mq, a] if first else [mq, mp, ls, a]
    g = grad(R.sampler_mix(mq, mp, ls, eps, a, 1 - a, temp), dz, *leaves)
    ref = R.sampler_mix_bwd(*R.f64(mq, mp, ls), eps, dz, a.detach(), 1 - a.detach(), temp)
    same(ref[0], g[0], 'd mu_q')
    if not first:
        same(ref[1], g[1], 'd mu_p')
        same(ref[2], g[2], 'd logsig_p')
    same(R.sampler_alpha_terms(*R.f64(mq, mp, ls), eps, dz, temp).flatten(1).sum(dim=1), g[-1].flatten(), 'd alpha')


def test_latent_mix_rows_backward_and_alpha_terms():
    R_, rep, J, D = 6, 3, 5, 8
    codes, avg, styles, dout = d(R_ // rep, J, D, seed=1), d(J, D, seed=2), d(R_, J, D, seed=3), d(R_, J, D, seed=4)
    a = torch.rand(R_, J, generator=torch.Generator().manual_seed(5), dtype=torch.float64).requires_grad_(True)
    for av in (avg, None):
        c = codes.clone().requires_grad_(True)
        gc_, ga = grad(R.latent_mix_rows(c, av, styles, a, rep), dout, c, a)
        same(R.latent_mix_rows_bwd(dout, a.detach(), rep), gc_, 'd codes')
        same(R.latent_alpha_terms(codes, av, styles, dout, rep).sum(dim=-1), ga, 'd alpha')


def test_dml_mean_backward_and_the_oracle_forward():
    from oracle.nvae_oracle import disc_mix_logistic_mean
    c = CS.dml_case()
    lg, dn, dc = R.f64(c['logits'], c['dimg_nhwc'], c['dimg_nchw'])
    K, nmix = c['K'], c['nmix']
    same(R.dml_mean(lg, nmix), (disc_mix_logistic_mean(lg.permute(0, 3, 1, 2), nmix) * 0.5 + 0.5).permute(0, 2, 3, 1), 'dml forward')
    lr = R.rep_rows(lg, K).requires_grad_(True)
    cot = dn + dc.permute(0, 2, 3, 1)
    (gl,) = grad(R.dml_mean(lr, nmix), cot, lr)
    same(R.dml_mean_bwd(lg, nmix, cot, act_rep=K), gl, 'dml backward')


def test_maxpool2_backward_routes_to_the_first_maximum():
    c = CS.maxpool_case()
    x, dy = R.f64(c['x'], c['dy'])
    xr = R.rep_rows(x, c['K']).requires_grad_(True)
    y = torch.nn.functional.max_pool2d(xr.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    same(R.maxpool2(xr.detach()), y.detach())
    (gx,) = grad(y, dy, xr)
    ours = R.maxpool2_bwd(x, dy, act_rep=c['K'])
    assert torch.equal(ours, gx)                      # aten keeps the first maximum as well: planted ties included
    assert ours[0, 0, 0, 0] == dy[0, 0, 0, 0] and ours[0, 0, 1, 0] == 0 and ours[0, 1, 0, 0] == 0


@pytest.mark.parametrize('mode', ['silu', 'silu_affine', 'prelu'])
def test_interleave2_is_the_epilogue_of_a_strided_transpose(mode):
    c = CS.interleave_case()
    K, N, H, W, C = c['K'], c['N'], c['H'], c['W'], c['C']
    planes, u, slope, sc, sh, a1, a2 = R.f64(c['planes'], c['dact_x'], c['slope'], c['scale'], c['shift'], c['addend'], c['addend2'])
    s = [planes[..., i * C:(i + 1) * C] for i in range(4)]
    s[1] = None
    ur = R.rep_rows(u, K).requires_grad_(True)
    if mode == 'prelu':
        f = R.prelu(ur, slope)
        kw = dict(dact_scale=slope, dact_prelu=True)
    elif mode == 'silu_affine':
        f = R.act(ur * sc + sh, R.SILU)
        kw = dict(dact_scale=sc, dact_shift=sh, dact_act=R.SILU)
    else:
        f = R.act(ur, R.SILU)
        kw = dict(dact_act=R.SILU)
    dense = R.interleave2(s, N, H, W, C)
    (gu,) = grad(f, dense, ur)
    same(R.interleave2(s, N, H, W, C, dact_x=u, addend=a1, addend2=a2, dact_rep=K, **kw), gu + a1 + a2, mode)
    assert (dense[:, 0::2, 1::2] == 0).all()


def test_image_io_backward_and_layouts():
    c = CS.image_case()
    x, noise, coef, dy = R.f64(c['x'], c['noise'], c['coef'], c['dy'])
    B, rep, K = c['B'], c['rep'], c['K']
    # K cotangents: forward row r = image*rep + j is used K times (cotangent rows r*K + k)
    xr = x.clone().requires_grad_(True)
    fwd = R.image_io(xr, noise, coef, rep)                                   # [B*rep, H, W, C]
    loss = (R.rep_rows(fwd, K) * dy).sum()
    (gx,) = torch.autograd.grad(loss, [xr], retain_graph=True)               # sums over j AND k
    ref = R.image_io_bwd(x, noise, coef, rep, dy, cot_rep=K)                 # [B*K, C, H, W]: k kept apart
    same(ref.view(B, K, *x.shape[1:]).sum(dim=1), gx, 'image_io backward')
    for k in range(K):                                                       # and each k on its own
        (gk,) = torch.autograd.grad((fwd * dy.view(B * rep, K, *dy.shape[1:])[:, k]).sum(), [xr], retain_graph=True)
        same(ref.view(B, K, *x.shape[1:])[:, k], gk, f'image_io backward k={k}')
    pre = R.image_pre(x, noise, coef, rep)
    lo, hi = (pre < 0).double().mean().item(), (pre > 1).double().mean().item()
    assert 0.25 < lo < 0.42 and 0.25 < hi < 0.42, (lo, hi)
    img = fwd.detach()
    packed = R.s2d_pack(img, 4, -7.0)
    assert packed.shape == (B * rep, 3, 5, 16)
    back = R.s2d_unpack(packed, 4)
    assert torch.equal(back[..., :3], img) and (back[..., 3] == -7.0).all()
    assert packed[1, 2, 3, 1 * 4 + 2] == img[1, 4, 7, 2] and packed[0, 1, 1, 2 * 4 + 0] == img[0, 3, 2, 0]
    assert torch.equal(R.pitched(img, 8, 5.0)[..., :3], img)


@pytest.mark.parametrize('shape', CS.ADAIN_SHAPES)
@pytest.mark.parametrize('offset', [0.0, 8.0])
def test_avae_adain(shape, offset):
    c = CS.adain_case(*shape, offset=offset)
    x, noise, wn, style, dy = R.f64(c['x'], c['noise'], c['wn'], c['style'], c['dy'])
    C = x.shape[-1]
    xr, sr = x.clone().requires_grad_(True), style.clone().requires_grad_(True)
    y, stats = R.avae_adain(xr, noise, wn, sr)
    u = R._lrelu02(R.avae_adain_pre(x, noise, wn))
    inorm = torch.nn.functional.instance_norm(u.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
    same(y.detach(), style[:, None, :C] * inorm + style[:, None, C:], 'adain forward vs instance_norm')
    gx, gs = grad(y, dy, xr, sr)
    dx, dgb = R.avae_adain_bwd(x, noise, wn, style, dy)
    same(dx, gx, 'adain dx')
    same(dgb, gs, 'adain dgamma | dbeta')
    same(stats[..., 0], u.mean(dim=1))


@pytest.mark.parametrize('k', [2, 4])
def test_avae_avgpool_and_pool_denorm_adjoints(k):
    N, H, W, C = 2, 8, 12, 12
    x, y = d(N, H, W, C, seed=1), d(N, H // k, W // k, C, seed=2)
    lhs, rhs = (R.avgpool(x, k) * y).sum(), (x * R.avgpool_bwd(y, k)).sum()
    assert abs(lhs - rhs) <= TOL * abs(lhs)
    for band in (0, 2):
        xi, yo, yn = d(N, 6 * k, 10 * k, 4, seed=3), d(N, 6, 10, 3, seed=4), d(N, 3, 6, 10, seed=5)
        A = lambda v: R.pool_denorm(v, k, band) - R.pool_denorm(torch.zeros_like(v), k, band)       # the linear part
        lhs = (A(xi) * (yo + yn.permute(0, 2, 3, 1))).sum()
        rhs = (xi[..., :3] * R.pool_denorm_bwd(yo, yn, k, band)).sum()
        assert abs(lhs - rhs) <= TOL * abs(lhs)
        assert band == 0 or (R.pool_denorm(xi, k, band)[:, :band] == 0).all()


def test_avae_pixelnorm_sample_prelu_modout_latent_mix_unary():
    x, dy = d(7, 100, seed=1), d(7, 100, seed=2)
    xr = x.clone().requires_grad_(True)
    same(R.pixelnorm_bwd(x, dy), grad(R.pixelnorm(xr), dy, xr)[0], 'pixelnorm')
    c = CS.sample_case()
    t, eps, dz = R.f64(c['t'], c['eps'], c['dz'])
    tr = t.clone().requires_grad_(True)
    same(R.avae_sample_bwd(t, eps, c['f0'], dz), grad(R.avae_sample(tr, eps, c['f0']), dz, tr)[0], 'sample')
    c = CS.prelu_case()
    x, sl, dy = R.f64(c['x'], c['slope'], c['dy'])
    nz = x != 0                                               # the derivative at an exact zero is the slope branch by definition
    xr = x.clone().requires_grad_(True)
    same(R.prelu_bwd(x, sl, dy)[nz], grad(R.prelu(xr, sl), dy, xr)[0][nz], 'prelu')
    assert torch.equal(R.prelu_bwd(x, sl, dy)[~nz], (dy * sl.expand_as(x))[~nz]) and int((~nz).sum()) == 9
    for P in (35, 700):
        c = CS.modout_case(P)
        t, sc, ad, do = R.f64(c['t'], c['scale'], c['add'], c['dout'])
        for a in (R.FLRELU, R.NONE):
            for s_, a_ in ((sc, ad), (None, ad), (sc, None), (None, None)):
                tr = t.clone().requires_grad_(True)
                dt, red = R.modout_bwd(t, s_, a_, a, do)
                same(dt, grad(R.modout(tr, s_, a_, a), do, tr)[0], 'modout')
                same(red, (dt * t).sum(dim=1))
    R_, J, D = 6, 5, 12
    for rep in (1, 3):
        codes, avg, st, al, do = d(R_ // rep, J, D, seed=1), d(J, D, seed=2), d(R_, J, D, seed=3), torch.rand(J, dtype=torch.float64), d(R_, J, D, seed=4)
        cr = codes.clone().requires_grad_(True)
        same(R.latent_mix_bwd(do, al, rep), grad(R.latent_mix(cr, avg, st, al, rep), do, cr)[0], 'latent_mix')
    xs, gs = torch.rand(50, dtype=torch.float64) + 0.1, d(50, seed=5)
    xr = xs.clone().requires_grad_(True)
    same(R.unary(xs, gs, 1), grad(R.unary(xr, None, 0), gs, xr)[0], 'unary 1 = backward of 0')
    same(R.unary(xs, None, 2, 1e-8), (xs + 1e-8) ** -0.5)
    lo = d(2, 3, 5, 4, seed=6)
    fir = torch.tensor([1., 3., 3., 1.], dtype=torch.float64)
    k2 = torch.outer(fir, fir) / fir.sum() ** 2 * 4          # make_kernel normalises to sum 1, Upsample scales by factor^2
    up = torch.zeros(2, 4, 6, 10, dtype=torch.float64)
    up[:, :, ::2, ::2] = lo.permute(0, 3, 1, 2)
    want = torch.nn.functional.conv2d(torch.nn.functional.pad(up, (2, 1, 2, 1)), k2.flip(0, 1).view(1, 1, 4, 4).expand(4, 1, 4, 4), groups=4)
    same(R.up2_blur(lo), want.permute(0, 2, 3, 1), 'up2_blur = upfirdn2d(up 2, pad (2, 1))')


@pytest.mark.parametrize('dh,heads,Tk,qscale', [(16, 3, 5, 1.0), (48, 1, 257, 1.0), (112, 3, 300, 1.0), (80, 3, 300, 30.0), (128, 1, 1, 1.0)])
def test_attn_against_autograd_through_softmax(dh, heads, Tk, qscale):
    N, Tq, E = 2, 16, heads * dh
    q, k, v, dout = d(N, Tq, E, seed=1) * qscale, d(N, Tk, E, seed=2), d(N, Tk, E, seed=3), d(N, Tq, E, seed=4)
    scale = dh ** -0.5
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    sc = scale * torch.einsum('nqhc,nkhc->nhqk', qr.view(N, Tq, heads, dh), kr.view(N, Tk, heads, dh))
    pr = torch.softmax(sc, dim=-1)
    want = torch.einsum('nhqk,nkhc->nqhc', pr, vr.view(N, Tk, heads, dh)).reshape(N, Tq, E)
    out, p = R.attn(q, k, v, heads, scale)
    same(out, want.detach(), 'attn out')
    same(p, pr.detach(), 'attn p')
    for got, ref, what in zip(R.attn_bwd(q, k, v, heads, scale, dout), grad(want, dout, qr, kr, vr), ('dq', 'dk', 'dv')):
        same(got, ref, f'attn {what}')
    # the kernel-order yardstick is the same sum
    same(R.attn(q, k, v, heads, scale, rows=R.weighted_rows_in_groups)[0], out, 'attn out, group order')
    same(R.attn_bwd(q, k, v, heads, scale, dout, rows=R.weighted_rows_in_groups)[0], R.attn_bwd(q, k, v, heads, scale, dout)[0], 'dq, group order')
    if qscale > 1:
        assert float((sc.detach().amax(dim=-1) - sc.detach().amin(dim=-1)).min()) > 30 and float(sc.detach().abs().max()) > 89   # expf overflows
    if Tk == 1:
        assert bool((p == 1).all()) and torch.equal(out, v.expand(N, Tq, E))


@pytest.mark.parametrize('C', [4, 100, 260, 1028])
@pytest.mark.parametrize('with_b', [True, False])
def test_layernorm_against_f_layer_norm(C, with_b):
    rows, eps = 7, 1e-5
    a, b, gamma, beta, dy = d(rows, C, seed=1), (d(rows, C, seed=2) if with_b else None), d(C, seed=3), d(C, seed=4), d(rows, C, seed=5)
    a = a + 100.0 * d(rows, 1, seed=6)
    ar = a.clone().requires_grad_(True)
    x = ar if b is None else ar + b
    want = torch.nn.functional.layer_norm(x, (C,), gamma, beta, eps)
    y, stats = R.layernorm(a, b, gamma, beta, eps)
    same(y, want.detach(), 'layernorm')
    same(stats[:, 0], x.detach().mean(dim=-1))
    same(stats[:, 1], (x.detach().var(dim=-1, unbiased=False) + eps) ** -0.5)
    same(R.layernorm_bwd(a, b, gamma, eps, dy), grad(want, dy, ar)[0], 'layernorm backward')


@pytest.mark.parametrize('H,W,crop', [(1, 1, 0), (5, 7, 0), (5, 7, 1), (6, 10, 3), (8, 8, 0)])
def test_resize2_crop_against_interpolate(H, W, crop):
    N, C = 3, 4
    x, dy = d(N, H, W, C, seed=1), d(N, 2 * H - 2 * crop, 2 * W, C, seed=2)
    xr = x.clone().requires_grad_(True)
    up = torch.nn.functional.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False)
    want = up[:, :, crop:2 * H - crop].permute(0, 2, 3, 1)
    same(R.resize2_crop(x, crop), want.detach(), 'resize2_crop')
    same(R.resize2_crop_adjoint(dy, crop), grad(want, dy, xr)[0], 'resize2_crop adjoint')


def _torch_w(w, cg, KH, KW):
    """ga_gconv layout [C][(kh*KW + kw)*cg + ci] -> [C, cg, KH, KW]"""
    return w.view(w.shape[0], KH, KW, cg).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('cg', [4, 12])
@pytest.mark.parametrize('stride', [1, 2])
def test_gconv_against_grouped_conv2d(cg, stride):
    from gen_adversarial_amd.folding import conv_fwd_layout, grouped_bwd_weights, grouped_subpixel_weights
    N, G, H, W = 2, 3, 9 if stride == 1 else 6, 11 if stride == 1 else 10
    C = G * cg
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    x, w, b = d(N, H, W, C, seed=1), d(C, 9 * cg, seed=2, scale=0.2).float().double(), d(C, seed=3)   # folding returns fp32 weights
    xr = x.clone().requires_grad_(True)
    wt = _torch_w(w, cg, 3, 3)
    want = torch.nn.functional.conv2d(torch.relu(xr).permute(0, 3, 1, 2), wt, b, stride=stride, padding=1, groups=G).permute(0, 2, 3, 1)
    same(R.gconv(x, w, b, cg, 3, 3, stride, 1, Ho, Wo, pro_act=R.RELU), want.detach(), 'gconv forward')
    same(R.gconv(x, w, None, cg, 3, 3, stride, 1, Ho, Wo), torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), wt, None, stride=stride, padding=1,
                                                                                       groups=G).permute(0, 2, 3, 1), 'no bias, no act')
    K = 3                                                               # K cotangents per forward row
    cot = d(N * K, Ho, Wo, C, seed=4)
    xk = R.rep_rows(x, K).requires_grad_(True)
    yk = torch.nn.functional.conv2d(torch.relu(xk).permute(0, 3, 1, 2), wt, b, stride=stride, padding=1, groups=G).permute(0, 2, 3, 1)
    (gx,) = grad(yk, cot, xk)
    if stride == 1:                                                     # its own backward-to-input: swapped, flipped weights and act'
        wb = conv_fwd_layout(grouped_bwd_weights(wt, G))
        same(R.gconv(cot, wb, None, cg, 3, 3, 1, 1, H, W, dact_x=x, dact_act=R.RELU, dact_rep=K), gx, 'gconv backward')
    else:                                                               # the transpose as four anchored windows, one per output parity
        sub = grouped_subpixel_weights(wt, G)
        assert sorted((kh, kw) for _, kh, kw in sub.values()) == [(1, 1), (1, 2), (2, 1), (2, 2)]
        dense = torch.zeros(N * K, H, W, C, dtype=torch.float64)
        for (pa, pb), (wab, kh, kw) in sub.items():
            dense[:, pa::2, pb::2] = R.gconv(cot, wab, None, cg, kh, kw, 1, 0, Ho, Wo, dact_x=x[:, pa::2, pb::2], dact_act=R.RELU, dact_rep=K)
        same(dense, gx, 'stride-2 transpose from anchored sub-kernels')


@pytest.mark.parametrize('H,W,k,radius', [(8, 12, 15, 0), (12, 8, 15, 0), (5, 90, 9, 0), (12, 40, 23, 0), (12, 40, 23, 4)])
def test_gauss_blur_against_reflect_pad_and_conv2d(H, W, k, radius):
    x, dy = d(3, H, W, seed=1), d(3, H, W, seed=2)
    taps = torch.exp(-(torch.arange(k, dtype=torch.float64) - k // 2) ** 2 / 2)
    taps = taps / taps.sum()
    used = taps.clone()
    if radius:
        used[:k // 2 - radius] = 0
        used[k // 2 + radius + 1:] = 0
    xr = x.clone().requires_grad_(True)
    p = k // 2
    y = torch.nn.functional.pad(xr[:, None], (p, p, p, p), mode='reflect')
    y = torch.nn.functional.conv2d(torch.nn.functional.conv2d(y, used.view(1, 1, 1, k)), used.view(1, 1, k, 1))[:, 0]
    same(R.gauss_blur(x, taps, radius), y.detach(), 'blur')
    same(R.gauss_blur_adjoint(dy, taps, radius), grad(y, dy, xr)[0], 'blur adjoint')
    if radius:                                                          # the skipped taps lie below the resolution of the result
        assert (R.gauss_blur(x, taps, radius) - R.gauss_blur(x, taps)).abs().max().item() < 1e-3


def test_rowchan_reduce_and_its_summation_orders():
    N, P, C = 2, 4100, 20
    a, b, gate, skip = d(N, P, C, seed=1), d(N, P, C, seed=2), d(N, C, seed=3), d(N, P, C, seed=4)
    out, scaled = R.rowchan_reduce(a, b, 0.5, gate, skip)
    same(out, 0.5 * (a * b).sum(dim=1))
    same(scaled, a * gate[:, None] + skip)
    assert R.rowchan_reduce(a, None, 1.0)[1] is None
    same(R.rowchan_reduce(a, None, 1.0)[0], a.sum(dim=1))
    src, aw = d(N, P, 4, seed=5), d(C, 4, seed=6)
    same(R.rowchan_reduce(None, b, 1.0, a_src=src, a_w=aw)[0], (torch.einsum('npk,ck->npc', src, aw) * b).sum(dim=1))
    for S, lanes in ((2, 32), (5, 64), (3, 16)):
        same(R.segment_sum(a, S, lanes), a.sum(dim=1), 'segment order')
    same(R.lane_sum(a[:, :4095], 16, False), a[:, :4095].sum(dim=1), 'lane order')


@pytest.mark.parametrize('P,C', CS.AVGPOOL_SHAPES)
@pytest.mark.parametrize('a', [R.NONE, R.RELU, R.SILU])
def test_avgpool_act(P, C, a):
    c = CS.avgpool_case(P, C)
    x, dy = R.f64(c['x'], c['dy'])
    K = 3
    xr = x.clone().requires_grad_(True)
    f = {R.NONE: lambda u: u, R.RELU: torch.relu, R.SILU: torch.nn.functional.silu}[a]
    want = f(xr).mean(dim=1)
    same(R.avgpool_act(x, a), want.detach(), 'avgpool_act')
    (gx,) = grad(want, dy, xr)
    same(R.avgpool_act_bwd(x, a, dy), gx, 'avgpool_act backward')
    same(R.avgpool_act_bwd(x, a, R.rep_rows(dy, K), act_rep=K), R.rep_rows(gx, K), 'act_rep')


def test_seeded_gpu_inputs_stay_under_the_kink_cap():
    for name, pre, kinks in CS.kink_sites():
        share = R.near_kink(pre, kinks).double().mean().item()
        assert share <= R.KINK_CAP, f'{name}: {share:.2e} of the decisions lie within {R.KINK_REL} of a tie'
    c = CS.maxpool_case()
    gap = R.maxpool2_gap(R.f64(c['x']))
    assert int((gap == 0).sum()) == 3                         # the planted ties, compared exactly by the GPU test, and no other
