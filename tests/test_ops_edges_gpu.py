"""
Kernels against tests/opref.py (float64, written from include/ga_ops.h) where only whole-model tests went before:
  A. the K-cotangent / replica fields (act_rep, dact_rep, cot_rep), backward with K = 3 cotangents per forward row;
  B. entry points without a direct test (ga_avae, ga_unary, ga_prelu, ga_pixelnorm, ga_axpby, ga_pool_denorm, interleaved
     ga_modout, shared-alpha ga_latent_mix, ga_sampler_mix mode 1);
  C. shapes: odd / non-square / ragged images and one trip past every capped grid.
Conventions: outputs start as NaN, pad channels and one extra trailing row as a sentinel; whatever the header says is written
must be finite and close, whatever it says is left alone must still hold the sentinel.
Tolerances: exact ops are compared for equality with the float64 result rounded once to fp32; ops with an older op test use
that test's tolerance and `close`; every other op may differ from float64 by at most opref.bound() = 4 x the error of the
same formula in plain fp32 PyTorch on the CPU (floor 2^-22 of max |ref|), measured on the test's own inputs; the measured
figures are in the docstrings.  Gradient elements whose decision lies within 1e-6 of a kink are left out (at most 0.1 %;
tests/test_opref_cpu.py asserts that cap on the same seeds with the reference alone).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

import opref as R   # noqa: E402
import opref_cases as CS   # noqa: E402
from gen_adversarial_amd import _lib as L   # noqa: E402
from test_ops_gpu import DEV, close, g, nchw, nhwc   # noqa: E402,F401

SENT = -777.25
NAN = float('nan')


class Out:
    """an output buffer of `shape` pre-filled with `fill`, plus one trailing row of sentinels that must survive"""

    def __init__(self, *shape, fill=NAN):
        self.n, row = math.prod(shape), math.prod(shape[1:])
        self.flat = torch.full((self.n + row,), SENT, device=DEV)
        self.flat[:self.n] = fill
        self.t = self.flat[:self.n].view(*shape)

    @classmethod
    def of(cls, t):
        """an in / out buffer holding t"""
        o = cls(*t.shape)
        o.t.copy_(t)
        return o

    def done(self):
        torch.cuda.synchronize()
        assert bool((self.flat[self.n:] == SENT).all()), 'the row behind the output was written'
        return self.t.cpu()


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def launch(cls, **kw):
    d, keep = cls(), []
    for k, v in kw.items():
        if isinstance(v, Out):
            v = v.t
        if isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                getattr(d, k)[i] = None if e is None else e.data_ptr() if torch.is_tensor(e) else e
            keep.append(v)
            continue
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(d, k, v)
    L.run(d)
    torch.cuda.synchronize()
    return d


def near(what, out, ref, fp32, skip=None):
    """new-op rule: finite, and within opref.bound(fp32 CPU result, float64 reference); `skip` = near-kink mask"""
    out, ref = out.double(), ref.double()
    assert torch.isfinite(out).all(), f'{what}: not every element was written'
    if skip is not None:
        share = skip.double().mean().item()
        assert share <= R.KINK_CAP, f'{what}: {share:.2e} of the elements sit on a kink'
        out, ref, fp32 = out[~skip], ref[~skip], fp32[~skip]
    b, cpu, err = R.bound(fp32, ref), R.max_err(fp32, ref), R.max_err(out, ref)
    print(f'{what}: fp32-CPU err {cpu:.3e}, bound {b:.3e}, kernel err {err:.3e} (ref max {ref.abs().max().item():.3e})')
    assert err <= b, f'{what}: kernel err {err:.3e} > bound {b:.3e} (fp32 CPU {cpu:.3e})'


def exact(what, out, ref, skip=None):
    want = ref.float()
    if skip is not None:
        assert skip.double().mean().item() <= R.KINK_CAP
        out, want = out[~skip], want[~skip]
    assert torch.equal(out, want), f'{what}: {int((out != want).sum())} elements differ, max {(out - want).abs().max().item():.3e}'


def f32(*ts):
    return tuple(None if t is None else t.float() for t in ts)


# =====================================================================================================================
# A. replica / cotangent fields
# =====================================================================================================================
@pytest.mark.parametrize('N,H,W,C,pool', [(54, 4, 4, 36, False), (6, 12, 20, 40, True), (6, 6, 10, 8, False)])
def test_dwconv5_backward_act_rep(N, H, W, C, pool):
    """the 4 x 4 kernel (4 blocks of 16 images, the last one partial), the windowed kernel with pool2 (both axes ragged, two
    32-channel chunks) and without; the act' source has N / 3 rows.  dwconv5's own tolerance: 1e-5 (kernel err 4.7e-7, 1.5e-6,
    5.4e-7)."""
    K = 3
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    cot, w, u = g(N, H, W, C, seed=1), g(25, C, seed=2, scale=0.2), g(N // K, Ho, Wo, C, seed=3)
    ref = R.dwconv5(*R.f64(cot, w), dact_x=R.f64(u), dact_act=R.SILU, pool2=pool, act_rep=K)
    y = Out(N, Ho, Wo, C)
    launch(L.DwDesc, x=dev(cot), w=dev(w), dact_x=dev(u), y=y, N=N, H=H, W=W, C=C, dact_act=L.GA_ACT_SILU, pool2=int(pool), act_rep=K)
    out = y.done()
    assert torch.isfinite(out).all()
    print(f'dwconv5 act_rep: kernel err {R.max_err(out, ref):.3e}')
    close(out, ref, 1e-5, 'dwconv5 backward, act_rep = 3')


def test_se_excite_fused_backward_act_rep():
    """N = 6 cotangent rows on 2 forward rows, P = 35, C = 132, Hd = 16.  fp32-CPU err / bound / kernel err:
    hid 2.0e-7 / 7.9e-7 / 1.6e-7, gate 9.6e-8 / 3.8e-7 / 1.1e-7, pro_scale 1.1e-8 / 4.6e-8 / 1.2e-8, pro_shift 1.3e-8 / 5.2e-8 / 8.2e-9."""
    c = CS.se_case()
    K, N, P, C, Hd, rs = c['K'], c['N'], c['P'], c['C'], c['Hd'], c['res_scale']
    names = ('t', 'dout', 'w1', 'b1', 'w2', 'b2')
    t, dout, w1, b1, w2, b2 = (c[k] for k in names)
    td, dd, W = dev(t), dev(dout), [dev(c[k]) for k in names[2:]]
    hid, gate = Out(N // K, Hd), Out(N // K, C)
    wk = dict(w1=W[0], b1=W[1], w2=W[2], b2=W[3], C=C, Hd=Hd, P=P, res_scale=rs)
    launch(L.SeExciteDesc, t=td, hid=hid, gate=gate, N=N // K, **wk)
    ps, pb = Out(N, C), Out(N, C)
    launch(L.SeExciteDesc, t=td, dout=dd, hid=hid, gate=gate, pro_scale=ps, pro_shift=pb, N=N, backward=1, act_rep=K, **wk)

    def ref(cast):
        t_, do_, w1_, b1_, w2_, b2_ = cast(t, dout, w1, b1, w2, b2)
        h_, g_ = R.se_excite_fwd(t_.mean(dim=1), w1_, b1_, w2_, b2_)
        return (h_, g_) + R.se_excite_bwd_fused(t_, do_, h_, g_, w1_, w2_, rs, act_rep=K)
    r64, r32 = ref(R.f64), ref(f32)
    near('se hid', hid.done(), r64[0], r32[0])
    near('se gate', gate.done(), r64[1], r32[1])
    near('se pro_scale', ps.done(), r64[2], r32[2])
    near('se pro_shift', pb.done(), r64[3], r32[3])


@pytest.mark.parametrize('ld_img', [0, 4])
def test_dml_mean_backward_act_rep(ld_img):
    """both cotangents (NHWC with pitch ld_img, NCHW), logits with N / 3 rows, H x W = 6 x 10.  dml's own tolerance: 1e-6
    (kernel err 2.6e-7)."""
    c = CS.dml_case()
    K, N, H, W, nmix, ld = (c[k] for k in ('K', 'N', 'H', 'W', 'nmix', 'ld'))
    lg, dn, dc = c['logits'], c['dimg_nhwc'], c['dimg_nchw']
    ref = R.dml_mean_bwd(R.f64(lg), nmix, R.f64(dn) + R.f64(dc).permute(0, 2, 3, 1), act_rep=K)
    skip = R.rep_rows(R.near_kink(R.dml_pre(R.f64(lg), nmix), (-1.0, 1.0)).any(dim=-1), K)
    assert skip.double().mean().item() <= R.KINK_CAP
    dl = Out(N, H, W, ld)
    launch(L.DmlDesc, logits=dev(lg), ld=ld, nmix=nmix, dimg_nhwc=dev(R.pitched(dn, ld_img, SENT) if ld_img else dn), dimg_nchw=dev(dc),
           dlogits=dl, N=N, H=H, W=W, backward=1, ld_img=ld_img, act_rep=K)
    out = dl.done()
    assert torch.isfinite(out).all()
    print(f'dml act_rep: kernel err {R.max_err(out[~skip], ref[~skip]):.3e}')
    close(out[~skip], ref[~skip], 1e-6, 'dml backward, act_rep = 3')
    # forward at the same non-square shape, image pitch included: pad channels are zeroed
    ldi = ld_img or 3
    o1, o2 = Out(N // K, 3, H, W), Out(N // K, H, W, ldi, fill=SENT)
    launch(L.DmlDesc, logits=dev(lg), ld=ld, nmix=nmix, img_nchw=o1, img_nhwc=o2, N=N // K, H=H, W=W, ld_img=ld_img)
    img = R.dml_mean(R.f64(lg), nmix)
    close(o1.done().permute(0, 2, 3, 1), img, 1e-6, 'dml nchw')
    close(o2.done()[..., :3], img, 1e-6, 'dml nhwc')
    assert bool((o2.t[..., 3:] == 0).all())


def test_maxpool2_backward_act_rep_with_ties():
    """exact: dy lands on the first maximum in scan order of forward row n // 3, planted ties included"""
    c = CS.maxpool_case()
    K, x, dy = c['K'], c['x'], c['dy']
    N, Ho, Wo, C = dy.shape
    dx = Out(N, 2 * Ho, 2 * Wo, C)
    launch(L.MaxpoolDesc, x=dev(x), dy=dev(dy), dx=dx, N=N, H=2 * Ho, W=2 * Wo, C=C, backward=1, act_rep=K)
    exact('maxpool2 backward', dx.done(), R.maxpool2_bwd(R.f64(x), R.f64(dy), act_rep=K))
    y = Out(N // K, Ho, Wo, C)
    launch(L.MaxpoolDesc, x=dev(x), y=y, N=N // K, H=2 * Ho, W=2 * Wo, C=C)
    exact('maxpool2 forward 6 x 10', y.done(), R.maxpool2(R.f64(x)))


@pytest.mark.parametrize('mode', ['silu', 'silu_affine', 'prelu', 'copy'])
def test_interleave2_dact_rep(mode):
    """dact_rep = 3, the planes are channel slices of one [N,H/2,W/2,4C] tensor (lds = 4C), plane (0, 1) is NULL, addend aliases
    y, a second addend.  'copy' (no dact, no addends) is exact.  fp32-CPU err / bound / kernel err: silu 3.7e-7 / 1.5e-6 /
    4.9e-7, silu_affine 5.2e-7 / 2.1e-6 / 7.3e-7, prelu 3.9e-7 / 1.5e-6 / 3.9e-7."""
    c = CS.interleave_case()
    K, N, H, W, C = c['K'], c['N'], c['H'], c['W'], c['C']
    planes = dev(c['planes'])
    ptrs = [planes.data_ptr() + 4 * i * C for i in range(4)]
    ptrs[1] = None
    kw = dict(s=ptrs, N=N, H=H, W=W, C=C, lds=4 * C)
    if mode == 'copy':
        y = Out(N, H, W, C)
        launch(L.Interleave2Desc, y=y, **kw)
        s64 = [R.f64(c['planes'])[..., i * C:(i + 1) * C] for i in range(4)]
        s64[1] = None
        exact('interleave2 copy', y.done(), R.interleave2(s64, N, H, W, C))
        return

    def ref(cast):
        pl, u, sl, sc, sh, a1, a2 = cast(c['planes'], c['dact_x'], c['slope'], c['scale'], c['shift'], c['addend'], c['addend2'])
        s = [pl[..., i * C:(i + 1) * C] for i in range(4)]
        s[1] = None
        rk = dict(prelu=dict(dact_scale=sl, dact_prelu=True), silu_affine=dict(dact_scale=sc, dact_shift=sh, dact_act=R.SILU),
                  silu=dict(dact_act=R.SILU))[mode]
        return R.interleave2(s, N, H, W, C, dact_x=u, addend=a1, addend2=a2, dact_rep=K, dtype=pl.dtype, **rk)
    y = Out.of(dev(c['addend']))
    kw.update(y=y, dact_x=dev(c['dact_x']), addend=y.t, addend2=dev(c['addend2']), dact_rep=K)
    if mode == 'prelu':
        kw.update(dact_scale=dev(c['slope']), dact_prelu=1)
    elif mode == 'silu_affine':
        kw.update(dact_scale=dev(c['scale']), dact_shift=dev(c['shift']), dact_act=L.GA_ACT_SILU)
    else:
        kw.update(dact_act=L.GA_ACT_SILU)
    launch(L.Interleave2Desc, **kw)
    near(f'interleave2 {mode}', y.done(), ref(R.f64), ref(f32))


@pytest.mark.parametrize('s2d', [0, 1])
def test_image_io_cot_rep(s2d):
    """2 images x rep 2 x K = 3 cotangents, 6 x 10, pitch 4, plain and space-to-depth; noise clamps about a third of the pixels
    on each side.  Backward: the mask is exact and the two-term sum is one rounding -> equality away from the clamp bounds.
    Forward (rep = 2): fp32-CPU err 4.3e-8, bound 2.4e-7 (the 2^-22 floor), kernel err 3.0e-8; pad channels zero."""
    c = CS.image_case()
    B, rep, K, C, H, W = (c[k] for k in ('B', 'rep', 'K', 'C', 'H', 'W'))
    x, noise, coef, dy = c['x'], c['noise'], c['coef'], c['dy']
    ld, N = 4, B * rep * K
    pack = (lambda t: R.s2d_pack(t, ld, SENT)) if s2d else (lambda t: R.pitched(t, ld, SENT))
    unpack = (lambda t: R.s2d_unpack(t, ld)) if s2d else (lambda t: t)
    io = dict(x_nchw=dev(x), noise_nchw=dev(noise), noise_coef=dev(coef), C=C, H=H, W=W, rep=rep, ld=ld, s2d=s2d)
    dx = Out(B * K, C, H, W)
    launch(L.ImageIoDesc, dy_nhwc=dev(pack(dy)), dx_nchw=dx, N=N, backward=1, cot_rep=K, **io)
    pre = R.image_pre(*R.f64(x, noise, coef), rep)
    kink = R.near_kink(pre, (0.0, 1.0)).view(B, rep, C, H, W).any(dim=1)                       # [B, C, H, W]
    skip = kink[:, None].expand(B, K, C, H, W).reshape(B * K, C, H, W)
    exact('image_io backward, cot_rep = 3', dx.done(), R.image_io_bwd(*R.f64(x, noise, coef), rep, R.f64(dy), cot_rep=K), skip)
    shape = (B * rep, H // 2, W // 2, 4 * ld) if s2d else (B * rep, H, W, ld)
    y = Out(*shape)
    launch(L.ImageIoDesc, y_nhwc=y, N=B * rep, **io)
    out = unpack(y.done())
    near('image_io forward', out[..., :C], R.image_io(*R.f64(x, noise, coef), rep), R.image_io(x, noise, coef, rep))
    assert bool((out[..., C:] == 0).all()), 'pad channels are zero-filled'


@pytest.mark.parametrize('N,H,Cc,Hd,variant', [(6, 8, 256, 64, 0), (6, 16, 128, 32, 1)])
def test_dec_cell_backward_act_rep(N, H, Cc, Hd, variant):
    """ga_dec_cell backward with 3 cotangents per forward row against the plain-PyTorch cell of test_dec_cell_gpu.py through
    autograd, at that file's tolerance (2e-4; kernel err 4.9e-6 and 4.5e-6 of 1.05), and row by row against the float64 cell of
    tests/cellref.py within cellref.row_bound (emulation err / bound / kernel err: 4.8e-6 / 1.9e-5 / 4.9e-6 and 4.6e-6 / 1.8e-5 /
    4.5e-6; kernel / emulation of the worst row 1.03 and 1.05)"""
    from test_dec_cell_gpu import _cell, _split, _torch_cell
    K = 3
    assert L.lib.ga_dec_cell_supported(N, H, H, Cc, Hd) == 1
    x, w1, b1, wd, bd, w2, b2 = _cell(N // K, H, Cc, Hd, seed=11)
    t1, _, t3 = _torch_cell(x.repeat_interleave(K, dim=0), w1, b1, wd, bd, w2, b2)
    dout = g(N, Cc, H, H, seed=21)
    ps, pb = g(N, Cc, seed=22).abs() * 0.1 + 0.05, g(N, Cc, seed=23) * 0.01
    (gt1,) = torch.autograd.grad((t3 * (dout * ps.view(N, Cc, 1, 1) + pb.view(N, Cc, 1, 1))).sum(), [t1])
    w1f, w2t = w1[:, :, 0, 0].contiguous().to(DEV), w2[:, :, 0, 0].t().contiguous().to(DEV)
    w1h, w1l = _split(w1f)
    w2h, w2l = _split(w2t)
    dt1 = Out(N, H, H, Hd)
    launch(L.DecCellDesc, x=nhwc(x), w1_hi=w1h, w1_lo=w1l, b1=dev(b1), wd=dev(wd.reshape(Hd, 25).t()),
           wd_bwd=dev(wd.flip(2, 3).reshape(Hd, 25).t()), bd=dev(bd), w2_hi=w2h, w2_lo=w2l, dout=nhwc(dout), pro_scale=dev(ps),
           pro_shift=dev(pb), y=dt1, N=N, H=H, W=H, C=Cc, Hd=Hd, backward=1, act_rep=K, variant=variant)
    out = dt1.done()
    assert torch.isfinite(out).all()
    print(f'dec_cell act_rep: kernel err {R.max_err(out.permute(0, 3, 1, 2), gt1):.3e} of {gt1.abs().max().item():.3e}')
    close(out.permute(0, 3, 1, 2), gt1, 2e-4, 'dec_cell backward, act_rep = 3')
    # and row by row against float64, within 4 x the error of the split-bf16 emulation (tests/cellref.py)
    import cellref as CR
    args = [t.contiguous() for t in (x.permute(0, 2, 3, 1), w1[:, :, 0, 0], b1, wd.reshape(Hd, 25).t(), bd, w2[:, :, 0, 0], b2,
                                     dout.permute(0, 2, 3, 1), ps, pb)]
    CR.check_rows('dec_cell backward, act_rep = 3', out, CR.emulate_backward(*args, act_rep=K),
                  CR.cell_backward(*R.f64(*args), act_rep=K))


@pytest.mark.parametrize('K', [1, 3])
def test_sampler_mode1(K):
    """the ND-VAE posterior sample, N = 6, 4 x 6 pixels, NL = 6, ldq = ldp = 16, ldz = 8: forward, backward, backward with
    act_rep = 3.  The sampler's own tolerance: 1e-6 of max |ref| (backward: kernel err 1.3e-5 of 1.7e2).  Pad channels of z / dmu_q / dp keep what the caller left there."""
    N, h, w, NL, ldq, ldz = 6, 4, 6, 6, 16, 8
    Nf = N // K
    mq, p = g(Nf, h, w, 2 * NL, seed=1, scale=3), g(Nf, h, w, 2 * NL, seed=2, scale=3)
    eps, dz = g(Nf, NL, h, w, seed=3), g(N, h, w, NL, seed=4)
    e64 = R.f64(eps).permute(0, 2, 3, 1)
    sm = dict(mu_q=dev(R.pitched(mq, ldq, SENT)), ldq=ldq, p=dev(R.pitched(p, ldq, SENT)), ldp=ldq, eps=dev(eps), eps_nchw=1,
              h=h, w=w, NL=NL, ldz=ldz, mode=1)
    if K == 1:
        z = Out(N, h, w, ldz, fill=SENT)
        launch(L.SamplerDesc, z=z, N=N, **sm)
        out = z.done()
        close(out[..., :NL], R.sampler_nd(*R.f64(mq, p), e64), 1e-6, 'mode 1 forward')
        assert bool((out[..., NL:] == SENT).all())
    dq, dp = Out(N, h, w, ldq, fill=SENT), Out(N, h, w, ldq, fill=SENT)
    launch(L.SamplerDesc, dz=dev(R.pitched(dz, ldz, SENT)), dmu_q=dq, dp=dp, N=N, backward=1, act_rep=K, **sm)
    oq, op = dq.done(), dp.done()
    ref = R.sampler_nd_bwd(*R.f64(mq, p), e64, R.f64(dz), act_rep=K)
    print(f'sampler mode 1 backward K={K}: kernel err {R.max_err(oq[..., :2 * NL], ref):.3e}')
    close(oq[..., :2 * NL], ref, 1e-6, 'mode 1 d mu_q')
    assert torch.equal(oq[..., :2 * NL], op[..., :2 * NL])
    assert bool((oq[..., 2 * NL:] == SENT).all()) and bool((op[..., 2 * NL:] == SENT).all())


# =====================================================================================================================
# B. entry points without a direct test
# =====================================================================================================================
def _adain_run(c):
    x, noise, wn, style, dy = (c[k] for k in ('x', 'noise', 'wn', 'style', 'dy'))
    N, P, C = x.shape
    io = dict(x=dev(x), a=dev(noise), b=dev(wn), c=dev(style), mode=L.GA_AVAE_ADAIN, N=N, P=P, C=C)
    y, st = Out(N, P, C), Out(N, C, 2)
    launch(L.AvaeDesc, y=y, y2=st, **io)
    dx, dgb = Out(N, P, C), Out(N, 2 * C)
    launch(L.AvaeDesc, y=dx, y2=dgb, s=st, dy=dev(dy), backward=1, **io)
    return y.done(), st.done(), dx.done(), dgb.done()


@pytest.mark.parametrize('shape', CS.ADAIN_SHAPES)
def test_avae_adain(shape):
    """NoiseInjection -> LeakyReLU(0.2) -> InstanceNorm -> style affine, forward (y, stats) and backward (dx, dgamma | dbeta).
    fp32-CPU err / bound / kernel err, (3, 35, 36) with noise: y 7.4e-7 / 2.9e-6 / 7.7e-7, stats 2.8e-7 / 1.1e-6 / 3.3e-7,
    dx 1.2e-6 / 4.8e-6 / 1.6e-6, dgamma | dbeta 2.9e-6 / 1.2e-5 / 2.5e-6; without noise: y 6.9e-7 / 2.8e-6 / 8.1e-7,
    dgamma | dbeta 2.0e-6 / 8.1e-6 / 4.5e-6; (2, 1024, 8): y 1.0e-6 / 4.1e-6 / 1.0e-6, dgamma | dbeta 1.3e-5 / 5.1e-5 / 1.2e-5."""
    c = CS.adain_case(*shape)
    y, st, dx, dgb = _adain_run(c)
    args = ('x', 'noise', 'wn', 'style')
    a64, a32 = R.f64(*(c[k] for k in args)), f32(*(c[k] for k in args))
    r64, r32 = R.avae_adain(*a64), R.avae_adain(*a32)
    near('adain y', y, r64[0], r32[0])
    near('adain stats', st, r64[1], r32[1])
    b64, b32 = R.avae_adain_bwd(*a64, R.f64(c['dy'])), R.avae_adain_bwd(*a32, c['dy'])
    near('adain dx', dx, b64[0], b32[0], skip=R.near_kink(R.avae_adain_pre(*a64[:3])))
    near('adain dgamma | dbeta', dgb, b64[1], b32[1])


@pytest.mark.parametrize('shape', CS.ADAIN_SHAPES)
def test_avae_adain_offset_channels(shape):
    """every channel carries a constant of 8 standard deviations: mean^2 is 64 x the variance, which is where a variance formed
    as E[u^2] - mean^2 in fp32 loses its digits.  The kernel's error against float64 may be at most 4 x that of
    torch.nn.functional.instance_norm in fp32 on the CPU on the same u.
    Measured, instance_norm fp32 err / bound / kernel err: (3, 35, 36) with noise 2.0e-6 / 8.1e-6 / 1.7e-6, without
    1.3e-6 / 5.2e-6 / 1.7e-6, (2, 1024, 8) 1.5e-6 / 5.9e-6 / 1.5e-6.  With the variance as E[u^2] - mean^2 the kernel's error
    was 6.6e-5, 1.0e-4 and 4.7e-5 (rstd off by 1.6e-5 .. 3.4e-5 relative): the kernel now sums the mean around the row's first
    pixel and the squares around the mean, each in the fixed order of before."""
    c = CS.adain_case(*shape, offset=8.0)
    y, st, _, _ = _adain_run(c)
    x, noise, wn, style = R.f64(c['x'], c['noise'], c['wn'], c['style'])
    C = x.shape[-1]
    r64 = R.avae_adain(x, noise, wn, style)
    u32 = R._lrelu02(R.avae_adain_pre(c['x'], c['noise'], c['wn']))
    inorm = torch.nn.functional.instance_norm(u32.permute(0, 2, 1).contiguous(), eps=1e-5).permute(0, 2, 1)
    cpu = c['style'][:, None, :C] * inorm + c['style'][:, None, C:]
    e_cpu, e_k = R.max_err(cpu, r64[0]), R.max_err(y, r64[0])
    b = max(4 * e_cpu, 2.0 ** -22 * r64[0].abs().max().item())
    e_rstd = ((st[..., 1].double() - r64[1][..., 1]).abs() / r64[1][..., 1]).max().item()
    print(f'adain offset {shape}: instance_norm fp32 err {e_cpu:.3e}, bound {b:.3e}, kernel err {e_k:.3e}, kernel rstd rel err {e_rstd:.3e}')
    assert torch.isfinite(y).all() and e_k <= b, f'kernel err {e_k:.3e} > 4 x instance_norm fp32 err {e_cpu:.3e}'


@pytest.mark.parametrize('k', [2, 4])
def test_avae_avgpool(k):
    """k x k mean and its adjoint, 8 x 12 x 12 channels.  fp32-CPU err / bound / kernel err: k = 2 9.7e-8 / 4.8e-7 / 1.1e-7, k = 4
    6.7e-8 / 2.7e-7 / 7.4e-8;
    the adjoint is one rounded product: exact."""
    N, H, W, C = 3, 8, 12, 12
    x, dy = g(N, H, W, C, seed=1), g(N, H // k, W // k, C, seed=2)
    y = Out(N, H // k, W // k, C)
    launch(L.AvaeDesc, x=dev(x), y=y, mode=L.GA_AVAE_AVGPOOL, N=N, H=H, W=W, C=C, k=k)
    near('avgpool', y.done(), R.avgpool(R.f64(x), k), R.avgpool(x, k))
    dx = Out(N, H, W, C)
    launch(L.AvaeDesc, x=dev(x), dy=dev(dy), y=dx, mode=L.GA_AVAE_AVGPOOL, N=N, H=H, W=W, C=C, k=k, backward=1)
    exact('avgpool adjoint', dx.done(), R.avgpool_bwd(R.f64(dy), k))


@pytest.mark.parametrize('C', [12, 100, 512])
def test_avae_pixelnorm_and_ga_pixelnorm(C):
    """7 rows (4 per workgroup: the second one is partial).  fp32-CPU err / bound / kernel err, forward (both entry
    points): C = 12 1.7e-7 / 6.8e-7 / 1.6e-7, C = 100 4.3e-7 / 1.7e-6 / 2.8e-7, C = 512 2.1e-7 / 8.9e-7 / 2.3e-7; backward:
    1.8e-7 / 7.1e-7 / 1.8e-7, 3.7e-7 / 1.5e-6 / 3.5e-7, 3.9e-7 / 1.6e-6 / 2.6e-7."""
    rows = 7
    x, dy = g(rows, C, seed=1), g(rows, C, seed=2)
    y, dx, y2 = Out(rows, C), Out(rows, C), Out(rows, C)
    launch(L.AvaeDesc, x=dev(x), y=y, mode=L.GA_AVAE_PIXELNORM, N=rows, C=C)
    launch(L.AvaeDesc, x=dev(x), dy=dev(dy), y=dx, mode=L.GA_AVAE_PIXELNORM, N=rows, C=C, backward=1)
    launch(L.PixelnormDesc, x=dev(x), y=y2, rows=rows, C=C)
    near('avae pixelnorm', y.done(), R.pixelnorm(R.f64(x)), R.pixelnorm(x))
    near('avae pixelnorm backward', dx.done(), R.pixelnorm_bwd(*R.f64(x, dy)), R.pixelnorm_bwd(x, dy))
    near('ga_pixelnorm', y2.done(), R.pixelnorm(R.f64(x)), R.pixelnorm(x))


def test_avae_sample():
    """z = lrelu(m) + eps * exp(0.5 lrelu(v)) * f0 with eps in NCHW, N = 3, P = 35, C = 6.  fp32-CPU err / bound / kernel
    err: forward 3.2e-7 / 1.7e-6 / 5.3e-7, backward 2.0e-7 / 7.9e-7 / 2.1e-7.  The decisions read t itself: no element is left out."""
    c = CS.sample_case()
    t, eps, f0, dz = c['t'], c['eps'], c['f0'], c['dz']
    N, P, C = dz.shape
    z, dt = Out(N, P, C), Out(N, P, 2 * C)
    launch(L.AvaeDesc, x=dev(t), a=dev(eps), y=z, mode=L.GA_AVAE_SAMPLE, N=N, P=P, C=C, f0=f0)
    launch(L.AvaeDesc, x=dev(t), a=dev(eps), dy=dev(dz), y=dt, mode=L.GA_AVAE_SAMPLE, N=N, P=P, C=C, f0=f0, backward=1)
    near('sample', z.done(), R.avae_sample(*R.f64(t, eps), f0), R.avae_sample(t, eps, f0))
    near('sample backward', dt.done(), R.avae_sample_bwd(*R.f64(t, eps), f0, R.f64(dz)), R.avae_sample_bwd(t, eps, f0, dz))


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_unary(mode):
    """n = 1000.  Modes 0, 1, 3 are one or two rounded products; mode 2 is rsqrtf.  fp32-CPU err / bound / kernel err: mode 0
    4.7e-7 / 3.7e-6 / 4.7e-7, mode 1 4.8e-7 / 2.7e-6 / 4.8e-7, mode 2 2.9e-7 / 1.2e-6 / 2.4e-7, mode 3 1.1e-7 / 4.5e-7 / 1.1e-7
    (modes 0 and 1: the 2^-22 floor)."""
    n = 1000
    x = (CS.u(n, seed=1) + 0.1) if mode >= 2 else g(n, seed=1)
    gr = g(n, seed=2)
    y = Out(n)
    launch(L.UnaryDesc, x=dev(x), g=dev(gr), y=y, n=n, mode=mode, eps=1e-8)
    near(f'unary {mode}', y.done(), R.unary(*R.f64(x, gr), mode, 1e-8), R.unary(x, gr, mode, 1e-8))


def test_prelu():
    """rows = 37, C = 12, exact zeros (and a -0.0) take the slope branch.  One rounded product per element: exact."""
    c = CS.prelu_case()
    x, slope, dy = c['x'], c['slope'], c['dy']
    rows, C = x.shape
    y, dx = Out(rows, C), Out(rows, C)
    launch(L.PreluDesc, x=dev(x), slope=dev(slope), y=y, rows=rows, C=C)
    launch(L.PreluDesc, x=dev(x), slope=dev(slope), dy=dev(dy), dx=dx, rows=rows, C=C, backward=1)
    exact('prelu', y.done(), R.prelu(*R.f64(x, slope)))
    exact('prelu backward', dx.done(), R.prelu_bwd(*R.f64(x, slope, dy)))
    assert torch.equal(dx.t.cpu()[0, :4], (dy * slope)[0, :4])


def test_axpby():
    """n = 1001.  fp32-CPU err 2.3e-7, bound 1.2e-6 (the 2^-22 floor), kernel err 2.3e-7.  beta = 0: the engines pass 0 for the FIRST write into a gradient buffer
    that was never initialised (engine_trans / engine_ndvae: `1.0 if g_written else 0.0`), so y's old content, NaN included,
    must not reach the result: y = alpha * x exactly."""
    n = 1001
    x, y0 = g(n, seed=1), g(n, seed=2)
    y = Out.of(dev(y0))
    launch(L.AxpbyDesc, x=dev(x), y=y, n=n, alpha=0.7, beta=-1.3)
    a, b = float(torch.tensor(0.7)), float(torch.tensor(-1.3))          # the scalars as the fp32 arguments carry them
    near('axpby', y.done(), R.axpby(*R.f64(x, y0), a, b), torch.tensor(a) * x + torch.tensor(b) * y0)
    y = Out(n)                                                           # NaN everywhere
    launch(L.AxpbyDesc, x=dev(x), y=y, n=n, alpha=0.7, beta=0.0)
    exact('axpby beta = 0 over NaN', y.done(), R.f64(x) * a)


@pytest.mark.parametrize('k', [1, 2, 4])
@pytest.mark.parametrize('ld', [4, 8])
@pytest.mark.parametrize('band', [0, 2])
def test_pool_denorm(k, ld, band):
    """k x k mean + 0.5 x + 0.5 into the space-to-depth image [N,3,5,4,ld] and its adjoint with and without the NCHW cotangent.
    Lane 3 and the lanes >= 4 are zero, band rows are zero.  fp32-CPU err / bound / kernel err, forward: k = 1 6.0e-8 / 4.2e-7 /
    6.0e-8, k = 2 6.7e-8 / 3.0e-7 / 8.0e-8, k = 4 5.2e-8 / 2.1e-7 / 5.4e-8; backward with the NCHW cotangent: 6.0e-8 / 5.0e-7 /
    6.0e-8, 1.5e-8 / 1.2e-7 / 1.5e-8, 3.7e-9 / 3.1e-8 / 3.7e-9 (all at the 2^-22 floor); without it the result is exact."""
    N, H, W = 3, 6, 10
    x = R.pitched(g(N, H * k, W * k, 3, seed=1), 4, SENT)
    y = Out(N, H // 2, W // 2, 4 * ld)
    launch(L.PoolDenormDesc, x=dev(x), y=y, N=N, H=H, W=W, k=k, ld=ld, band=band)
    out = R.s2d_unpack(y.done(), ld)
    near('pool_denorm', out[..., :3], R.pool_denorm(R.f64(x), k, band), R.pool_denorm(x, k, band))
    assert bool((out[..., 3:] == 0).all())
    if band:
        assert bool((out[:, :band] == 0).all()) and bool((out[:, H - band:] == 0).all())
    dy, dyn = g(N, H, W, 3, seed=2), g(N, 3, H, W, seed=3)
    for nch in (None, dyn):
        dx = Out(N, H * k, W * k, 4)
        launch(L.PoolDenormDesc, dy=dev(R.s2d_pack(dy, ld, SENT)), dy_nchw=dev(nch), dx=dx, N=N, H=H, W=W, k=k, ld=ld, band=band, backward=1)
        o = dx.done()
        near('pool_denorm backward', o[..., :3], R.pool_denorm_bwd(R.f64(dy), None if nch is None else R.f64(nch), k, band),
             R.pool_denorm_bwd(dy, nch, k, band))
        assert bool((o[..., 3] == 0).all())


@pytest.mark.parametrize('act', [L.GA_ACT_FLRELU, L.GA_ACT_NONE])
@pytest.mark.parametrize('with_scale,with_add', [(True, True), (True, False), (False, True), (False, False)])
def test_modout_interleaved(act, with_scale, with_add):
    """StyledConv's tail on plain [N,P,C] tensors, N = 3, P = 35, C = 12, and its backward with the fused reduction at P = 700
    (three pixel segments).  fp32-CPU err / bound / kernel err at FLRELU with scale and add: out 5.3e-7 / 2.1e-6 /
    3.3e-7, dt 2.4e-7 / 1.2e-6 / 2.4e-7, P = 700: out 7.3e-7 / 2.9e-6 / 5.4e-7, dt 4.7e-7 / 1.9e-6 / 4.7e-7, red 9.6e-6 / 3.9e-5 /
    7.6e-6; the least margin of the eight cases: red 4.7e-6 / 2.0e-5 / 6.0e-6."""
    for P, with_red in ((35, False), (700, True)):
        c = CS.modout_case(P)
        t, dout = c['t'], c['dout']
        scale, add = (c['scale'] if with_scale else None), (c['add'] if with_add else None)
        N, _, C = t.shape
        io = dict(t=dev(t), scale=dev(scale), add=dev(add), N=N, P=P, C=C, act=act)
        out, dt = Out(N, P, C), Out(N, P, C)
        launch(L.ModoutDesc, out=out, **io)
        near('modout', out.done(), R.modout(*R.f64(t, scale, add), act), R.modout(t, scale, add, act))
        kw = {}
        if with_red:
            red, ws = Out(N, C), torch.zeros(64 * N * C, device=DEV)
            kw = dict(red=red, ws=ws, ws_floats=ws.numel())
        launch(L.ModoutDesc, dout=dev(dout), dt=dt, backward=1, **io, **kw)
        r64, r32 = R.modout_bwd(*R.f64(t, scale, add), act, R.f64(dout)), R.modout_bwd(t, scale, add, act, dout)
        skip = R.near_kink(R.modout_u(*R.f64(t, scale, add))) if act == L.GA_ACT_FLRELU else None
        near('modout dt', dt.done(), r64[0], r32[0], skip=skip)
        if with_red:
            near('modout red', red.done(), r64[1], r32[1])


@pytest.mark.parametrize('rep', [1, 3])
@pytest.mark.parametrize('with_avg', [True, False])
def test_latent_mix_shared_alpha(rep, with_avg):
    """alpha [J] shared by all rows (alpha_ld = 0), R = 6, J = 5, D = 12.  fp32-CPU err / bound / kernel err: forward
    2.7e-7 / 1.1e-6 / 2.0e-7 (rep 1), 1.8e-7 / 8.8e-7 / 2.1e-7 (rep 3); backward 6.9e-8 / 6.8e-7 / 6.9e-8, 2.0e-7 / 9.9e-7 / 2.0e-7."""
    Rr, J, D = 6, 5, 12
    codes, avg, styles = g(Rr // rep, J, D, seed=1), (g(J, D, seed=2) if with_avg else None), g(Rr, J, D, seed=3)
    alpha, dout = CS.u(J, seed=4), g(Rr, J, D, seed=5)
    out, dc = Out(Rr, J, D), Out(Rr // rep, J, D)
    launch(L.LatentMixDesc, codes=dev(codes), avg=dev(avg), styles=dev(styles), alpha=dev(alpha), out=out, R=Rr, J=J, D=D, rep=rep)
    launch(L.LatentMixDesc, alpha=dev(alpha), dout=dev(dout), dcodes=dc, R=Rr, J=J, D=D, rep=rep, backward=1)
    near('latent_mix', out.done(), R.latent_mix(*R.f64(codes, avg, styles, alpha), rep), R.latent_mix(codes, avg, styles, alpha, rep))
    near('latent_mix backward', dc.done(), R.latent_mix_bwd(*R.f64(dout, alpha), rep), R.latent_mix_bwd(dout, alpha, rep))


# =====================================================================================================================
# C. shapes
# =====================================================================================================================
@pytest.mark.parametrize('H,W,up', [(5, 7, False), (6, 4, False), (4, 6, False), (2, 2, False), (9, 17, False), (12, 36, True)])
def test_dwconv5_odd_and_ragged_shapes(H, W, up):
    """(5, 7) and (9, 17): odd W, single-output strips; (6, 4): W == 4 with H != 4 stays on the windowed kernel; (12, 36): ragged
    8 x 16 windows with up2 forward and pool2 backward.  C = 36 (a partial second chunk), N = 3.  dwconv5's tolerance: 1e-5
    (backward kernel err 1.5e-7 .. 1.2e-6)."""
    N, C = 3, 36
    hs, ws = (H // 2, W // 2) if up else (H, W)
    x, w, b, cot = g(N, hs, ws, C, seed=1), g(25, C, seed=2, scale=0.2), g(C, seed=3), g(N, H, W, C, seed=4)
    y = Out(N, H, W, C)
    launch(L.DwDesc, x=dev(x), w=dev(w), bias=dev(b), y=y, N=N, H=H, W=W, C=C, pro_act=L.GA_ACT_SILU, up2=int(up))
    out = y.done()
    assert torch.isfinite(out).all()
    close(out, R.dwconv5(*R.f64(x, w, b), pro_act=R.SILU, up2=up), 1e-5, 'dwconv5 forward')
    wf = w.view(5, 5, C).flip(0, 1).reshape(25, C)
    dx = Out(N, hs, ws, C)
    launch(L.DwDesc, x=dev(cot), w=dev(wf), dact_x=dev(x), y=dx, N=N, H=H, W=W, C=C, dact_act=L.GA_ACT_SILU, pool2=int(up))
    out = dx.done()
    assert torch.isfinite(out).all()
    print(f'dwconv5 {H}x{W}: backward kernel err {R.max_err(out, R.dwconv5(*R.f64(cot, wf), dact_x=R.f64(x), dact_act=R.SILU, pool2=up)):.3e}')
    close(out, R.dwconv5(*R.f64(cot, wf), dact_x=R.f64(x), dact_act=R.SILU, pool2=up), 1e-5, 'dwconv5 backward')


@pytest.mark.parametrize('skip_mode', [0, 1, 2])
def test_se_apply_and_bilinear_adjoint_non_square(skip_mode):
    """6 x 10 output.  fp32-CPU err / bound / kernel err: skip_mode 0 1.3e-7 / 8.8e-7 / 1.2e-7, skip_mode 1 3.8e-7 / 1.5e-6 /
    4.1e-7, skip_mode 2 1.3e-7 / 8.8e-7 / 1.2e-7, bilinear adjoint 6.3e-7 / 2.5e-6 / 6.8e-7."""
    N, H, W, C = 3, 6, 10, 8
    t, gate = g(N, H, W, C, seed=1), CS.u(N, C, seed=2)
    skip = g(N, *{0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[skip_mode], C, seed=3)
    out = Out(N, H, W, C)
    launch(L.SeApplyDesc, skip=dev(skip), t=dev(t), gate=dev(gate), out=out, N=N, H=H, W=W, C=C, skip_mode=skip_mode, res_scale=0.1)
    rs = float(torch.tensor(0.1))
    near(f'se_apply {skip_mode}', out.done(), R.se_apply(*R.f64(skip, t, gate), rs, skip_mode), R.se_apply(skip, t, gate, rs, skip_mode))
    if skip_mode == 1:
        cot = g(N, H, W, C, seed=4)
        dl = Out(N, H // 2, W // 2, C)
        launch(L.BilinearBwdDesc, dhigh=dev(cot), dlow=dl, N=N, h=H // 2, w=W // 2, C=C)
        near('bilinear adjoint', dl.done(), R.bilinear_up2_adjoint(R.f64(cot)), R.bilinear_up2_adjoint(cot))


# ---- one trip past every capped grid ---------------------------------------------------------------------------------
CAP = 8192 * 256
T = CAP + 257            # work items: the second trip of the grid-stride loop is partial


def _cap_se_apply():
    t, gate = g(1, 1, T, 4, seed=1), CS.u(1, 4, seed=2)
    out = Out(1, 1, T, 4)
    launch(L.SeApplyDesc, t=dev(t), gate=dev(gate), out=out, N=1, H=1, W=T, C=4, skip_mode=0, res_scale=0.5)
    return out, R.f64(gate).view(1, 1, 1, 4) * 0.5 * R.f64(t), (gate.view(1, 1, 1, 4) * 0.5) * t


def _cap_bilinear():
    N, h = 32769, 8                                     # N * 8 * 8 = CAP + 64
    cot = g(N, 2 * h, 2 * h, 4, seed=1)
    dl = Out(N, h, h, 4)
    launch(L.BilinearBwdDesc, dhigh=dev(cot), dlow=dl, N=N, h=h, w=h, C=4)
    return dl, R.bilinear_up2_adjoint(R.f64(cot)), R.bilinear_up2_adjoint(cot)


def _cap_sampler():
    N, NL = T, 1                                        # one pixel, one latent channel per row
    mq, p, eps = g(N, 1, 1, 2, seed=1), g(N, 1, 1, 2, seed=2), g(N, 1, 1, 1, seed=3)
    z = Out(N, 1, 1, 1)
    launch(L.SamplerDesc, mu_q=dev(mq), ldq=2, p=dev(p), ldp=2, eps=dev(eps), z=z, N=N, h=1, w=1, NL=NL, mode=1)
    return z, R.sampler_nd(*R.f64(mq, p, eps)), R.sampler_nd(mq, p, eps)


def _cap_maxpool2():
    x = g(1, 2, 2 * T, 4, seed=1)
    y = Out(1, 1, T, 4)
    launch(L.MaxpoolDesc, x=dev(x), y=y, N=1, H=2, W=2 * T, C=4)
    return y, R.maxpool2(R.f64(x)), None


def _cap_maxpool3s2():
    x = g(1, 2, 2 * T, 4, seed=1)
    y = Out(1, 1, T, 4)
    launch(L.Maxpool3s2Desc, x=dev(x), y=y, N=1, H=2, W=2 * T, C=4)
    return y, R.maxpool3s2(R.f64(x)), None


def _cap_unary():
    x = g(T, seed=1)
    y = Out(T)
    launch(L.UnaryDesc, x=dev(x), y=y, n=T, mode=0)
    return y, R.f64(x) ** 2, None


def _cap_modout():
    t, sc = g(1, T, 4, seed=1), g(1, 4, seed=2)
    out = Out(1, T, 4)
    launch(L.ModoutDesc, t=dev(t), scale=dev(sc), out=out, N=1, P=T, C=4, act=L.GA_ACT_NONE)
    return out, R.f64(sc)[:, None] * R.f64(t), None


def _cap_up2_blur():
    N, H = 8193, 8                                      # forward items = N * 16 * 16 = CAP + 256
    lo, hi0 = g(N, H, H, 4, seed=1), g(N, 2 * H, 2 * H, 4, seed=2)
    hi = Out.of(dev(hi0))
    launch(L.Up2BlurDesc, lo_in=dev(lo), hi=hi, N=N, H=H, W=H, C=4)
    return hi, R.f64(hi0) + R.up2_blur(R.f64(lo)), hi0 + R.up2_blur(lo)


def _cap_latent_mix():
    Rr, J, D = T, 1, 4
    codes, styles, alpha = g(Rr, J, D, seed=1), g(Rr, J, D, seed=2), CS.u(J, seed=3)
    out = Out(Rr, J, D)
    launch(L.LatentMixDesc, codes=dev(codes), styles=dev(styles), alpha=dev(alpha), out=out, R=Rr, J=J, D=D)
    return out, R.latent_mix(R.f64(codes), None, *R.f64(styles, alpha)), R.latent_mix(codes, None, styles, alpha)


def _cap_pool_denorm():
    N, H, W = 1, 2, 1048706                             # pooled pixels = 2 W = CAP + 260 (H and W even)
    x = R.pitched(g(N, H, W, 3, seed=1), 4, SENT)
    y = Out(N, 1, W // 2, 16)
    launch(L.PoolDenormDesc, x=dev(x), y=y, N=N, H=H, W=W, k=1, ld=4)
    want = R.s2d_pack(R.pitched(R.pool_denorm(R.f64(x), 1), 4, 0.0), 4, 0.0)
    return y, want, R.s2d_pack(R.pitched(R.pool_denorm(x, 1), 4, 0.0), 4, 0.0)


def _cap_prelu():
    x, slope = g(T, 4, seed=1), g(4, seed=2)
    y = Out(T, 4)
    launch(L.PreluDesc, x=dev(x), slope=dev(slope), y=y, rows=T, C=4)
    return y, R.prelu(*R.f64(x, slope)), None


def _cap_image_io():
    x = CS.u(1, 1, 1, T, seed=1) * 1.4 - 0.2
    y = Out(1, 1, T, 1)
    launch(L.ImageIoDesc, x_nchw=dev(x), y_nhwc=y, N=1, C=1, H=1, W=T, rep=1)
    return y, R.f64(x).clamp(0, 1).permute(0, 2, 3, 1), None


def _cap_interleave2():
    N, H, W, C = 1, 2, 1048706, 4                       # items = 2 W = CAP + 260 (H and W even)
    planes = [g(N, 1, W // 2, C, seed=i) for i in range(4)]
    y = Out(N, H, W, C)
    launch(L.Interleave2Desc, s=[dev(p) for p in planes], y=y, N=N, H=H, W=W, C=C)
    return y, R.interleave2(list(R.f64(*planes)), N, H, W, C), None


def _cap_rep_sum():
    x = g(3, T, seed=1)
    y = Out(1, T)
    launch(L.RepSumDesc, x=dev(x), y=y, rows=3, inner=T, rep=3, accumulate=0)
    return y, R.rep_sum(x, 3).double(), None             # the fixed order in fp32: exact


def _cap_axpby():
    x, y0 = g(T, seed=1), g(T, seed=2)
    y = Out.of(dev(y0))
    launch(L.AxpbyDesc, x=dev(x), y=y, n=T, alpha=2.0, beta=1.0)
    return y, 2 * R.f64(x) + R.f64(y0), None             # 2 x is exact: one rounding


def _cap_avae_avgpool():
    x = g(1, 1, T, 4, seed=1)
    y = Out(1, 1, T, 4)
    launch(L.AvaeDesc, x=dev(x), y=y, mode=L.GA_AVAE_AVGPOOL, N=1, H=1, W=T, C=4, k=1)
    return y, R.f64(x), None


def _cap_avae_sample():
    t, eps = g(1, T, 2, seed=1), g(1, 1, T, seed=2)
    z = Out(1, T, 1)
    launch(L.AvaeDesc, x=dev(t), a=dev(eps), y=z, mode=L.GA_AVAE_SAMPLE, N=1, P=T, C=1, f0=0.7)
    f0 = float(torch.tensor(0.7))
    return z, R.avae_sample(*R.f64(t, eps), f0), R.avae_sample(t, eps, f0)


def _cap_pixelnorm():
    rows = 4 * 65535 + 5                                # ga_pixelnorm's own cap: 65535 workgroups of 4 rows
    x = g(rows, 4, seed=1)
    y = Out(rows, 4)
    launch(L.PixelnormDesc, x=dev(x), y=y, rows=rows, C=4)
    return y, R.pixelnorm(R.f64(x)), R.pixelnorm(x)


def _cap_resize2_crop():
    N, H, W = 1, 2, 262177                              # output quads = 4 * 2 W = CAP + 264 (attention.hip's grid_for2: 8192 workgroups too)
    x = g(N, H, W, 4, seed=1)
    y = Out(N, 2 * H, 2 * W, 4)
    launch(L.Resize2CropDesc, x=dev(x), y=y, N=N, H=H, W=W, C=4, crop=0)
    return y, R.resize2_crop(R.f64(x), 0), R.resize2_crop(x, 0)


def _cap_gconv_generic():
    Wi, cg = 699137, 12                                 # cg = 12 has no LDS-weights kernel; pixels * 3 quads = CAP + 259
    x, w, b = g(1, 1, Wi, cg, seed=1), g(cg, cg, seed=2, scale=0.3), g(cg, seed=3)
    y = Out(1, 1, Wi, cg)
    launch(L.GconvDesc, x=dev(x), w=dev(w), bias=dev(b), y=y, N=1, Hi=1, Wi=Wi, Ho=1, Wo=Wi, C=cg, cg=cg, KH=1, KW=1, stride=1, pad=0)
    x64, w64, b64 = R.f64(x, w, b)
    return y, x64 @ w64.t() + b64, x @ w.t() + b        # one group, one tap: a 12 x 12 matrix per pixel


CAPPED = dict(se_apply=_cap_se_apply, bilinear_up2_bwd=_cap_bilinear, sampler_mix=_cap_sampler, maxpool2=_cap_maxpool2,
              maxpool3s2=_cap_maxpool3s2, unary=_cap_unary, modout=_cap_modout, up2_blur=_cap_up2_blur, latent_mix=_cap_latent_mix,
              pool_denorm=_cap_pool_denorm, prelu=_cap_prelu, image_io=_cap_image_io, interleave2=_cap_interleave2,
              rep_sum=_cap_rep_sum, axpby=_cap_axpby, avae_avgpool=_cap_avae_avgpool, avae_sample=_cap_avae_sample,
              pixelnorm=_cap_pixelnorm, resize2_crop=_cap_resize2_crop, gconv_generic=_cap_gconv_generic)


@pytest.mark.parametrize('op', list(CAPPED))
def test_second_trip_of_the_capped_grid(op):
    """every entry point whose grid is capped at 8192 workgroups (ga_pixelnorm: 65535) with 8192 * 256 + 257 work items, or
    the nearest its shape rules allow, at its narrowest channel count: the grid-stride loop takes a second, partial trip.
    The WHOLE output is compared: exactly where the op is a selection, a copy or one rounded operation (the builder returns
    no fp32 result), else by the new-op rule.  resize2_crop's grid comes from attention.hip's own capping helper (8192 workgroups
    as well): fp32-CPU err / bound / kernel err 4.1e-7 / 1.6e-6 / 3.5e-7; gconv_generic is ga_gconv's grid-stride kernel (cg = 12, one
    tap): 1.1e-6 / 4.4e-6 / 8.0e-7."""
    out, ref, fp32 = CAPPED[op]()
    got = out.done()
    if fp32 is None:
        exact(op, got, ref)
    else:
        near(op, got, ref, fp32)
