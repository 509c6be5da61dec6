"""
CPU: tests/planref.py, the float64 interpreter of the non-conv plan descriptors, checked without a GPU.
  1. Field accounting: every non-conv, non-cell descriptor of the dry-run plans of tests/planzoo.py (every shipped defender and
     its K-cotangent / alpha_rows / alpha_grad variants) has a handler, sets no field its handler does not read, and has
     consistent extents (rows divisible by the replica fields, pitches >= channel counts: planref.capture refuses otherwise).
     The same holds for the reduced engines the GPU test adds to its pool (planzoo.device_engines, built dry here).
  2. The interpreter against opref: for every kind (and every mode of ga_sampler_mix, ga_latent_mix and ga_avae) a synthetic
     descriptor with pitched, sliced, aliased and in-place buffers laid out by planref.Buffers, a replica field > 1 where the op
     has one and accumulate / in-place where it allows it, gives exactly what the matching opref call gives on dense tensors.
  3. Kink cap: on the seeds the GPU test uses (planref.seed_of), the reference alone leaves out at most opref.KINK_CAP of the
     elements of any output, at the reduced row count of the smallest member of every class.
"""
import collections
import itertools

import pytest
import torch

import opref as R
import planref as PR
import planzoo
from gen_adversarial_amd import _lib as L


@pytest.fixture(scope='module')
def zoo():
    """distinct PlanOps of the dry-run plans and capture failures"""
    ops, fails = {}, []
    more = ((name, build()) for name, build in planzoo.device_engines('cpu', dry_run=True))
    for name, eng in itertools.chain(planzoo.dry_engines(), more):
        for plan, tag in ((eng.fwd, 'fwd'), (eng.bwd, 'bwd')):
            for d, nm in zip(plan.descs, plan.names):
                if isinstance(d, PR.ELSEWHERE):
                    continue
                where = f'{name}.{tag}.{nm}'
                try:
                    op = PR.capture(d, where)
                except PR.PlanRefError as ex:
                    fails.append(f'{where}: {ex}')
                    continue
                if op.key in ops:
                    ops[op.key].where.append(where)
                else:
                    ops[op.key] = op
    return list(ops.values()), fails


def test_every_plan_descriptor_is_read_by_its_handler(zoo):
    ops, fails = zoo
    per = collections.Counter(op.cls.__name__ for op in ops)
    print('\ndistinct non-conv descriptors per kind: ' + ', '.join(f'{k} {v}' for k, v in sorted(per.items())))
    assert not fails, '\n'.join(fails[:40])
    assert set(per) == {c.__name__ for c in PR.HANDLERS}, 'a handler no shipped plan uses, or the zoo lost a kind'
    listed = {o.cls for o in L._H.ops}
    assert listed == set(PR.HANDLERS) | set(PR.ELSEWHERE)      # every line of GA_OP_LIST is accounted for
    for op in ops:
        small = op.with_rows()
        h = op.h
        if h.rows is not None:
            assert small.f[h.rows] == h.least_rows(op.f, op.has) and op.f[h.rows] % small.f[h.rows] == 0, op.label()
        for k, v in small.h.operands(small.f, small.has).items():
            assert v.ld >= v.used


def test_a_field_no_reference_reads_is_refused():
    d = L.LayernormDesc()
    d.a, d.gamma, d.beta, d.y, d.stats = 4096, 8192, 12288, 1 << 14, 1 << 15
    d.rows, d.C, d.eps = 4, 8, 1e-5
    PR.capture(d)
    d.accumulate = 1                                   # read by the backward only
    with pytest.raises(PR.PlanRefError, match='accumulate'):
        PR.capture(d)
    m = L.ModoutDesc()
    m.t = m.out = 4096
    m.N, m.P, m.C, m.act = 2, 16, 8, 5
    assert PR.capture(m).groups == ((('out', 0), ('t', 0)),)          # in place: one storage
    m.dt = 8192                                        # a backward output on a forward launch
    with pytest.raises(PR.PlanRefError):
        PR.capture(m)
    s = L.SamplerDesc()
    s.mu_q, s.eps, s.z = 4096, 1 << 14, 1 << 15
    s.N, s.h, s.w, s.NL, s.ldq, s.q_rep = 4, 2, 2, 4, 8, 3
    with pytest.raises(PR.PlanRefError, match='q_rep'):              # 4 rows on 3 replicas
        PR.capture(s)


def test_operands_that_overlap_without_being_one_tensor_are_refused():
    """equal pointers and channel slices of operands with the same extent are rebuilt as one storage; any other overlap would
    be rebuilt as two tensors and pass as unaliased, so the descriptor is refused"""
    d = L.LayernormDesc()
    d.a, d.gamma, d.beta, d.y, d.stats = 4096, 8192, 12288, 1 << 14, 1 << 15
    d.rows, d.C, d.eps = 4, 8, 1e-5
    d.gamma = 4096                                     # equal pointers, [rows, C] and [C]
    with pytest.raises(PR.PlanRefError, match='a and gamma overlap'):
        PR.capture(d)
    d.gamma, d.y = 8192, 4096 + 4 * 8 * 2              # y two rows into a
    with pytest.raises(PR.PlanRefError, match='a and y overlap'):
        PR.capture(d)
    d.y = 4096 + 4 * 8 * 4                             # y right behind a's last row
    PR.capture(d)


def _op(cls, f, ptr):
    return PR.capture(PR.make_desc(cls, f, ptr), 'synthetic')


def _run(op, seed=3):
    b = PR.Buffers(op, 'cpu', seed)
    t = b.inputs(torch.float64)
    return b, t, PR.reference(op, t)


def test_interpreter_modout_planes_are_slices_of_one_pitched_tensor():
    """t and dt in depth-to-space form, ld_planes = 4C: the four planes are channel slices of one [N, H/2, W/2, 4C] tensor"""
    N, H, W, C = 2, 4, 6, 8
    base, dbase = 1 << 20, 1 << 22
    f = dict(N=N, P=H * W, C=C, act=5, backward=1, W=W, ld_planes=4 * C, ws_floats=4 * N * C)
    ptr = dict(scale=4096, add=8192, dout=1 << 16, red=1 << 18, ws=1 << 19)
    ptr.update({f't_planes{i}': base + 4 * C * i for i in range(4)})
    ptr.update({f'dt_planes{i}': dbase + 4 * C * i + 8 for i in range(4)})        # 8 bytes off a 16-byte boundary
    op = _op(L.ModoutDesc, f, ptr)
    assert (('t_planes0', 0), ('t_planes1', C), ('t_planes2', 2 * C), ('t_planes3', 3 * C)) in op.groups and ('dt_planes0', 2) in op.align
    b, t, r = _run(op)
    whole = b.store[[g[0][0] for g in op.groups].index('t_planes0')][:N * (H // 2) * (W // 2) * 4 * C].view(N, H // 2, W // 2, 2, 2, C).double()
    dense = whole.permute(0, 1, 3, 2, 4, 5).reshape(N, H * W, C)                    # pixel (h, w) from plane (h&1)*2 + (w&1)
    dt, red = R.modout_bwd(dense, t['scale'], t['add'], 5, t['dout'])
    assert torch.equal(r['red'].value, red)
    got = torch.zeros(N, H, W, C, dtype=torch.float64)
    for i in range(4):
        got[:, i // 2::2, i % 2::2] = r[f'dt_planes{i}'].value
    assert torch.equal(got.view(N, H * W, C), dt) and 'dt' not in r


def test_interpreter_reduce_in_place_skip_and_formed_operand():
    N, P, C = 2, 9, 12
    f = dict(N=N, P=P, C=C, scale=0.5)
    op = _op(L.ReduceDesc, f, dict(a_src=4096, a_w=8192, b=1 << 16, out=1 << 17, gate=1 << 18, skip=1 << 20, scaled=1 << 20))
    assert (('scaled', 0), ('skip', 0)) in op.groups
    b, t, r = _run(op)
    assert b.role['scaled'] == 'inout' and torch.equal(t['skip'], t['scaled'])
    out, scaled = R.rowchan_reduce(None, t['b'], 0.5, t['gate'], t['skip'], t['a_src'], t['a_w'])
    assert torch.equal(r['out'].value, out) and torch.equal(r['scaled'].value, scaled)


def test_interpreter_interleave2_sliced_sources_and_replicas():
    N, H, W, C, K = 6, 4, 4, 8, 3
    f = dict(N=N, H=H, W=W, C=C, dact_act=3, lds=4 * C, dact_rep=K)
    ptr = dict(y=1 << 20, addend=1 << 20, dact_x=1 << 16)
    ptr.update({f's{i}': (1 << 22) + 4 * C * i for i in range(4)})
    op = _op(L.Interleave2Desc, f, ptr)
    assert op.with_rows().f['N'] == K
    b, t, r = _run(op)
    assert t['dact_x'].shape[0] == N // K and b.role['y'] == 'inout'
    want = R.interleave2([t[f's{i}'] for i in range(4)], N, H, W, C, t['dact_x'], addend=t['addend'], dact_act=R.RELU, dact_rep=K)
    assert torch.equal(r['y'].value, want)
    src = b.store[[g[0][0] for g in op.groups].index('s0')]
    assert bool((src[C * 4 * N * (H // 2) * (W // 2):] == torch.tensor(PR.POISON)).all())    # the sentinel row behind the planes


def test_interpreter_attn_thirds_of_one_projection():
    N, Tk, heads, dh = 2, 5, 2, 16
    E = heads * dh
    f = dict(N=N, Tq=16, Tk=16, heads=heads, dh=dh, scale=dh ** -0.5, ldq=3 * E, ldk=3 * E, ldv=3 * E, ldo=E)
    op = _op(L.AttnDesc, f, dict(q=1 << 20, k=(1 << 20) + 4 * E, v=(1 << 20) + 8 * E, out=1 << 16, p=1 << 18))
    gi = op.groups.index((('k', E), ('q', 0), ('v', 2 * E)))
    b, t, r = _run(op)
    whole = b.store[gi][:N * 16 * 3 * E].view(N, 16, 3 * E).double()
    out, p = R.attn(whole[..., :E], whole[..., E:2 * E], whole[..., 2 * E:], heads, op.f['scale'])
    assert torch.equal(r['out'].value, out) and torch.equal(r['p'].value, p)


def test_interpreter_layernorm_accumulates_and_sampler_pitches():
    op = _op(L.LayernormDesc, dict(rows=5, C=12, eps=1e-5, backward=1, accumulate=1), dict(a=4096, b=8192, gamma=1 << 14, stats=1 << 15, dy=1 << 16, dx=1 << 17))
    b, t, r = _run(op)
    assert torch.equal(r['dx'].value, t['dx'] + R.layernorm_bwd(t['a'], t['b'], t['gamma'], op.f['eps'], t['dy']))
    f = dict(N=6, h=2, w=3, NL=4, ldq=8, ldp=12, ldz=8, eps_nchw=1, q_rep=3, alpha=0.25, one_minus_alpha=0.75, temp=0.6)
    op = _op(L.SamplerDesc, f, dict(mu_q=4096, p=1 << 14, eps=1 << 16, z=1 << 18))
    assert op.with_rows().f['N'] == 3
    b, t, r = _run(op)
    assert t['mu_q'].shape == (2, 2, 3, 4) and t['eps'].shape == (6, 4, 2, 3) and float(b.view['mu_q'].max()) < 1e3
    mq = t['mu_q'].repeat_interleave(3, dim=0)
    want = R.sampler_mix(mq, t['p'][..., :4], t['p'][..., 4:], t['eps'].permute(0, 2, 3, 1), 0.25, 0.75, op.f['temp'])
    assert torch.equal(r['z'].value, want)
    # the backward formulas of opref.sampler_mix against autograd of the forward
    leaves = [v.clone().requires_grad_(True) for v in (mq, t['p'][..., :4], t['p'][..., 4:])]
    dz = torch.randn(want.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    g = torch.autograd.grad((R.sampler_mix(*leaves, t['eps'].permute(0, 2, 3, 1), 0.25, 0.75, 0.6) * dz).sum(), leaves)
    for a, c in zip(g, R.sampler_mix_bwd(mq, t['p'][..., :4], t['p'][..., 4:], t['eps'].permute(0, 2, 3, 1), dz, 0.25, 0.75, 0.6)):
        assert (a - c).abs().max().item() < 1e-12


def A(i):
    return (i + 1) << 22


def P(*names, **same):
    """distinct addresses for `names`; name=other puts name at other's address (alias)"""
    p = {n: A(i) for i, n in enumerate(names)}
    p.update({n: p[o] for n, o in same.items()})
    return p


def _s2d_dense(v):
    N, h, w, _, c = v.shape
    return R.s2d_unpack(v.reshape(N, h, w, 4 * c), c)


def _s2d(img, ld):
    N, H, W, _ = img.shape
    return R.s2d_pack(img, ld, 0.0).view(N, H // 2, W // 2, 4, ld)


def _maxpool3_bwd(x, dy, K):
    xr = R.rep_rows(x, K).clone().requires_grad_(True)
    return torch.autograd.grad((R.maxpool3s2(xr) * dy).sum(), [xr])[0]


def _up2_blur_adj(hi, shape):
    lo = torch.zeros(shape, dtype=hi.dtype, requires_grad=True)
    return torch.autograd.grad((R.up2_blur(lo) * hi).sum(), [lo])[0]


def _mix_parts(t, q, K):
    mq = R.rep_rows(R.rep_rows(t['mu_q'], q), K)
    p = R.rep_rows(t['p'], K)
    return mq, p[..., :4], p[..., 4:], R.rep_rows(t['eps'].permute(0, 2, 3, 1), K)


def _mode2(t, f):
    term = R.sampler_alpha_terms(*_mix_parts(t, 2, 1), t['dz'], f['temp'])
    z = torch.zeros(4, 5, 1, dtype=torch.float64)
    z[:, 3, 0] = term.flatten(1).sum(dim=1)
    return dict(z=z)


SMP = dict(N=4, h=2, w=3, NL=4, ldq=8, ldp=12, ldz=8, eps_nchw=1, temp=0.6)
# (id, descriptor type, fields, pointers, expected outputs from the dense inputs t and the fields f as the descriptor holds them)
KINDS = [
    ('dw', L.DwDesc, dict(N=6, H=4, W=6, C=8, dact_act=1, pool2=1, act_rep=3), P('x', 'w', 'dact_x', 'y'),
     lambda t, f: dict(y=R.dwconv5(t['x'], t['w'], None, t['dact_x'], 0, R.SILU, False, True, 3))),
    ('se_apply', L.SeApplyDesc, dict(N=2, H=4, W=4, C=8, skip_mode=1, res_scale=0.1), P('skip', 't', 'gate', 'out'),
     lambda t, f: dict(out=R.se_apply(t['skip'], t['t'], t['gate'], f['res_scale'], 1))),
    ('se_excite_bwd', L.SeExciteDesc, dict(N=4, C=8, Hd=4, P=6, res_scale=0.1, backward=1, act_rep=2),
     P('t', 'w1', 'b1', 'w2', 'b2', 'hid', 'gate', 'dout', 'pro_scale', 'pro_shift'),
     lambda t, f: dict(zip(('pro_scale', 'pro_shift'), R.se_excite_bwd_fused(t['t'], t['dout'], t['hid'], t['gate'], t['w1'], t['w2'], f['res_scale'], 2)))),
    ('se_excite_unfused', L.SeExciteDesc, dict(N=3, C=8, Hd=4, P=6, res_scale=0.1), P('m', 'w1', 'b1', 'w2', 'b2', 'hid', 'gate'),
     lambda t, f: dict(zip(('hid', 'gate'), R.se_excite_fwd(t['m'], t['w1'], t['b1'], t['w2'], t['b2'])))),
    ('bilinear_bwd', L.BilinearBwdDesc, dict(N=2, h=3, w=3, C=4, accumulate=1), P('dhigh', 'dlow'),
     lambda t, f: dict(dlow=t['dlow'] + R.bilinear_up2_adjoint(t['dhigh']))),
    ('maxpool_bwd', L.MaxpoolDesc, dict(N=4, H=4, W=4, C=4, backward=1, act_rep=2), P('x', 'dy', 'dx'),
     lambda t, f: dict(dx=R.maxpool2_bwd(t['x'], t['dy'], 2))),
    ('avgpool_act_bwd', L.AvgpoolActDesc, dict(N=4, P=5, C=8, act=3, backward=1, act_rep=2), P('x', 'dy', 'dx'),
     lambda t, f: dict(dx=R.avgpool_act_bwd(t['x'], R.RELU, t['dy'], 2))),
    ('axpby', L.AxpbyDesc, dict(n=12, alpha=2.0, beta=0.5), P('x', 'y'), lambda t, f: dict(y=R.axpby(t['x'], t['y'], 2.0, 0.5))),
    ('rep_sum', L.RepSumDesc, dict(rows=6, inner=8, rep=3, accumulate=1), P('x', 'y'), lambda t, f: dict(y=t['y'] + R.rep_sum(t['x'], 3))),
    ('pixelnorm', L.PixelnormDesc, dict(rows=3, C=8), P('x', 'y'), lambda t, f: dict(y=R.pixelnorm(t['x']))),
    ('prelu_bwd', L.PreluDesc, dict(rows=5, C=8, backward=1), P('x', 'slope', 'dy', 'dx'),
     lambda t, f: dict(dx=R.prelu_bwd(t['x'], t['slope'], t['dy']))),
    ('unary_in_place', L.UnaryDesc, dict(n=16, mode=3), P('x', 'g', y='g'), lambda t, f: dict(y=R.unary(t['x'], t['y'], 3))),
    ('up2_blur', L.Up2BlurDesc, dict(N=2, H=3, W=3, C=4), P('lo_in', 'hi'), lambda t, f: dict(hi=t['hi'] + R.up2_blur(t['lo_in']))),
    ('up2_blur_bwd', L.Up2BlurDesc, dict(N=2, H=3, W=3, C=4, backward=1), P('hi_in', 'lo'),
     lambda t, f: dict(lo=_up2_blur_adj(t['hi_in'], (2, 3, 3, 4)))),
    ('latent_mix_rows', L.LatentMixDesc, dict(R=4, J=3, D=8, rep=2, alpha_ld=5), P('codes', 'avg', 'styles', 'alpha', 'out'),
     lambda t, f: dict(out=R.latent_mix_rows(t['codes'], t['avg'], t['styles'], t['alpha'], 2))),
    ('latent_mix_rows_bwd', L.LatentMixDesc, dict(R=4, J=3, D=8, rep=2, alpha_ld=5, backward=1), P('dout', 'alpha', 'dcodes'),
     lambda t, f: dict(dcodes=R.latent_mix_rows_bwd(t['dout'], t['alpha'], 2))),
    ('latent_mix_shared_bwd', L.LatentMixDesc, dict(R=4, J=3, D=8, rep=2, backward=1), P('dout', 'alpha', 'dcodes'),
     lambda t, f: dict(dcodes=R.latent_mix_bwd(t['dout'], t['alpha'], 2))),
    ('latent_mix_dalpha', L.LatentMixDesc, dict(R=4, J=3, D=8, rep=2, backward=2), P('codes', 'avg', 'styles', 'dout', 'out'),
     lambda t, f: dict(out=R.latent_alpha_terms(t['codes'], t['avg'], t['styles'], t['dout'], 2).sum(dim=-1))),
    ('resize2_crop_bwd', L.Resize2CropDesc, dict(N=2, H=4, W=4, C=4, crop=1, backward=1, accumulate=1), P('dy', 'dx'),
     lambda t, f: dict(dx=t['dx'] + R.resize2_crop_adjoint(t['dy'], 1))),
    ('maxpool3s2_bwd', L.Maxpool3s2Desc, dict(N=4, H=6, W=6, C=4, backward=1, act_rep=2), P('x', 'dy', 'dx'),
     lambda t, f: dict(dx=_maxpool3_bwd(t['x'], t['dy'], 2))),
    ('sampler_bwd_q_rep', L.SamplerDesc, dict(SMP, alpha=0.25, one_minus_alpha=0.75, q_rep=2, backward=1), P('mu_q', 'p', 'eps', 'dz', 'dmu_q_rows', 'dp'),
     lambda t, f: (lambda g: dict(dmu_q_rows=g[0], dp=torch.cat(g[1:], dim=-1)))(R.sampler_mix_bwd(*_mix_parts(t, 2, 1), t['dz'], 0.25, 0.75, f['temp']))),
    ('sampler_bwd_act_rep', L.SamplerDesc, dict(SMP, alpha=0.25, one_minus_alpha=0.75, q_rep=1, backward=1, act_rep=2), P('mu_q', 'p', 'eps', 'dz', 'dmu_q', 'dp'),
     lambda t, f: (lambda g: dict(dmu_q=g[0], dp=torch.cat(g[1:], dim=-1)))(R.sampler_mix_bwd(*_mix_parts(t, 1, 2), t['dz'], 0.25, 0.75, f['temp']))),
    ('sampler_nd', L.SamplerDesc, dict(SMP, ldq=12, mode=1), P('mu_q', 'p', 'eps', 'z'),
     lambda t, f: dict(z=R.sampler_nd(t['mu_q'], t['p'], t['eps'].permute(0, 2, 3, 1)))),
    ('sampler_nd_bwd', L.SamplerDesc, dict(SMP, ldq=12, mode=1, backward=1, act_rep=2), P('mu_q', 'p', 'eps', 'dz', 'dmu_q', 'dp'),
     lambda t, f: (lambda g: dict(dmu_q=g, dp=g))(R.sampler_nd_bwd(t['mu_q'], t['p'], t['eps'].permute(0, 2, 3, 1), t['dz'], 2))),
    ('sampler_dalpha', L.SamplerDesc, dict(SMP, q_rep=2, mode=2, backward=1, alpha_ld=5, alpha_col=3), P('mu_q', 'p', 'eps', 'dz', 'z'), _mode2),
    ('dml_bwd', L.DmlDesc, dict(ld=104, nmix=10, N=4, H=2, W=3, backward=1, ld_img=8, act_rep=2), P('logits', 'dimg_nhwc', 'dimg_nchw', 'dlogits'),
     lambda t, f: dict(dlogits=R.pitched(R.dml_mean_bwd(t['logits'], 10, t['dimg_nhwc'] + t['dimg_nchw'].permute(0, 2, 3, 1), 2), 104, 0.0))),
    ('dml', L.DmlDesc, dict(ld=104, nmix=10, N=2, H=2, W=3, ld_img=8), P('logits', 'img_nchw', 'img_nhwc'),
     lambda t, f: dict(img_nchw=R.dml_mean(t['logits'], 10).permute(0, 3, 1, 2), img_nhwc=R.pitched(R.dml_mean(t['logits'], 10), 8, 0.0))),
    ('image_io_bwd', L.ImageIoDesc, dict(N=8, C=3, H=4, W=4, rep=2, backward=1, ld=8, s2d=1, cot_rep=2), P('x_nchw', 'noise_nchw', 'noise_coef', 'dy_nhwc', 'dx_nchw'),
     lambda t, f: dict(dx_nchw=R.image_io_bwd(t['x_nchw'], t['noise_nchw'], t['noise_coef'], 2, _s2d_dense(t['dy_nhwc']), 2))),
    ('image_io', L.ImageIoDesc, dict(N=4, C=3, H=4, W=4, rep=2, ld=8), P('x_nchw', 'noise_nchw', 'noise_coef', 'y_nhwc'),
     lambda t, f: dict(y_nhwc=R.pitched(R.image_io(t['x_nchw'], t['noise_nchw'], t['noise_coef'], 2), 8, 0.0))),
    ('blur_adjoint', L.BlurDesc, dict(planes=2, H=8, W=10, k=5, radius=1, backward=1), P('x', 'y', 'taps'),
     lambda t, f: dict(y=R.gauss_blur_adjoint(t['x'], t['taps'], 1))),
    ('gconv', L.GconvDesc, dict(N=4, Hi=4, Wi=4, Ho=4, Wo=4, C=8, cg=4, KH=3, KW=3, stride=1, pad=1, dact_act=3, dact_rep=2), P('x', 'w', 'dact_x', 'y'),
     lambda t, f: dict(y=R.gconv(t['x'], t['w'], None, 4, 3, 3, 1, 1, 4, 4, dact_x=t['dact_x'], dact_act=R.RELU, dact_rep=2))),
    ('pool_denorm_bwd', L.PoolDenormDesc, dict(N=2, H=4, W=4, k=2, ld=8, backward=1, band=1), P('dy', 'dy_nchw', 'dx'),
     lambda t, f: dict(dx=R.pitched(R.pool_denorm_bwd(_s2d_dense(t['dy']), t['dy_nchw'], 2, 1), 4, 0.0))),
    ('pool_denorm', L.PoolDenormDesc, dict(N=2, H=4, W=4, k=2, ld=8, band=1), P('x', 'y'),
     lambda t, f: dict(y=_s2d(R.pool_denorm(R.pitched(t['x'], 4, 0.0), 2, 1), 8))),
    ('avae_adain_bwd', L.AvaeDesc, dict(mode=0, backward=1, N=4, P=6, C=4, act_rep=2), P('x', 'a', 'b', 'c', 's', 'dy', 'y', 'y2'),
     lambda t, f: dict(zip(('y', 'y2'), R.avae_adain_bwd(R.rep_rows(t['x'], 2), R.rep_rows(t['a'], 2), t['b'], R.rep_rows(t['c'], 2), t['dy'])))),
    ('avae_avgpool', L.AvaeDesc, dict(mode=1, N=2, H=4, W=4, C=4, k=2), P('x', 'y'), lambda t, f: dict(y=R.avgpool(t['x'], 2))),
    ('avae_pixelnorm_bwd', L.AvaeDesc, dict(mode=2, backward=1, N=4, C=8, act_rep=2), P('x', 'dy', 'y'),
     lambda t, f: dict(y=R.pixelnorm_bwd(R.rep_rows(t['x'], 2), t['dy']))),
    ('avae_sample_bwd', L.AvaeDesc, dict(mode=3, backward=1, N=4, P=6, C=4, f0=0.6, act_rep=2), P('x', 'a', 'dy', 'y'),
     lambda t, f: dict(y=R.avae_sample_bwd(R.rep_rows(t['x'], 2), R.rep_rows(t['a'], 2), f['f0'], t['dy']))),
]


@pytest.mark.parametrize('case', KINDS, ids=[c[0] for c in KINDS])
def test_interpreter_against_opref(case):
    _, cls, f, ptr, expect = case
    op = _op(cls, f, ptr)
    small = op.with_rows()
    assert op.h.rows is None or op.f[op.h.rows] % small.f[op.h.rows] == 0
    b, t, r = _run(op)
    want = expect(t, op.f)
    assert set(want) == set(r)
    for k, v in want.items():
        assert r[k].value.shape == v.shape and torch.equal(r[k].value, v), k
        assert b.view[k].shape == v.shape                                   # the extent the handler derived holds the result
    for st in b.store:                                                      # every buffer ends in a poisoned sentinel row
        assert float(st[-1]) == float(torch.tensor(PR.POISON))


def test_every_kind_has_a_synthetic_case():
    assert {c[1] for c in KINDS} | {L.ModoutDesc, L.ReduceDesc, L.Interleave2Desc, L.AttnDesc, L.LayernormDesc} == set(PR.HANDLERS)


def test_kink_exclusions_stay_under_the_cap(zoo):
    """per class the member with the fewest pixels, at its least row count, on the GPU test's seed"""
    ops = zoo[0]
    by = {}
    for op in ops:
        by.setdefault(op.klass(), []).append(op)
    worst, n = {}, 0
    for k in sorted(by, key=repr):
        op = min(by[k], key=lambda o: (o.pixels(), repr(o.key))).with_rows()
        b = PR.Buffers(op, 'cpu', PR.seed_of(op))
        for name, res in PR.reference(op, b.inputs(torch.float64)).items():
            if res.skip is None or res.tol is not None:
                continue
            n += 1
            share = res.skip.double().mean().item()
            worst[op.cls.__name__] = max(worst.get(op.cls.__name__, 0.0), share)
            assert share <= R.KINK_CAP, f'{op.label()} {name}: {share:.2e} of the elements sit on a kink'
    print(f'\n{n} kinked outputs; largest excluded share per kind: ' + ', '.join(f'{k} {v:.1e}' for k, v in sorted(worst.items())))
    assert n > 20
