"""
CPU: the host side of the K-cotangent backward plan of the bare ResNet-50 / ResNeXt-50 classifiers —
`Engine(None, None, ..., resnet_spec, cot_rep=K)` builds in dry-run mode, with input noise and with blur too; every backward
descriptor counts rows x K cotangent rows and every one that reads a tensor of the forward pass says so in its replica field
(`dact_rep` of ga_conv_desc / ga_interleave2_desc / ga_gconv_desc, `cot_rep` of ga_image_io_desc, `act_rep` of the two pools);
a purifier in front of a ResNet stays refused; the descriptor layouts did not move.  No kernel is launched.
"""
import ctypes as C

import pytest

from gen_adversarial_amd import _lib as L
from gen_adversarial_amd.engine import Engine
from gen_adversarial_amd.nvae_spec import init_nvae_state_dict
from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict

K = 3
RES = (3, 64, 64)
# 'resnet_id': a second block in layer 1, i.e. an identity shortcut, whose cotangent passes relu' through GA_CONV_ADDEND_PRE_DACT
NETS = {'resnet': (4, 8, (1, 1, 1, 1)), 'resnext': (4, 2, (1, 1, 1, 1), 4, 8), 'resnet_id': (4, 8, (2, 1, 1, 1))}
FRONTS = {'plain': dict(rows=2, rep=1), 'noise': dict(rows=4, rep=2, noise_eps=0.05), 'blur': dict(rows=2, rep=2, blur=True)}
REP_FIELD = {L.ConvDesc: 'dact_rep', L.Interleave2Desc: 'dact_rep', L.GconvDesc: 'dact_rep', L.ImageIoDesc: 'cot_rep'}   # others: act_rep


def _engine(net, front, **kw):
    a = NETS[net]
    rspec, rsd = build_resnet_spec(*a), init_resnet_state_dict(a[0], a[1], 3, *a[2:])
    return Engine(None, None, RES, rsd, rspec, alphas=[], device='cpu', dry_run=True, **FRONTS[front], **kw)


def _pointers(d):
    return {name: getattr(d, name) for name, typ in d._fields_ if typ is L.fp and getattr(d, name)}


def _rows(d):
    """the row count of a backward descriptor, in cotangent rows"""
    return d.planes // 3 if isinstance(d, L.BlurDesc) else d.N


@pytest.mark.parametrize('front', list(FRONTS))
@pytest.mark.parametrize('net', list(NETS))
def test_backward_plan_carries_the_cotangent_count(net, front):
    eng = _engine(net, front, cot_rep=K)               # ValueError without the ResNet-side plan
    rows, images = FRONTS[front]['rows'], FRONTS[front]['rows'] // FRONTS[front]['rep']
    assert eng.cot_rep == K
    assert eng.dlogits.shape[0] == rows * K and eng.dx.shape[0] == images * K and eng.logits.shape[0] == rows
    fwd = {a.t.data_ptr(): name for name, a in eng.acts.items()}            # the tensors of the forward pass, by base address
    grads = {a._g.data_ptr() for a in eng.acts.values() if a._g is not None}
    for a in eng.acts.values():
        assert a.t.shape[0] == rows and (a._g is None or a._g.shape[0] == rows * K), a.name
    readers, kinds = 0, set()
    for d, name in zip(eng.bwd.descs, eng.bwd.names):
        field = REP_FIELD.get(type(d), 'act_rep')
        if isinstance(d, L.BlurDesc):                       # the adjoint blur runs on the K gradients of every image, reads no activation
            assert _rows(d) == images * K, name
            continue
        assert _rows(d) == rows * K, (name, _rows(d))
        if isinstance(d, L.ImageIoDesc):
            assert d.cot_rep == K and d.backward == 1, name
            continue
        read = [f for f, p in _pointers(d).items() if p in fwd and p not in grads]
        if not read:
            assert getattr(d, field) in (0, 1), name
            continue
        readers += 1
        kinds.add(type(d))
        assert getattr(d, field) == K, f'{name} reads {[fwd[getattr(d, f)] for f in read]} of the forward pass without {field} = {K}'
    want = {L.ConvDesc, L.Interleave2Desc, L.Maxpool3s2Desc, L.AvgpoolActDesc} | ({L.GconvDesc} if net == 'resnext' else set())
    assert kinds == want and readers >= 14
    by_name = dict(zip(eng.bwd.names, eng.bwd.descs))
    assert by_name['resnet.maxpool^T'].act_rep == K and by_name['resnet.avgpool^T'].act_rep == K
    if net == 'resnext':                                    # the stride-1 grouped transpose carries relu'(t1) itself
        g = by_name['resnet.layer1.0.conv2^T']
        assert isinstance(g, L.GconvDesc) and g.dact_x and g.dact_rep == K and g.N == rows * K
    # the sub-pixel planes of the stride-2 transposes have one row per cotangent, their assembly maps act' to row n / K
    il = [d for d in eng.bwd.descs if isinstance(d, L.Interleave2Desc)]
    assert len(il) == 6 and all(d.N == rows * K and (d.dact_rep == K if d.dact_x else True) for d in il)
    pre = [d for d in eng.bwd.descs if isinstance(d, L.ConvDesc) and d.flags & L.GA_CONV_ADDEND_PRE_DACT]
    assert len(pre) == (1 if net == 'resnet_id' else 0) and all(d.dact_rep == K for d in pre)
    # no forward op carries a replica count
    for d, name in zip(eng.fwd.descs, eng.fwd.names):
        assert _rows(d) in (rows, images) and getattr(d, REP_FIELD.get(type(d), 'act_rep'), 0) in (0, 1), name


@pytest.mark.parametrize('front', list(FRONTS))
@pytest.mark.parametrize('net', list(NETS))
def test_one_cotangent_per_row_is_the_plan_of_an_engine_built_without_the_argument(net, front):
    one, plain = _engine(net, front, cot_rep=1), _engine(net, front)
    for a, b in ((one.fwd, plain.fwd), (one.bwd, plain.bwd)):
        assert a.names == b.names
        for da, db, name in zip(a.descs, b.descs, a.names):
            assert type(da) is type(db), name
            for f, typ in da._fields_:                      # every scalar field; the pointers are those of another allocation
                va, vb = getattr(da, f), getattr(db, f)
                if hasattr(va, '__len__'):                  # ga_interleave2_desc.s: four plane pointers, some NULL
                    assert [bool(v) for v in va] == [bool(v) for v in vb], (name, f)
                elif typ is not L.fp:
                    assert va == vb, (name, f)
            assert set(_pointers(da)) == set(_pointers(db)), name
            assert getattr(da, REP_FIELD.get(type(da), 'act_rep'), 0) in (0, 1), name
    rows = FRONTS[front]['rows']
    assert all(_rows(d) in (rows, rows // FRONTS[front]['rep']) for d in one.bwd.descs)


def test_a_purifier_in_front_of_a_resnet_stays_refused():
    cfg = {'initial_channels': 8, 'num_pre-post_process_blocks': 2, 'num_pre-post_process_cells': 2, 'num_scales': 2,
           'num_groups_per_scale': 2, 'is_adaptive': False, 'min_groups_per_scale': 1, 'num_cells_per_group': 2,
           'num_latent_per_group': 4, 'num_logistic_mixtures': 10, 'num_nf_cells': None}
    rspec, rsd = build_resnet_spec(4, 8, (1, 1, 1, 1)), init_resnet_state_dict(4, 8, 3, (1, 1, 1, 1))
    with pytest.raises((ValueError, NotImplementedError)):
        Engine(init_nvae_state_dict(cfg, (3, 32, 32), 1), cfg, (3, 32, 32), rsd, rspec, rows=2, rep=1, alphas=[0.0] * 4,
               device='cpu', dry_run=True, cot_rep=K)
    with pytest.raises(ValueError):
        _engine('resnet', 'plain', cot_rep=0)


def test_descriptor_layouts_did_not_move():
    assert C.sizeof(L.Maxpool3s2Desc) == 56 and L.ABI_VERSION == 8 and L.lib.ga_abi_version() == 8
    assert C.sizeof(L.Op) == 288 == L.lib.ga_sizeof_op()
    assert L.Maxpool3s2Desc.backward.offset == 48 and L.Maxpool3s2Desc.act_rep.offset == 52
    assert [f[0] for f in L.AvgpoolActDesc._fields_][-1] == 'act_rep' and C.sizeof(L.AvgpoolActDesc) == 56
    assert L.AvgpoolActDesc.act_rep.offset == 52
    assert [f[0] for f in L.GconvDesc._fields_][-1] == 'dact_rep' and L.GconvDesc.dact_rep.offset == C.sizeof(L.GconvDesc) - 4


def test_the_library_refuses_a_ragged_or_forward_replica_count_without_a_gpu():
    """GA_E_BADARG (-1) comes from the argument checks, in front of any launch"""
    for cls, fn in ((L.Maxpool3s2Desc, L.lib.ga_maxpool3s2), (L.AvgpoolActDesc, L.lib.ga_avgpool_act)):
        d = cls()
        d.x = d.y = d.dy = d.dx = 16
        d.C, d.N, d.backward, d.act_rep = 8, 6, 0, 3
        if cls is L.Maxpool3s2Desc:
            d.H = d.W = 4
        else:
            d.P = 4
        assert fn(C.byref(d), None) == L.GA_E_BADARG            # act_rep on a forward launch
        d.N, d.backward = 5, 1
        assert fn(C.byref(d), None) == L.GA_E_BADARG            # 5 cotangent rows are no multiple of 3
    g = L.GconvDesc()
    g.x = g.w = g.y = g.dact_x = 16
    g.N, g.Hi, g.Wi, g.Ho, g.Wo, g.C, g.cg, g.KH, g.KW, g.stride, g.pad, g.dact_rep = 5, 4, 4, 4, 4, 8, 4, 3, 3, 1, 1, 3
    assert L.lib.ga_gconv(C.byref(g), None) == L.GA_E_BADARG
