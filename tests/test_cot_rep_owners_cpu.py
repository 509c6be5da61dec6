"""
CPU: the host side of the K-cotangent backward plan of the ND-VAE, A-VAE and noise / blur defenders — `Engine.bare(cot_rep=K)`,
the dry-run plans of build_ndvae_defense / build_avae_defense with K = 3 (every backward descriptor counts rows x K cotangent
rows, and every one that reads a tensor of the forward pass says so in its replica field: `dact_rep` of ga_conv_desc /
ga_interleave2_desc, `cot_rep` of ga_image_io_desc, `act_rep` of the others), and `supports_class_jacobian` of the three
owners.  No kernel is launched.
"""
import ctypes as C
import inspect
from types import SimpleNamespace

import pytest
import torch

from gen_adversarial_amd import _lib as L
from gen_adversarial_amd.avae_spec import build_avae_spec, init_avae_state_dict
from gen_adversarial_amd.defenses.ablations.models import GaussianBlurDefenseModel, GaussianNoiseDefenseModel
from gen_adversarial_amd.defenses.competitors.a_vae import AVaeDefenseModel
from gen_adversarial_amd.defenses.competitors.nd_vae import NDVaeDefenseModel
from gen_adversarial_amd.engine import Engine
from gen_adversarial_amd.ndvae_spec import build_ndvae_spec, init_ndvae_h, init_ndvae_state_dict
from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict

ROWS, REP, K = 4, 2, 3
ND_CFG = {'x_channels': 3, 'encoding_channels': 8, 'pre_proc_groups': 2, 'scales': 2, 'groups': 1, 'cells': 2, 'input_dim': 32}
REP_FIELD = {L.ConvDesc: 'dact_rep', L.Interleave2Desc: 'dact_rep', L.ImageIoDesc: 'cot_rep'}       # every other one: act_rep


def _ndvae(cot_rep, cspec=None, csd=None):
    spec, sd, h = build_ndvae_spec(ND_CFG), init_ndvae_state_dict(ND_CFG, 21), init_ndvae_h(ND_CFG, 22)
    if cspec is None:
        cspec, csd = build_vgg_spec(100, 16), init_vgg_state_dict(100, 16, 3)
    eng = Engine.bare(ROWS, device='cpu', dry_run=True, rep=REP, resolution=(3, 32, 32), alphas=[], noise_eps=0.07, cot_rep=cot_rep)
    return eng.build_ndvae_defense(sd, spec, h, csd, cspec)


def _avae(cot_rep, cspec=None, csd=None):
    spec, sd = build_avae_spec(64, 8), init_avae_state_dict(64, 51, 8)
    if cspec is None:
        cspec, csd = build_vgg_spec(100, 16), init_vgg_state_dict(100, 16, 3)
    eng = Engine.bare(ROWS, device='cpu', dry_run=True, rep=REP, resolution=(3, 64, 64), alphas=[], cot_rep=cot_rep)
    return eng.build_avae_defense(sd, spec, 2, csd, cspec)


def _pointers(d):
    return {name: getattr(d, name) for name, typ in d._fields_ if typ is L.fp and getattr(d, name)}


def _rows(d):
    """the row count of a backward descriptor, in cotangent rows"""
    if isinstance(d, L.AxpbyDesc):
        return None                                          # a flat element count: checked against its tensors below
    if isinstance(d, L.BlurDesc):
        return d.planes // 3
    return d.N


@pytest.mark.parametrize('build', [_ndvae, _avae], ids=['ndvae', 'avae'])
def test_backward_plans_carry_the_cotangent_count(build):
    eng = build(K)
    assert eng.cot_rep == K
    # the tensors of the forward pass, by base address: activations, latent draws / noise images, the input and its noise
    fwd = {a.t.data_ptr(): name for name, a in eng.acts.items()}
    fwd.update({e.data_ptr(): f'eps[{i}]' for i, e in enumerate(eng.eps)})
    if eng.noise is not None:
        fwd[eng.noise.data_ptr()] = 'noise'
    grads = {a._g.data_ptr() for a in eng.acts.values() if a._g is not None}
    for a in eng.acts.values():
        assert a._g is None or a._g.shape[0] == a.n * K, a.name
    assert eng.dlogits.shape[0] == ROWS * K and eng.dx.shape[0] == ROWS // REP * K
    readers = 0
    for d, name in zip(eng.bwd.descs, eng.bwd.names):
        n = _rows(d)
        if isinstance(d, L.ImageIoDesc):
            assert n == ROWS * K and d.cot_rep == K, name
            continue
        assert n is None or n == ROWS * K, (name, n)
        read = [f for f, p in _pointers(d).items() if p in fwd and p not in grads]
        if not read:
            continue
        readers += 1
        field = REP_FIELD.get(type(d), 'act_rep')
        assert getattr(d, field) == K, f'{name} reads {[fwd[getattr(d, f)] for f in read]} of the forward pass without {field} = {K}'
    assert readers > 20
    # ... and with one cotangent per row nothing changes: no replica field is set, N counts forward rows
    one = build(1)
    for d, name in zip(one.bwd.descs, one.bwd.names):
        assert getattr(d, REP_FIELD.get(type(d), 'act_rep'), 0) in (0, 1), name
        n = _rows(d)
        assert n is None or n == ROWS, (name, n)
    assert one.bwd.names == eng.bwd.names


def test_avae_backward_ops_read_the_forward_at_row_n_over_k():
    eng = _avae(K)
    ops = [(d, n) for d, n in zip(eng.bwd.descs, eng.bwd.names) if isinstance(d, L.AvaeDesc)]
    modes = {L.GA_AVAE_ADAIN: 0, L.GA_AVAE_AVGPOOL: 0, L.GA_AVAE_PIXELNORM: 0, L.GA_AVAE_SAMPLE: 0}
    for d, name in ops:
        assert (d.backward, d.N, d.act_rep) == (1, ROWS * K, K), name
        modes[d.mode] += 1
    assert modes == {L.GA_AVAE_ADAIN: 2 * len(build_avae_spec(64, 8).blocks), L.GA_AVAE_AVGPOOL: 1, L.GA_AVAE_PIXELNORM: 1,
                     L.GA_AVAE_SAMPLE: 1}
    for d in eng.fwd.descs:
        if isinstance(d, L.AvaeDesc):
            assert (d.backward, d.N, d.act_rep) == (0, ROWS, 0)
    # the draws and the AdaIN statistics stay at one row per forward row
    assert all(e.shape[0] == ROWS for e in eng.eps)
    # the act' sources of the PReLU epilogues are forward tensors: the convs and the stride-2 assemblies name the replica count
    prelu = [d for d in eng.bwd.descs if isinstance(d, L.ConvDesc) and d.flags & L.GA_CONV_DACT_PRELU]
    assert len(prelu) >= 3 and all(d.dact_rep == K and d.N == ROWS * K for d in prelu)
    il = [d for d in eng.bwd.descs if isinstance(d, L.Interleave2Desc)]
    assert len(il) == 3 and all(d.dact_prelu == 1 and d.dact_rep == K and d.N == ROWS * K for d in il)


def test_the_library_refuses_a_ragged_or_forward_act_rep_without_a_gpu():
    d = L.AvaeDesc()
    d.x = d.y = d.dy = 16
    d.mode, d.C, d.N, d.backward, d.act_rep = L.GA_AVAE_PIXELNORM, 8, 4, 0, 2
    assert L.lib.ga_avae(C.byref(d), None) == -1             # GA_E_BADARG: act_rep on a forward launch
    d.N, d.backward = 5, 1
    assert L.lib.ga_avae(C.byref(d), None) == -1             # 5 cotangent rows are no multiple of 2
    assert [f[0] for f in L.AvaeDesc._fields_][-1] == 'act_rep' and L.ABI_VERSION == L.lib.ga_abi_version()


def test_bare_engine_checks_cot_rep():
    for bad in (0, -2):
        with pytest.raises(ValueError):
            Engine.bare(ROWS, device='cpu', dry_run=True, rep=REP, resolution=(3, 32, 32), alphas=[], cot_rep=bad)
    assert Engine.bare(ROWS, device='cpu', dry_run=True).cot_rep == 1


def test_competitors_refuse_a_resnet_classifier_with_k_cotangents():
    rspec, rsd = build_resnet_spec(4, 8, (1, 1, 1, 1)), init_resnet_state_dict(4, 8, 3, (1, 1, 1, 1))
    for build in (_avae, _ndvae):
        with pytest.raises(NotImplementedError):
            build(K, rspec, rsd)


@pytest.mark.parametrize('owner', [NDVaeDefenseModel, AVaeDefenseModel, GaussianNoiseDefenseModel, GaussianBlurDefenseModel])
def test_supports_class_jacobian_follows_the_classifier_spec(owner):
    """owners need a GPU to be constructed; the property only looks at the base classifier's spec"""
    assert 'cot_rep' in inspect.signature(owner._make_engine).parameters
    for spec, want in ((build_vgg_spec(100, 16), True), (build_resnet_spec(4, 8, (1, 1, 1, 1)), False)):
        m = owner.__new__(owner)
        torch.nn.Module.__init__(m)
        m.base_classifier = SimpleNamespace(classifier=SimpleNamespace(spec=spec))
        assert m.supports_class_jacobian is want
        if not want:                                         # no plan: callers fall back to one autograd backward per class
            assert m.class_jacobian_rows(torch.zeros(1, 3, 64, 64), 2) is None
