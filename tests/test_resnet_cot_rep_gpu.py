"""
GPU: the K-cotangent backward plan of the bare ResNet-50 / ResNeXt-50 classifiers.

  Op level      ga_maxpool3s2 / ga_avgpool_act (act_rep) and ga_gconv (dact_rep, both kernels): ONE backward launch with K = 3
                cotangents over 2 forward rows against three one-cotangent launches on the cotangent slices (cotangent k of forward
                row r sits at row r * K + k), bitwise.  Forward rows differ and so do the cotangents of a row: a wrong row index
                cannot pass.  Outputs start as NaN with a sentinel row behind them (test_ops_edges_gpu.Out).
  Engine level  dx of one Engine(cot_rep = 3) replay against three backward replays of a cot_rep = 1 engine on the same forward,
                bitwise.  The convs of both engines are pinned to one (tile, splits) per layer: the tuned choice is keyed by the
                pixel count, which differs between 2 and 6 rows, and another tile sums in another order.
  API level     CelebaGenderClassifier / CarsTypeClassifier: class_jacobian is the plan, its gradients are those of the per-class
                autograd loop, and DeepFool through it returns what DeepFool through the loop returns (bitwise; the engines are
                built without the tune table, so the layers of the 1-row and the K-row backward share their tile).
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from opref_cases import g   # noqa: E402
from gen_adversarial_amd import _lib as L   # noqa: E402
from gen_adversarial_amd import engine as engine_mod   # noqa: E402
from gen_adversarial_amd.engine import Engine, WeightStore   # noqa: E402
from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict   # noqa: E402
from test_ops_edges_gpu import DEV, SENT, Out, dev, launch   # noqa: E402

K, NF = 3, 2            # cotangents per forward row, forward rows


def _slice(t, k):
    """cotangent k of every forward row: [NF * K, ...] -> [NF, ...]"""
    return t.view(NF, K, *t.shape[1:])[:, k].contiguous()


# ------------------------------------------------------------------------------------------------------------------ op level
def test_maxpool3s2_backward_act_rep_with_ties():
    """6 x 6 x 8, x in multiples of 0.25: about every window holds a tie, at the borders (windows cut by the padding) too; the first
    maximum in scan order takes the cotangent, as aten::max_pool2d_with_indices keeps it"""
    H = W = 6
    C_ = 8
    x = (g(NF, H, W, C_, seed=1) * 4).round() / 4
    assert len(x.unique()) < x.numel() // 8 and not torch.equal(x[0], x[1])      # few distinct values: ties in about every window
    dy = g(NF * K, H // 2, W // 2, C_, seed=2)
    io = dict(x=dev(x), H=H, W=W, C=C_, backward=1)
    dx = Out(NF * K, H, W, C_)
    launch(L.Maxpool3s2Desc, dy=dev(dy), dx=dx, N=NF * K, act_rep=K, **io)
    dx = dx.done()
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(xr, 3, 2, 1)
    for k in range(K):
        dx1 = Out(NF, H, W, C_)
        launch(L.Maxpool3s2Desc, dy=dev(_slice(dy, k)), dx=dx1, N=NF, act_rep=1, **io)
        assert torch.equal(_slice(dx, k), dx1.done()), f'cotangent {k} differs from the act_rep = 1 launch'
        (ref,) = torch.autograd.grad(y, [xr], _slice(dy, k).permute(0, 3, 1, 2), retain_graph=True)
        err = (_slice(dx, k) - ref.permute(0, 2, 3, 1)).abs().max().item()
        print(f'maxpool3s2 backward, cotangent {k}: max err against aten {err:.2e}')
        assert err <= 1e-6
    dx0 = Out(NF, H, W, C_)                                  # act_rep = 0 keeps its meaning
    launch(L.Maxpool3s2Desc, dy=dev(_slice(dy, 0)), dx=dx0, N=NF, act_rep=0, **io)
    assert torch.equal(dx0.done(), _slice(dx, 0))


def test_avgpool_act_backward_act_rep():
    """P = 5 pixels over the 16 pixel lanes, C = 68 = one full 64-channel chunk and one of 4; ReLU with some x exactly 0 (relu'(0) = 0)"""
    P, C_ = 5, 68
    x = g(NF, P, C_, seed=1)
    x[0, 1, :5] = 0.0
    x[1, 4, 64:] = 0.0
    x[1, 0, 7] = -0.0
    dy = g(NF * K, C_, seed=2)
    io = dict(x=dev(x), P=P, C=C_, act=L.GA_ACT_RELU, backward=1)
    dx = Out(NF * K, P, C_)
    launch(L.AvgpoolActDesc, dy=dev(dy), dx=dx, N=NF * K, act_rep=K, **io)
    dx = dx.done()
    for k in range(K):
        dx1 = Out(NF, P, C_)
        launch(L.AvgpoolActDesc, dy=dev(_slice(dy, k)), dx=dx1, N=NF, act_rep=1, **io)
        assert torch.equal(_slice(dx, k), dx1.done()), f'cotangent {k} differs from the act_rep = 1 launch'
        # dy / P is one rounding (x * (1 / P) in the kernel: two), relu' is exact
        ref = (_slice(dy, k).double() / P).view(NF, 1, C_) * (x > 0).double()
        assert (_slice(dx, k).double() - ref).abs().max().item() <= 2.0 ** -22 * ref.abs().max().item()
        assert bool((_slice(dx, k)[x <= 0] == 0).all())


@pytest.mark.parametrize('cg', [4, 12], ids=['lds_cg4', 'generic_cg12'])
def test_gconv_dact_rep(cg):
    """3 x 3 / stride 1 / pad 1 on 5 x 5 x 24 with the relu' epilogue: cg = 4 runs gconv_group_kernel<4> (weights in LDS), cg = 12
    the generic kernel"""
    H = W = 5
    C_ = 24
    x, w = g(NF * K, H, W, C_, seed=1), g(C_, 9 * cg, seed=2, scale=0.3)
    dact = g(NF, H, W, C_, seed=3)
    dact[0, 0, 0, :4] = 0.0
    assert not torch.equal(dact[0], dact[1])
    io = dict(w=dev(w), dact_x=dev(dact), Hi=H, Wi=W, Ho=H, Wo=W, C=C_, cg=cg, KH=3, KW=3, stride=1, pad=1, dact_act=L.GA_ACT_RELU)
    y = Out(NF * K, H, W, C_)
    launch(L.GconvDesc, x=dev(x), y=y, N=NF * K, dact_rep=K, **io)
    y = y.done()
    groups = C_ // cg
    wt = w.view(C_, 3, 3, cg).permute(0, 3, 1, 2).contiguous()
    for k in range(K):
        y1 = Out(NF, H, W, C_)
        launch(L.GconvDesc, x=dev(_slice(x, k)), y=y1, N=NF, dact_rep=1, **io)
        assert torch.equal(_slice(y, k), y1.done()), f'cotangent {k} differs from the dact_rep = 1 launch'
        ref = torch.nn.functional.conv2d(_slice(x, k).permute(0, 3, 1, 2).double(), wt.double(), padding=1, groups=groups)
        ref = ref.permute(0, 2, 3, 1) * (dact > 0).double()
        # 9 * cg fp32 products summed in fp32 against float64: n * 2^-24 of the sum of magnitudes bounds it
        mag = torch.nn.functional.conv2d(_slice(x, k).permute(0, 3, 1, 2).abs().double(), wt.abs().double(), padding=1, groups=groups)
        assert (_slice(y, k).double() - ref).abs().max().item() <= (9 * cg + 1) * 2.0 ** -24 * mag.max().item()
        assert bool((_slice(y, k)[dact <= 0] == 0).all())


@pytest.mark.parametrize('op,what', [('maxpool3s2', 'ragged'), ('avgpool_act', 'ragged'), ('gconv', 'ragged'),
                                     ('maxpool3s2', 'forward'), ('avgpool_act', 'forward')])
def test_replica_count_refusals(op, what):
    """N = 5 with a replica count of 3 (all three ops), and act_rep = 3 on a forward launch (the two pools; ga_gconv has no
    backward flag): GA_E_BADARG, nothing launched (the outputs still hold their sentinel)"""
    n = 5 if what == 'ragged' else 6
    a, b = dev(g(n, 4, 4, 8, seed=1)), dev(g(n, 4, 4, 8, seed=2))
    w = dev(g(8, 9 * 4, seed=3))
    out = torch.full((n, 4, 4, 8), SENT, device=DEV)
    if op == 'gconv':
        d, fn = L.GconvDesc(), L.lib.ga_gconv
        d.x, d.w, d.dact_x, d.y = a.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr()
        d.N, d.Hi, d.Wi, d.Ho, d.Wo, d.C, d.cg, d.KH, d.KW, d.stride, d.pad, d.dact_act, d.dact_rep = n, 4, 4, 4, 4, 8, 4, 3, 3, 1, 1, 1, 3
    else:
        cls, fn = ((L.Maxpool3s2Desc, L.lib.ga_maxpool3s2) if op == 'maxpool3s2' else (L.AvgpoolActDesc, L.lib.ga_avgpool_act))
        d = cls()
        d.x, d.dy, d.y, d.dx = a.data_ptr(), b.data_ptr(), out.data_ptr(), out.data_ptr()
        d.N, d.C, d.act_rep, d.backward = n, 8, 3, int(what == 'ragged')
        if op == 'maxpool3s2':
            d.H = d.W = 4
        else:
            d.P, d.act = 16, L.GA_ACT_RELU
    assert fn(C.byref(d), 0) == L.GA_E_BADARG
    with pytest.raises(L.GaError, match='GA_E_BADARG'):
        L.run(d)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# -------------------------------------------------------------------------------------------------------------- engine level
RES = (3, 64, 64)
NETS = {'resnet': (4, 8, (2, 1, 1, 1)),             # a second block in layer 1: the identity shortcut (GA_CONV_ADDEND_PRE_DACT)
        'resnext': (4, 2, (2, 1, 1, 1), 4, 8)}      # grouped 3x3 convs, 4 .. 32 channels per group: gconv_group_kernel<4 .. 32>


def _pin_convs(eng):
    """one (tile, splits) per conv layer whatever the row count: the library's choice for a small launch (tile 4 up to 32 output
    channels, else tile 3; ga_conv2d's own rule below 512 workgroups), no split-K"""
    for d in eng._conv_descs():
        d.tile, d.splits, d.ws, d.ws_floats = (4 if d.Cout <= 32 else 3), 1, None, 0
    eng.fwd.finalize()
    eng.bwd.finalize()


@pytest.mark.parametrize('front', ['plain', 'blur_noise_rep2'])
@pytest.mark.parametrize('net', list(NETS))
def test_k_cotangent_engine_equals_repeated_backward(net, front, monkeypatch):
    monkeypatch.setattr(engine_mod, 'tune_cache', lambda: {})      # no per-shape table: split-bf16 everywhere, in both engines
    a = NETS[net]
    rspec, rsd = build_resnet_spec(*a), init_resnet_state_dict(a[0], a[1], 7, *a[2:])
    rep, kw = (1, {}) if front == 'plain' else (2, dict(blur=True, noise_eps=2.0))
    rows = NF                                                   # 2 forward rows: two images, or one image x 2 replicas
    store = WeightStore(DEV)
    gen = torch.Generator().manual_seed(23)
    imgs = torch.rand(rows // rep, *RES, generator=gen).to(DEV)
    noise = torch.randn(rows, *RES, generator=gen).to(DEV)
    cot = torch.randn(rows, K, 4, generator=gen).to(DEV)        # dense cotangents, K = 3 of the 4 classes' worth of rows
    engs = {k: Engine(None, None, RES, rsd, rspec, rows=rows, rep=rep, alphas=[], device=DEV, store=store, cot_rep=k, **kw)
            for k in (1, K)}
    for e in engs.values():
        _pin_convs(e)
        e.x_in.copy_(imgs)
        if e.noise is not None:
            e.noise.copy_(noise)
            e.noise_coef.copy_(e.noise_eps / noise.flatten(1).norm(dim=1))
        e.forward()
    assert torch.equal(engs[1].logits, engs[K].logits)
    assert engs[K].bwd.names == engs[1].bwd.names
    engs[K].dlogits.view(rows, K, 4).copy_(cot)
    engs[K].backward()
    got = engs[K].dx.view(rows // rep, K, *RES).clone()
    assert torch.isfinite(got).all() and got.abs().max().item() > 0
    for k in range(K):
        engs[1].dlogits.view(rows, 4).copy_(cot[:, k])
        engs[1].backward()
        ref = engs[1].dx
        assert ref.abs().max().item() > 0
        assert torch.equal(got[:, k], ref), \
            f'cotangent {k}: {int((got[:, k] != ref).sum())} elements differ, max {(got[:, k] - ref).abs().max().item():.3e}'
    assert not torch.equal(got[:, 0], got[:, 1])


# ----------------------------------------------------------------------------------------------------------------- API level
def _classifier(kind, tmp_path):
    from gen_adversarial_amd.defenses.ours.models import CarsTypeClassifier, CelebaGenderClassifier
    if kind == 'gender':
        sd, cls = init_resnet_state_dict(2, 8, 5, (1, 1, 1, 1)), CelebaGenderClassifier
    else:
        sd, cls = init_resnet_state_dict(4, 2, 5, (1, 1, 1, 1), 4, 16), CarsTypeClassifier
    torch.save({'state_dict': sd}, tmp_path / f'{kind}.pt')
    return cls(str(tmp_path / f'{kind}.pt'), DEV)


@pytest.mark.parametrize('kind,n_classes', [('gender', 2), ('cars', 4)])
def test_classifier_class_jacobian_and_deepfool_take_the_plan(kind, n_classes, tmp_path, monkeypatch):
    from gen_adversarial_amd.attacks.l2_attacks import ClassJacobian, DeepFool
    monkeypatch.setattr(engine_mod, 'tune_cache', lambda: {})          # every engine below: the library's tile per layer
    clf = _classifier(kind, tmp_path)
    assert clf.supports_class_jacobian and (clf.classifier.groups > 1) == (kind == 'cars')
    x = torch.rand(1, *RES, generator=torch.Generator().manual_seed(17)).to(DEV)
    calls = {'n': 0}
    real = Engine.backward

    def counting(self, *a, **k):
        calls['n'] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(Engine, 'backward', counting)

    assert clf.class_jacobian(x) is not None
    fast = ClassJacobian(clf, x)
    assert fast._fast is not None, 'the ResNet classifier must offer its K-cotangent plan'
    assert fast._fast.eng.cot_rep == n_classes                         # jacobian_cot_rows // 1 row, clamped to the class count
    g_fast = fast.grads()
    assert calls['n'] == 1                                             # all classes in ONE backward replay
    run = lambda: DeepFool(num_classes=n_classes, overshoot=0.02, max_iter=3)(x.clone(), fast.logits.argmax(dim=1), clf)   # noqa: E731
    calls['n'] = 0
    s_fast, l2_fast, adv_fast = run()
    n_fast = calls['n']
    assert 1 <= n_fast <= 3                                            # one replay per DeepFool iteration
    monkeypatch.setattr(type(clf), 'jacobian_cot_rows', 0)             # no K-cotangent plan: autograd per class
    calls['n'] = 0
    slow = ClassJacobian(clf, x)
    assert slow._fast is None
    g_slow = slow.grads()
    assert calls['n'] == n_classes
    calls['n'] = 0
    s_slow, l2_slow, adv_slow = run()
    assert calls['n'] == n_fast * n_classes                            # the same iterations, one backward per class each
    assert g_fast.shape == g_slow.shape == (1, n_classes, *RES) and g_slow.abs().amax(dim=(2, 3, 4)).min().item() > 0
    assert torch.equal(fast.logits, slow.logits)
    assert torch.equal(g_fast, g_slow), f'max difference {(g_fast - g_slow).abs().max().item():.3e}'
    assert s_fast == s_slow and l2_fast == l2_slow and (math.isinf(l2_fast) or l2_fast > 0)
    assert torch.equal(adv_fast, adv_slow)
