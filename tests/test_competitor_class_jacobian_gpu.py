"""
GPU: the K-cotangent backward plan of the defenders the ids experiment can put in front of its VGG-11
besides the NVAE one — ND-VAE, A-VAE and the noise / blur ablations.
  * engine level: `Engine.bare(cot_rep=3)` + build_ndvae_defense / build_avae_defense on the reduced configurations of
    tests/test_competitors_gpu.py against three backward replays of the plain engine, with the bound of
    tests/test_api_gpu.py::test_k_cotangent_engine_equals_repeated_backward (1e-5 of max |g|; logits bitwise);
  * API level: `ClassJacobian` over `EoTWrapper(defender, 2)` takes the plan (ONE forward, ceil(columns / K) backward replays)
    and gives what one autograd backward per class gives, with the bounds of
    tests/test_api_gpu.py::test_class_jacobian_k_cotangent_plan_equals_one_backward_per_class (logits 1e-5, gradients 1e-4 of
    each column's max);
  * a ResNet classifier behind a competitor has no plan: `class_jacobian_rows` answers None and the builders raise.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from gen_adversarial_amd.attacks.l2_attacks import ClassJacobian   # noqa: E402
from gen_adversarial_amd.avae_spec import build_avae_spec, init_avae_state_dict   # noqa: E402
from gen_adversarial_amd.defenses.ablations.models import GaussianBlurDefenseModel, GaussianNoiseDefenseModel   # noqa: E402
from gen_adversarial_amd.defenses.competitors.a_vae import AVaeDefenseModel, load_AVAE   # noqa: E402
from gen_adversarial_amd.defenses.competitors.nd_vae import NDVaeDefenseModel, load_NDVAE   # noqa: E402
from gen_adversarial_amd.defenses.ours.models import CelebaGenderClassifier, CelebaIdentityClassifier   # noqa: E402
from gen_adversarial_amd.defenses.wrappers import EoTWrapper   # noqa: E402
from gen_adversarial_amd.engine import Engine, WeightStore   # noqa: E402
from gen_adversarial_amd.ndvae_spec import build_ndvae_spec, init_ndvae_h, init_ndvae_state_dict   # noqa: E402
from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict   # noqa: E402
from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict   # noqa: E402

DEV = 'cuda:0'
ROWS, REP, K = 4, 2, 3
ND_CFG = {'x_channels': 3, 'encoding_channels': 8, 'pre_proc_groups': 2, 'scales': 2, 'groups': 1, 'cells': 2, 'input_dim': 32}


# ------------------------------------------------------------------------------------------------------------ engine level
def _vgg():
    return build_vgg_spec(100, 16), init_vgg_state_dict(100, 16, 3)


def _ndvae_engines():
    spec, sd, h = build_ndvae_spec(ND_CFG), init_ndvae_state_dict(ND_CFG, 21), init_ndvae_h(ND_CFG, 22)
    cspec, csd = _vgg()
    store, std, D = WeightStore(DEV), 0.07, ND_CFG['input_dim']
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(ROWS // REP, 3, D, D, generator=gen).to(DEV)
    noise = torch.randn(ROWS, 3, D, D, generator=gen).to(DEV)
    eps = [torch.randn(ROWS, c, r, r, generator=gen).to(DEV) for c, r in spec.latent_shapes]
    engs = {}
    for k in (1, K):
        e = Engine.bare(ROWS, device=DEV, store=store, rep=REP, resolution=(3, D, D), alphas=[], noise_eps=std, cot_rep=k)
        e.build_ndvae_defense(sd, spec, h, csd, cspec)
        e.x_in.copy_(x)
        e.noise.copy_(noise)
        e.noise_coef.fill_(std)
        for dst, src in zip(e.eps, eps):
            dst.copy_(src)
        engs[k] = e
    return engs, D


def _avae_engines():
    spec, sd = build_avae_spec(64, 8), init_avae_state_dict(64, 51, 8)
    cspec, csd = _vgg()
    store, D = WeightStore(DEV), 64
    gen = torch.Generator().manual_seed(6)
    x = torch.rand(ROWS // REP, 3, D, D, generator=gen).to(DEV)
    eps = [torch.randn(ROWS, spec.c512, 4, 4, generator=gen).to(DEV)]
    eps += [torch.randn(ROWS, 1, b.res, b.res, generator=gen).to(DEV) for b in spec.blocks]
    engs = {}
    for k in (1, K):
        e = Engine.bare(ROWS, device=DEV, store=store, rep=REP, resolution=(3, D, D), alphas=[], cot_rep=k)
        e.build_avae_defense(sd, spec, 2, csd, cspec)
        e.x_in.copy_(x)
        for dst, src in zip(e.eps, eps):
            dst.copy_(src)
        engs[k] = e
    return engs, D


@pytest.mark.parametrize('which', ['ndvae', 'avae'])
def test_k_cotangent_competitor_engine_equals_repeated_backward(which):
    """dense random cotangents on the logits — and, where the engine takes one, on the purified image (ND-VAE's `dpurified`) —
    three per forward row in ONE replay against three replays of the plain engine"""
    engs, D = _ndvae_engines() if which == 'ndvae' else _avae_engines()
    for e in engs.values():
        e.forward()
    assert engs[K].cot_rep == K and engs[K].dlogits.shape[0] == ROWS * K
    assert torch.equal(engs[1].logits, engs[K].logits)
    gen = torch.Generator().manual_seed(23)
    cot = torch.randn(ROWS, K, 100, generator=gen).to(DEV)
    cot_img = torch.randn(ROWS, K, 3, D, D, generator=gen).to(DEV)
    from_image = which == 'ndvae'
    engs[K].dlogits.view(ROWS, K, 100).copy_(cot)
    engs[K].backward()
    got = engs[K].dx.view(ROWS // REP, K, 3, D, D).clone()
    if from_image:
        engs[K].dpurified.view(ROWS, K, 3, D, D).copy_(cot_img)
        engs[K].backward(from_logits=False, from_purified=True)
        got_img = engs[K].dx.view(ROWS // REP, K, 3, D, D).clone()
    for k in range(K):
        engs[1].dlogits.view(ROWS, 100).copy_(cot[:, k])
        engs[1].backward()
        ref = engs[1].dx.clone()
        e = (got[:, k] - ref).abs().max().item() / ref.abs().max().item()
        print(f'   {which} cotangent {k}: from logits {e:.2e} of max |g| {ref.abs().max().item():.2e}')
        assert ref.abs().max().item() > 0 and e < 1e-5
        if from_image:
            engs[1].dpurified.copy_(cot_img[:, k])
            engs[1].backward(from_logits=False, from_purified=True)
            ref_img = engs[1].dx.clone()
            e_img = (got_img[:, k] - ref_img).abs().max().item() / ref_img.abs().max().item()
            print(f'   {which} cotangent {k}: from the purified image {e_img:.2e} of max |g| {ref_img.abs().max().item():.2e}')
            assert ref_img.abs().max().item() > 0 and e_img < 1e-5
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- API level
B, EOT, RES = 2, 2, (3, 64, 64)
ND_API = dict(x_channels=3, encoding_channels=4, pre_proc_groups=2, scales=1, groups=2, cells=1)


@pytest.fixture(scope='module')
def classifier(tmp_path_factory):
    d = tmp_path_factory.mktemp('cls')
    torch.save({'state_dict': init_vgg_state_dict(100, 16, seed=6)}, d / 'vgg.pt')
    return CelebaIdentityClassifier(str(d / 'vgg.pt'), DEV)


def _defender(name, clf):
    """(defender, pinned latent draws or None, pinned input noise or None) for B images under EoT"""
    gen = torch.Generator().manual_seed(31)
    rows = B * EOT
    if name == 'ndvae':
        cfg = dict(ND_API, input_dim=64)
        nd = load_NDVAE(init_ndvae_state_dict(cfg, 31), image_size=64, **ND_API)
        eps = [torch.randn(rows, c, r, r, generator=gen).to(DEV) for c, r in build_ndvae_spec(cfg).latent_shapes]
        return NDVaeDefenseModel(clf, nd, 0.05), eps, torch.randn(rows, *RES, generator=gen).to(DEV)
    if name == 'avae':
        spec = build_avae_spec(64, 8)
        av = load_AVAE(init_avae_state_dict(64, 61, 8), 64, width_div=8)
        eps = [torch.randn(rows, spec.c512, 4, 4, generator=gen).to(DEV)]
        eps += [torch.randn(rows, 1, b.res, b.res, generator=gen).to(DEV) for b in spec.blocks]
        return AVaeDefenseModel(clf, av, 2), eps, None
    if name == 'noise':
        return GaussianNoiseDefenseModel(clf, 2.0), None, torch.randn(rows, *RES, generator=gen).to(DEV)
    return GaussianBlurDefenseModel(clf), None, None


@pytest.mark.parametrize('name', ['ndvae', 'avae', 'noise', 'blur'])
def test_class_jacobian_takes_the_k_cotangent_plan(name, classifier, monkeypatch):
    defender, eps, noise = _defender(name, classifier)
    assert defender.supports_class_jacobian
    model = EoTWrapper(defender, EOT)
    g = torch.Generator().manual_seed(17)
    x = torch.rand(B, *RES, generator=g).to(DEV)
    classes = torch.stack([torch.randperm(100, generator=g)[:5] for _ in range(B)]).to(DEV)
    calls = {'n': 0}
    real = Engine.backward

    def counting(self, *a, **k):
        calls['n'] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(Engine, 'backward', counting)
    defender.fixed_noise(eps, noise)
    try:
        for cols, n_cols in ((classes, 5), (None, 100)):
            calls['n'] = 0
            fast = ClassJacobian(model, x, cols)
            assert fast._fast is not None, 'the defender must offer its K-cotangent plan'
            Kc = fast._fast.eng.cot_rep
            assert Kc == min(n_cols, 512 // (B * EOT))
            g_fast = fast.grads()
            assert calls['n'] == math.ceil(n_cols / Kc), (calls['n'], n_cols, Kc)
            monkeypatch.setattr(type(defender), 'jacobian_cot_rows', 0)            # no K-cotangent plan: autograd per class
            calls['n'] = 0
            slow = ClassJacobian(model, x, cols)
            assert slow._fast is None
            g_slow = slow.grads()
            assert calls['n'] == n_cols
            monkeypatch.undo()
            monkeypatch.setattr(Engine, 'backward', counting)
            assert g_fast.shape == g_slow.shape == (B, n_cols, *RES)
            e_l = (fast.logits - slow.logits).abs().max().item()
            scale = g_slow.abs().amax(dim=(2, 3, 4), keepdim=True).clamp_min(1e-30)
            e_g = ((g_fast - g_slow).abs() / scale).max().item()
            print(f'   {name}: K-cotangent plan (K = {Kc}, {n_cols} columns): logits {e_l:.2e}, gradients {e_g:.2e} of each column\'s max')
            assert e_l < 1e-5 and e_g < 1e-4
    finally:
        defender.fixed_noise(None, None)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_no_plan_behind_a_resnet_classifier(tmp_path):
    torch.save({'state_dict': init_resnet_state_dict(2, 8, 3, (1, 1, 1, 1))}, tmp_path / 'resnet.pt')
    clf = CelebaGenderClassifier(str(tmp_path / 'resnet.pt'), DEV)
    x = torch.rand(1, *RES).to(DEV)
    av = AVaeDefenseModel(clf, load_AVAE(init_avae_state_dict(64, 61, 8), 64, width_div=8), 2)
    cfg = dict(ND_API, input_dim=64)
    nd = NDVaeDefenseModel(clf, load_NDVAE(init_ndvae_state_dict(cfg, 31), image_size=64, **ND_API), 0.05)
    for m in (av, nd, GaussianNoiseDefenseModel(clf, 2.0), GaussianBlurDefenseModel(clf)):
        assert not m.supports_class_jacobian
        assert m.class_jacobian_rows(x, EOT) is None
        assert EoTWrapper(m, EOT).class_jacobian(x) is None
    rspec, rsd = build_resnet_spec(4, 8, (1, 1, 1, 1)), init_resnet_state_dict(4, 8, 3, (1, 1, 1, 1))
    eng = Engine.bare(ROWS, device=DEV, rep=REP, resolution=(3, 64, 64), alphas=[], cot_rep=K)
    with pytest.raises(NotImplementedError):
        eng.build_avae_defense(init_avae_state_dict(64, 51, 8), build_avae_spec(64, 8), 2, rsd, rspec)
    eng = Engine.bare(ROWS, device=DEV, rep=REP, resolution=(3, 64, 64), alphas=[], noise_eps=0.05, cot_rep=K)
    with pytest.raises(NotImplementedError):
        eng.build_ndvae_defense(init_ndvae_state_dict(cfg, 31), build_ndvae_spec(cfg), init_ndvae_h(cfg, 22), rsd, rspec)
