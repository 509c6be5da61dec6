"""
GPU tests at the FULL size of BASELINE.json configs[1]: the assumed NVAE configuration (C=32, 3 scales x 8 groups,
20 latents, 64x64), the full-width VGG-11 (25088-wide projector head), EoT 32, alphas of
configs/ours_cosine_no_preprocessing_ids.yaml x 0.7 — the engine bench.py measures.

  * direct parity with the CPU oracle on 4 rows (2 images x EoT 2): the oracle needs ~1 s per row at this size;
  * size-independent properties on 64 rows (2 images x EoT 32): linearity of the backward pass in its cotangent,
    replica invariance (equal latent noise => bitwise equal rows), exactness of the shared-encoder de-duplication,
    row independence (a 64-row plan equals two 32-row plans), and a directional-derivative check of the NVAE gradient.
Tolerance 1e-3 absolute as BASELINE.json's north_star states; observed ~2e-5.
"""
import gc
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from gen_adversarial_amd.engine import Engine, WeightStore   # noqa: E402
from gen_adversarial_amd.nvae_spec import (ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION, build_spec,   # noqa: E402
                                           init_nvae_state_dict)
from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict   # noqa: E402

DEV = 'cuda:0'
TOL = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def model():
    with open(os.path.join(ROOT, 'configs', 'ours_cosine_no_preprocessing_ids.yaml')) as f:
        y = yaml.safe_load(f)
    alphas = [a * y['alpha_attenuation'] for a in y['interpolation_alphas']]
    sd = init_nvae_state_dict(ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION, 0)
    vspec = build_vgg_spec(100, 1)
    vsd = init_vgg_state_dict(100, 1, 1)
    return {'sd': sd, 'vsd': vsd, 'vspec': vspec, 'alphas': alphas, 'store': WeightStore(DEV),
            'spec': build_spec(ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION)}


def engine(m, rows, rep, **kw):
    # an engine and its Act buffers reference each other: `del eng` frees its device memory only at the next cyclic collection,
    # and two 1024-row plans do not fit beside each other
    gc.collect()
    torch.cuda.empty_cache()
    return Engine(m['sd'], ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION, m['vsd'], m['vspec'], rows=rows, rep=rep,
                  alphas=m['alphas'], temperature=0.6, noise_eps=0.0, device=DEV, store=m['store'], **kw)


def fill(eng, imgs, eps):
    eng.x_in.copy_(imgs.to(DEV))
    for b, e in zip(eng.eps, eps):
        b.copy_(e.to(DEV))


def err(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


def test_fullsize_parity_with_the_oracle(model):
    from oracle import defender_oracle as D
    from oracle import nvae_oracle as O
    m, spec = model, model['spec']
    rows, rep = 4, 2
    gen = torch.Generator().manual_seed(11)
    imgs = torch.rand(rows // rep, 3, 64, 64, generator=gen)
    eps = [torch.randn(rows, spec.num_latent, gs.res, gs.res, generator=gen) for gs in spec.groups]
    xr = imgs.clone().requires_grad_(True)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    purified = O.nvae_purify(m['sd'], spec, xr.repeat_interleave(rep, dim=0), m['alphas'], eps, 0.6)
    cot_img = torch.randn(purified.shape, generator=gen)
    (gx_img,) = torch.autograd.grad((purified * cot_img).sum(), [xr], retain_graph=True)
    logits = D.classifier_call(m['vsd'], m['vspec'], purified)
    cot = torch.randn(logits.shape, generator=gen)
    (gx,) = torch.autograd.grad((logits * cot).sum(), [xr])

    eng = engine(m, rows, rep)
    fill(eng, imgs, eps)
    eng.forward()
    e_p, e_l = err(eng.purified, purified), err(eng.logits, logits)
    eng.dpurified.copy_(cot_img.to(DEV))
    eng.backward(from_logits=False, from_purified=True)
    e_gi, gi_max = err(eng.dx, gx_img), gx_img.abs().max().item()
    eng.dlogits.view_as(eng.logits).copy_(cot.to(DEV))
    eng.backward()
    diff = (eng.dx.cpu() - gx).double()
    rel_l2 = (diff.norm() / gx.double().norm()).item()
    print(f'full-size oracle parity: purified {e_p:.2e} logits {e_l:.2e} (|logits| {logits.abs().max().item():.2f}) '
          f'nvae-grad {e_gi:.2e} (max {gi_max:.2e}) full-grad relL2 {rel_l2:.2e}')
    assert e_p < TOL and e_l < TOL
    assert e_gi < TOL * max(1.0, gi_max)
    from gradcheck import assert_grad_given_engine_decisions
    assert_grad_given_engine_decisions(
        eng, lambda t: (D.classifier_call(m['vsd'], m['vspec'], O.nvae_purify(m['sd'], spec, t.repeat_interleave(rep, dim=0),
                                                                              m['alphas'], eps, 0.6)) * cot).sum(),
        imgs, eng.dx, 1e-3, 'full-size input gradient through NVAE + VGG', min_matched=8)
    assert rel_l2 < 2e-2                      # secondary (tie-dependent elements included)


def test_fullsize_properties(model):
    m, spec = model, model['spec']
    rows, rep = 64, 32
    gen = torch.Generator().manual_seed(12)
    imgs = torch.rand(rows // rep, 3, 64, 64, generator=gen)
    eps = [torch.randn(rows, spec.num_latent, gs.res, gs.res, generator=gen) for gs in spec.groups]
    eng = engine(m, rows, rep)
    fill(eng, imgs, eps)
    eng.forward()
    logits = eng.logits.clone()
    purified = eng.purified.clone()
    assert torch.isfinite(logits).all() and 0.0 <= purified.min().item() and purified.max().item() <= 1.0

    # ---- the backward pass is linear in its cotangent
    a = torch.randn(logits.shape, generator=gen).to(DEV)
    b = torch.randn(logits.shape, generator=gen).to(DEV)
    grads = []
    for c in (a, b, a + b):
        eng.dlogits.view_as(eng.logits).copy_(c)
        eng.backward()
        grads.append(eng.dx.clone())
    lin = err(grads[2], grads[0] + grads[1])
    scale = grads[2].abs().max().item()
    print(f'backward linearity: {lin:.2e} of {scale:.2e}')
    assert lin < 1e-4 * max(1.0, scale)
    # gradient through the purifier alone (cotangent on the purified image): smooth, compared strictly below; the
    # classifier's max-pools make the full gradient discontinuous at near-ties, so that one is compared in relative L2
    u64 = torch.randn(purified.shape, generator=gen).to(DEV)
    eng.dpurified.copy_(u64)
    eng.backward(from_logits=False, from_purified=True)
    g_nvae = eng.dx.clone()
    s_nvae = g_nvae.abs().max().item()

    # ---- row independence: the same rows through two 32-row plans
    half = engine(m, 32, 32)
    for i in range(2):
        fill(half, imgs[i:i + 1], [e[32 * i:32 * (i + 1)] for e in eps])
        half.forward()
        assert err(half.logits, logits[32 * i:32 * (i + 1)]) < 1e-4
        half.dlogits.view_as(half.logits).copy_(a[32 * i:32 * (i + 1)])
        half.backward()
        assert rel_l2(half.dx, grads[0][i:i + 1]) < 2e-2
        half.dpurified.copy_(u64[32 * i:32 * (i + 1)])
        half.backward(from_logits=False, from_purified=True)
        assert err(half.dx, g_nvae[i:i + 1]) < 1e-4 * max(1.0, s_nvae)

    # ---- EoT replicas with equal latent noise are the same computation: bitwise equal rows
    same = [e[::rep].repeat_interleave(rep, dim=0) for e in eps]
    fill(eng, imgs, same)
    eng.forward()
    lg = eng.logits.view(rows // rep, rep, -1)
    assert torch.equal(lg, lg[:, :1].expand_as(lg))

    # ---- the shared encoder (one encoder pass per image) is exact when no input noise is configured
    shared = engine(m, rows, rep, share_encoder=True)
    assert shared.share_encoder and shared.enc_rows == rows // rep
    fill(shared, imgs, eps)
    shared.forward()
    assert err(shared.logits, logits) < 1e-4 and err(shared.purified, purified) < 1e-5
    shared.dlogits.view_as(shared.logits).copy_(a)
    shared.backward()
    assert rel_l2(shared.dx, grads[0]) < 2e-2
    shared.dpurified.copy_(u64)
    shared.backward(from_logits=False, from_purified=True)
    assert err(shared.dx, g_nvae) < 1e-4 * max(1.0, s_nvae)

    # ---- directional derivative of the purifier (smooth leg, exact-fp32 kernels) against central differences, with the
    # cotangent aligned to the response so that the inner product is well conditioned: <D, J v> = |D|^2 for D = J v
    fp = engine(m, 2, 1, precision='fp32')
    x0 = imgs.clamp(0.05, 0.95)
    e1 = [e[::rep].contiguous() for e in eps]
    v = torch.randn(x0.shape, generator=gen)
    v = v / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    h = 2e-2
    outs = []
    for sgn in (+1.0, -1.0):
        fill(fp, x0 + sgn * h * v, e1)
        fp.forward()
        outs.append(fp.purified.clone())
    D = (outs[0] - outs[1]) / (2 * h)
    numeric = (D * D).flatten(1).sum(dim=1).cpu()
    fill(fp, x0, e1)
    fp.forward()
    fp.dpurified.copy_(D)
    fp.backward(from_logits=False, from_purified=True)
    analytic = (fp.dx.cpu() * v).flatten(1).sum(dim=1)
    rel = ((analytic - numeric).abs() / numeric.abs()).max().item()
    print(f'directional derivative: analytic {analytic.tolist()} numeric {numeric.tolist()} rel {rel:.2e}')
    assert rel < 3e-2


def test_fused_decoder_cells_equal_the_unfused_launches_bitwise(model, monkeypatch):
    """The 32 decoder cells at 16 x 16 x 128 and 8 x 8 x 256 as ga_dec_cell launches (forced: an 8-row plan is far below the
    workgroup count from which the engine picks them) against the same plan built from the three launches per direction the
    fused kernel replaces: same operand split, k order and depthwise loop order => bitwise equal image, logits and input gradient."""
    from gen_adversarial_amd import _lib as L
    # the comparison is between KERNELS, not between tuning choices: with an empty tune table every conv of both plans runs the
    # library's default split-bf16 tile without split-K, so the unfused 1x1 convs sum in the fused kernel's k order whatever
    # conv_tune_gfx950.json holds (a table entry with split-K for one of these shapes broke the equality)
    monkeypatch.setattr('gen_adversarial_amd.engine.tune_cache', lambda: {})
    m, spec = model, model['spec']
    rows, rep = 8, 2
    gen = torch.Generator().manual_seed(21)
    imgs = torch.rand(rows // rep, 3, 64, 64, generator=gen)
    eps = [torch.randn(rows, spec.num_latent, gs.res, gs.res, generator=gen) for gs in spec.groups]
    dlog = torch.randn(rows, 100, generator=gen)
    out = []
    for fuse, min_wgs in ((False, 160), (True, 0), (True, 160)):
        monkeypatch.setattr(Engine, 'fuse_dec_cells', fuse)
        monkeypatch.setattr(Engine, 'fuse_min_workgroups', min_wgs)
        eng = engine(m, rows, rep)
        n_fused = sum(isinstance(d, L.DecCellDesc) for d in eng.fwd.descs), sum(isinstance(d, L.DecCellDesc) for d in eng.bwd.descs)
        assert n_fused == ((32, 32) if fuse and min_wgs == 0 else (0, 0)), n_fused      # 8 rows: fused only when forced
        eng.x_in.copy_(imgs.to(DEV))
        for dst, src in zip(eng.eps, eps):
            dst.copy_(src.to(DEV))
        eng.forward()
        eng.dlogits.view(rows, -1).copy_(dlog.to(DEV))
        eng.backward()
        torch.cuda.synchronize()
        out.append((eng.purified.clone(), eng.logits.clone(), eng.dx.clone(), eng.bytes))
        del eng
    (p0, l0, g0, b0), (p1, l1, g1, b1), _ = out
    assert torch.equal(p0, p1) and torch.equal(l0, l1) and torch.equal(g0, g1)
    assert b1 < 0.75 * b0          # the two 6C-wide tensors of those cells are no longer stored


def test_halo_fused_post_processing_cells_equal_the_unfused_launches(model, monkeypatch):
    """ga_dec_cell_halo (off by default: its backward is slower than the launches it replaces) selected for the two
    few-channel post-processing cells of a 32-row plan, against the default plan: the unfused 1x1 convs of these cells run on other
    kernels (tile shapes, exact-fp32 for the tiny K), so equality is at rounding level, not bitwise."""
    from gen_adversarial_amd import _lib as L
    m, spec = model, model['spec']
    rows, rep = 32, 4
    gen = torch.Generator().manual_seed(23)
    imgs = torch.rand(rows // rep, 3, 64, 64, generator=gen)
    eps = [torch.randn(rows, spec.num_latent, gs.res, gs.res, generator=gen) for gs in spec.groups]
    dlog = torch.randn(rows, 100, generator=gen)
    out = []
    for halo in (False, True):
        monkeypatch.setattr(Engine, 'fuse_halo_cells', halo)
        eng = engine(m, rows, rep)
        n_halo = sum(isinstance(d, L.DecCellHaloDesc) for pl in (eng.fwd, eng.bwd) for d in pl.descs)
        assert n_halo == (4 if halo else 0), n_halo
        fill(eng, imgs, eps)
        eng.forward()
        eng.dlogits.view(rows, -1).copy_(dlog.to(DEV))
        eng.backward()
        torch.cuda.synchronize()
        out.append((eng.purified.clone(), eng.logits.clone(), eng.dx.clone()))
        del eng
        torch.cuda.empty_cache()
    for a, b, what in zip(out[0], out[1], ('purified', 'logits', 'input gradient')):
        e = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
        print(f'halo-fused vs unfused post-processing cells, {what}: {e:.2e}')
        assert e < 2e-5, what


def test_bench_shape_1024_rows_fused_plan_vs_unfused_plan_and_oracle(model, monkeypatch):
    """The shape bench.py times (1024-row chunk plans since r04: 32 images x EoT 32): at 1024 / 512 workgroups the engine
    selects ga_dec_cell for 32 cells per direction BY ITSELF.  (a) That plan against the same plan built from the unfused launches,
    both with the tune table bench.py uses: equal to rounding (1e-5 of the tensor's scale; bitwise when the table gives the unfused
    1x1 convs no split-K — reported, not asserted: bitwise equality of the KERNELS is the 8-row test above, which pins the kernels
    instead of relying on the table's contents).  (b) Rows 0..3 of the fused plan against the CPU oracle on those four
    rows (rows are independent; the cotangent is zero on the other 1020): logits / purified at 1e-3, the input gradient on every
    element given the engine's ReLU / max-pool decisions."""
    from gen_adversarial_amd import _lib as L
    from oracle import defender_oracle as D
    m, spec = model, model['spec']
    rows, rep, k = 1024, 32, 4
    gen = torch.Generator().manual_seed(31)
    imgs = torch.rand(rows // rep, 3, 64, 64, generator=gen)
    eps = [torch.randn(rows, spec.num_latent, gs.res, gs.res, generator=gen) for gs in spec.groups]
    cot = torch.zeros(rows, 100)
    cot[:k] = torch.randn(k, 100, generator=gen)
    dense = torch.randn(rows, 100, generator=gen)
    out = {}
    for fuse in (True, False):
        monkeypatch.setattr(Engine, 'fuse_dec_cells', fuse)
        eng = engine(m, rows, rep)
        n_fused = sum(isinstance(d, L.DecCellDesc) for pl in (eng.fwd, eng.bwd) for d in pl.descs)
        assert n_fused == (64 if fuse else 0), n_fused           # the default gate (160 workgroups) picks them at this size
        fill(eng, imgs, eps)
        eng.forward()
        eng.dlogits.view(rows, -1).copy_(dense.to(DEV))
        eng.backward()
        g_dense = eng.dx.clone()
        eng.dlogits.view(rows, -1).copy_(cot.to(DEV))
        eng.backward()
        torch.cuda.synchronize()
        out[fuse] = (eng.purified.clone(), eng.logits.clone(), g_dense, eng.dx.clone())
        if fuse:
            # ---- (b) the oracle on rows 0..3 = image 0 under its first four latent draws
            torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
            e4 = [e[:k] for e in eps]
            x0 = imgs[:1].clone().requires_grad_(True)
            nz = torch.randn(k, 3, 64, 64, generator=gen)          # drawn and scaled by eps = 0 (abstract_models.py:132-138)
            lg, pur = D.nvae_defender(m['sd'], spec, m['vsd'], m['vspec'], x0.repeat_interleave(k, dim=0), m['alphas'], e4, nz, 0.0)
            e_l, e_p = err(eng.logits[:k], lg), err(eng.purified[:k], pur)
            print(f'1024-row fused plan vs oracle, rows 0..{k - 1}: logits {e_l:.2e} purified {e_p:.2e}')
            assert e_l < TOL and e_p < TOL
            from gradcheck import assert_grad_given_engine_decisions
            assert_grad_given_engine_decisions(
                eng, lambda t: (D.nvae_defender(m['sd'], spec, m['vsd'], m['vspec'], t.repeat_interleave(k, dim=0), m['alphas'], e4,
                                                nz, 0.0)[0] * cot[:k]).sum(),
                imgs[:1], eng.dx[:1], 1e-3, 'input gradient of rows 0..3 inside the fused 1024-row plan', min_matched=8, rows=slice(0, k))
            assert float(eng.dx[1:].abs().max()) == 0.0           # images whose rows carry no cotangent get no gradient
        del eng
        torch.cuda.empty_cache()
    for a, b, what in zip(out[True], out[False], ('purified', 'logits', 'dense input gradient', 'sparse input gradient')):
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
        print(f'fused vs unfused 1024-row plans, {what}: max |diff| {e:.1e} of the scale, bitwise {torch.equal(a, b)}')
        assert e < 1e-5, f'fused and unfused 1024-row plans differ in the {what}'
