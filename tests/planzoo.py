"""
The dry-run plans of every shipped defender, built the way the CPU tests build them one by one (tests/test_host_cpu.py,
test_alpha_search_cpu.py, test_alpha_grad_cpu.py, test_cot_rep_owners_cpu.py, test_resnet_cot_rep_cpu.py): the golden NVAE
configs, the e4e and Style-Transformer defenders, the ND-VAE and A-VAE competitors, the ResNet / ResNeXt classifiers with
their noise and blur fronts, and the K-cotangent, alpha_rows and alpha_grad variants of those.  No GPU, no kernel launch:
`dry_engines()` yields (name, engine) pairs whose fwd / bwd plans hold the descriptors as the engines compose them.
"""
import torch

from gen_adversarial_amd.engine import Engine


def _golden():
    from conftest import golden_cfg, load_golden
    from gen_adversarial_amd.nvae_spec import build_spec, init_nvae_state_dict
    from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict
    for name in ('A_cos07', 'A_zero_noise2', 'B_adaptive', 'A_nf2'):
        cfg, res = golden_cfg(load_golden(f'nvae_{name}.npz'))
        vspec, vsd = build_vgg_spec(10, 16), init_vgg_state_dict(10, 16, 2)
        n = len(build_spec(cfg, res).groups)

        def build(cfg=cfg, res=res, n=n, **kw):
            return Engine(init_nvae_state_dict(cfg, res, 1), cfg, res, vsd, vspec, alphas=[0.3] * n, device='cpu', dry_run=True, **kw)
        yield name, lambda b=build: b(rows=2, rep=1)
        yield f'{name}.eot', lambda b=build: b(rows=4, rep=2)
        yield f'{name}.noise', lambda b=build: b(rows=4, rep=2, share_encoder=True, noise_eps=0.1)
        yield f'{name}.blur', lambda b=build: b(rows=4, rep=2, blur=True)


def _alpha_variants():
    from test_alpha_grad_cpu import BUILDERS
    for ct, build in BUILDERS.items():
        yield f'alpha.{ct}.plain', lambda b=build: b()[0]
        yield f'alpha.{ct}.grad', lambda b=build: b(alpha_grad=True)[0]
        yield f'alpha.{ct}.rows', lambda b=build: b(alpha_rows=True)[0]
        yield f'alpha.{ct}.rows+grad', lambda b=build: b(alpha_rows=True, alpha_grad=True)[0]


def _defenders():
    from test_host_cpu import _small_e4e_defense
    yield 'e4e', lambda: _small_e4e_defense()[0]
    yield 'e4e.shared', lambda: _small_e4e_defense(rows=6, rep=3, share_encoder=True)[0]

    def trans():
        from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
        from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
        from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
        tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
        gspec = build_stylegan_spec(32, width_div=8, style_dim=tspec.d_model)
        cspec, csd = build_resnet_spec(4, 2, (1, 1, 1, 1), 4, 8), init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)
        eng = Engine.bare(4, device='cpu', dry_run=True, rep=2, resolution=(3, 64, 64), alphas=[0.1] * 16, share_encoder=True)
        return eng.build_trans_defense(tsd, tspec, init_stylegan_state_dict(gspec, 2), gspec, torch.zeros(16, tspec.d_model), csd, cspec,
                                       pool_to=32, mid=128, crop=16) or eng
    yield 'trans', trans


def _competitors():
    from test_cot_rep_owners_cpu import K, _avae, _ndvae
    from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
    res = (build_resnet_spec(4, 8, (1, 1, 1, 1)), init_resnet_state_dict(4, 8, 3, (1, 1, 1, 1)))
    for name, build in (('ndvae', _ndvae), ('avae', _avae)):
        yield f'{name}.vgg', lambda b=build: b(1)
        yield f'{name}.vgg.K{K}', lambda b=build: b(K)
        yield f'{name}.resnet', lambda b=build: b(1, *res)


def _classifiers():
    from test_resnet_cot_rep_cpu import FRONTS, K, NETS, _engine
    for net in NETS:
        for front in FRONTS:
            yield f'{net}.{front}', lambda n=net, f=front: _engine(n, f)
            yield f'{net}.{front}.K{K}', lambda n=net, f=front: _engine(n, f, cot_rep=K)


def dry_engines():
    """(name, engine), one engine alive at a time"""
    for group in (_golden, _defenders, _alpha_variants, _competitors, _classifiers):
        for name, build in group():
            yield name, build()


# ---------------------------------------------------------------------------------------------------- on a device
def nvae_variants(dev, first, model, eot=32, big=512):
    """(name, build) of the configs[1] NVAE + VGG plans bench.py builds and times beside its 1024-row chunk plan: the `big`-row
    (16 images) and the eot-row (1 image, the reference protocol) plans, the same two with the encoder shared by the EoT replicas
    (addend_rep > 1), the K-cotangent class-Jacobian plans of bench.class_jacobian_measurement (share_encoder, noise_eps 0.0,
    cot_rep = K: K = 16 at one image, K = 4 at 16 images; dact_rep > 1) and the fp32 secondary at eot rows.

    `first`, `model` are what bench.build_model returned for the chunk plan (of `first` only rep, noise_eps and the WeightStore are
    read: the engine itself may be gone).  Each variant is bench.clone_engine's Engine call, the one build_model makes, over that
    model and that store: build_model itself draws the state dicts again on every call (9 s each where this was measured, against
    under 0.1 s for an engine; the plans hold the same descriptors either way), and nothing is folded or split twice.  Real engines
    on `dev`, built when `build` is called."""
    from types import SimpleNamespace as NS
    from bench import clone_engine
    from gen_adversarial_amd.engine import Engine
    from gen_adversarial_amd.nvae_spec import ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION

    def plain(rows, precision='bf16x3', share_encoder=False):
        like = NS(rows=rows, rep=eot, noise_eps=first.noise_eps, store=first.store)
        return clone_engine(like, model, dev, NS(precision=precision, share_encoder=share_encoder))

    def jacobian(rows, K):
        sd, vsd, vspec, alphas = model
        return Engine(sd, ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION, vsd, vspec, rows=rows, rep=eot, alphas=alphas, temperature=0.6,
                      noise_eps=0.0, device=dev, precision='bf16x3', share_encoder=True, store=first.store, cot_rep=K)
    for rows in (big, eot):
        yield f'nvae.{rows}', lambda r=rows: plain(r)
        yield f'nvae.{rows}.shared', lambda r=rows: plain(r, share_encoder=True)
    yield f'nvae.{eot}.shared.K16', lambda: jacobian(eot, 16)
    yield f'nvae.{big}.shared.K4', lambda: jacobian(big, 4)
    yield f'nvae.{eot}.fp32', lambda: plain(eot, precision='fp32')


def device_engines(dev, dry_run=False):
    """(name, build) of the reduced engines the GPU tests build beside the benchmarked ones: the ND-VAE and A-VAE defenders of
    tests/test_competitors_gpu.py, the K-cotangent engines of tests/test_competitor_class_jacobian_gpu.py and
    tests/test_resnet_cot_rep_gpu.py, and the alpha-table / alpha-gradient engines of tests/alpha_search_cases.py.  Real
    engines on `dev` (the tuned tiles and workspaces are the ones a run uses); each is built when its `build` is called."""
    from alpha_search_cases import B, E, K, NVAE_CFG
    from gen_adversarial_amd.avae_spec import build_avae_spec, init_avae_state_dict
    from gen_adversarial_amd.ndvae_spec import build_ndvae_spec, init_ndvae_h, init_ndvae_state_dict
    from gen_adversarial_amd.nvae_spec import build_spec, nvae_checkpoint
    from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
    from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict
    from test_host_cpu import _small_e4e_defense
    nd_cfg = {'x_channels': 3, 'encoding_channels': 8, 'pre_proc_groups': 2, 'scales': 2, 'groups': 1, 'cells': 2, 'input_dim': 32}
    vgg = lambda: (build_vgg_spec(100, 16), init_vgg_state_dict(100, 16, 3))
    rows, rep = 4, 2

    def ndvae(k):
        cspec, csd = vgg()
        e = Engine.bare(rows, device=dev, dry_run=dry_run, rep=rep, resolution=(3, 32, 32), alphas=[], noise_eps=0.07, cot_rep=k)
        e.build_ndvae_defense(init_ndvae_state_dict(nd_cfg, 21), build_ndvae_spec(nd_cfg), init_ndvae_h(nd_cfg, 22), csd, cspec)
        return e

    def avae(k):
        cspec, csd = vgg()
        e = Engine.bare(rows, device=dev, dry_run=dry_run, rep=rep, resolution=(3, 64, 64), alphas=[], cot_rep=k)
        e.build_avae_defense(init_avae_state_dict(64, 51, 8), build_avae_spec(64, 8), 2, csd, cspec)
        return e
    for k in (1, 3):
        yield f'ndvae.K{k}', lambda k=k: ndvae(k)
        yield f'avae.K{k}', lambda k=k: avae(k)

    nets = {'resnet': (4, 8, (2, 1, 1, 1)), 'resnext': (4, 2, (1, 1, 1, 1), 4, 8)}
    fronts = {'plain': dict(rows=2, rep=1), 'noise': dict(rows=4, rep=2, noise_eps=0.05), 'blur': dict(rows=2, rep=2, blur=True)}
    for net, a in nets.items():
        for front, kw in fronts.items():
            yield f'{net}.{front}.K3', lambda a=a, kw=kw: Engine(None, None, (3, 64, 64), init_resnet_state_dict(a[0], a[1], 3, *a[2:]),
                                                                  build_resnet_spec(*a), alphas=[], device=dev, dry_run=dry_run, cot_rep=3, **kw)

    R_ = B * K * E

    def nvae(**kw):
        res = (3, 64, 64)
        sd = nvae_checkpoint(NVAE_CFG, res, seed=5)['state_dict_temp=0.6']
        n = len(build_spec(NVAE_CFG, res).groups)
        return Engine(sd, NVAE_CFG, res, init_vgg_state_dict(100, 16, seed=6), build_vgg_spec(100, 16), rows=R_, rep=K * E,
                      alphas=[0.1 * i for i in range(n)], device=dev, dry_run=dry_run, share_encoder=True, **kw)

    def e4e(**kw):
        _, (esd, espec, gsd, gspec, avg, csd, cspec, alphas) = _small_e4e_defense(dry_run=True, device='cpu')
        e = Engine.bare(R_, device=dev, dry_run=dry_run, rep=K * E, resolution=(3, 64, 64), alphas=alphas, share_encoder=True, **kw)
        e.build_e4e_defense(esd, espec, gsd, gspec, avg, csd, cspec, pool_to=64)
        return e

    def trans(**kw):
        tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
        gspec = build_stylegan_spec(64, width_div=8, style_dim=tspec.d_model)
        cspec, csd = build_resnet_spec(4, 2, (1, 1, 1, 1), 4, 8), init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)
        e = Engine.bare(R_, device=dev, dry_run=dry_run, rep=K * E, resolution=(3, 64, 64), alphas=[0.1] * 16, share_encoder=True, **kw)
        e.build_trans_defense(tsd, tspec, init_stylegan_state_dict(gspec, 2), gspec, torch.zeros(16, tspec.d_model), csd, cspec,
                              pool_to=64, mid=128, crop=16)
        return e
    for name, build in (('nvae', nvae), ('e4e', e4e), ('trans', trans)):
        yield f'alpha.{name}.rows', lambda b=build: b(alpha_rows=True)
        yield f'alpha.{name}.grad', lambda b=build: b(alpha_grad=True)
