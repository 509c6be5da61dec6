"""
GPU: ga_randn (csrc/randn.hip) against the CPU restatement of its contract (gen_adversarial_amd/noise.py), and the defenders'
seeded draws (`seeded_noise`) built on it.

Why 8e-6 * scale bounds |y - float64 reference| (scale 1: 16 fp32 ulps of a number in [4, 8), 16 * 2^-21 = 7.6e-6; the largest
possible |z| is sqrt(-2 ln 2^-24) = 5.768): the uniforms are exact in fp32, so only the functions err.  With e = 2^-24 = 6e-8 (half
an ulp, relative): logf is good to 1 ulp (2 e relative), -2 * L is exact, sqrtf is correctly rounded and halves its argument's
relative error (e + e); sincospif of the exact 2 u is good to 2 ulps of a number below 1 (<= 2 e absolute, 2 e relative to the
radius); the product and the multiplication by `scale` round once each (e + e).  Sum: <= 6 e of the radius = 5.768 * 3.6e-7 =
2.1e-6 — inside 8e-6 with a factor 3.8 to spare, while one wrong counter or key bit gives an unrelated normal: an error of order 1.
"""
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from gen_adversarial_amd import _lib as L   # noqa: E402
from gen_adversarial_amd import noise as N   # noqa: E402
from gen_adversarial_amd.experiments.load_defense import load   # noqa: E402
from gen_adversarial_amd.nvae_spec import build_spec, nvae_checkpoint   # noqa: E402
from gen_adversarial_amd.vgg_spec import init_vgg_state_dict   # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                       # floats of a NaN pattern behind every buffer
NAN_BITS = 0x7fc01234
TOL = 8e-6
SHAPES = [(3, 4), (5, 320), (2, 3072), (7, 20 * 4 * 4), (70000, 4)]      # 7 x 80 = 560 quads: not a multiple of 256
HIGH = dict(seed=0xDEADBEEF00000001, draw=0xFFFFFFFF, stream=0x80000001, row0=(1 << 31) + 5)


def _guarded(n):
    buf = torch.empty(n + GUARD, device=DEV, dtype=torch.float32)
    buf.view(torch.int32).fill_(NAN_BITS)
    return buf


def _intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == NAN_BITS).all())


def _randn(rows, inner, seed=11, draw=2, stream=1, row0=0, scale=1.0, mode=0, coef_eps=None):
    """-> (y [rows, inner] as a CPU tensor, coef [rows] or None); asserts that nothing behind y, coef or ws was written"""
    y = _guarded(rows * inner)
    coef = ws = None
    tail = (None, 0.0, None, 0)
    if coef_eps is not None:
        nblk = (inner // 4 + 255) // 256
        coef, ws = _guarded(rows), _guarded(rows * nblk)
        tail = (coef.data_ptr(), coef_eps, ws.data_ptr(), rows * nblk)
    L.check(L.lib.ga_randn(y.data_ptr(), rows, inner, seed, draw, stream, row0, scale, mode, *tail, torch.cuda.current_stream().cuda_stream),
            'ga_randn')
    torch.cuda.synchronize()
    assert _intact(y, rows * inner), 'wrote past the end of y'
    if coef is not None:
        assert _intact(coef, rows) and _intact(ws, rows * nblk), 'wrote past the end of coef or ws'
        coef = coef[:rows].cpu()
    return y[:rows * inner].view(rows, inner).cpu(), coef


def _bits(t):
    return t.view(torch.int32).numpy().view(np.uint32)


@pytest.mark.parametrize('rows, inner', SHAPES)
def test_raw_words_equal_the_reference(rows, inner):
    y, _ = _randn(rows, inner, mode=1)
    assert np.array_equal(_bits(y), N.reference_bits(11, 2, 1, 0, rows, inner))


def test_raw_words_with_high_bit_counters():
    """no sign extension of the row, the draw or the stream, and the key halves in the right order"""
    y, _ = _randn(6, 40, mode=1, **HIGH)
    assert np.array_equal(_bits(y), N.reference_bits(HIGH['seed'], HIGH['draw'], HIGH['stream'], HIGH['row0'], 6, 40))
    top, _ = _randn(2, 8, mode=1, row0=(1 << 32) - 2)            # the last two rows there are
    assert np.array_equal(_bits(top), N.reference_bits(11, 2, 1, (1 << 32) - 2, 2, 8))


@pytest.mark.parametrize('scale', [1.0, 0.8])
@pytest.mark.parametrize('rows, inner', SHAPES)
def test_normals_against_the_float64_reference(rows, inner, scale):
    y, _ = _randn(rows, inner, scale=scale)
    ref = N.reference_randn(11, 2, 1, 0, rows, inner, scale=scale)
    err = np.abs(y.numpy().astype(np.float64) - ref).max()
    print(f'   ({rows}, {inner}) scale {scale}: max |y - ref| = {err:.3e}, max |y| = {np.abs(ref).max():.3f}')
    assert err <= TOL * scale
    yh, _ = _randn(6, 40, scale=scale, **HIGH)
    refh = N.reference_randn(HIGH['seed'], HIGH['draw'], HIGH['stream'], HIGH['row0'], 6, 40, scale=scale)
    assert np.abs(yh.numpy().astype(np.float64) - refh).max() <= TOL * scale


def test_rows_do_not_depend_on_the_launch():
    whole, _ = _randn(8, 320)
    lo, _ = _randn(4, 320, row0=0)
    hi, _ = _randn(4, 320, row0=4)
    assert torch.equal(_as_int(whole), _as_int(torch.cat([lo, hi])))
    big, _ = _randn(600, 320)                                     # 48000 quads: many workgroups, rows cut inside workgroups
    assert torch.equal(_as_int(big[:8]), _as_int(whole))


def _as_int(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('rows, inner', [(4, 3072), (3, 3 * 8 * 8)])
def test_coef_is_eps_over_the_row_norm(rows, inner):
    y, coef = _randn(rows, inner, coef_eps=2.0)
    ref = N.reference_randn(11, 2, 1, 0, rows, inner)
    want = 2.0 / np.sqrt((ref ** 2).sum(axis=1))
    rel = np.abs(coef.numpy().astype(np.float64) / want - 1.0).max()
    print(f'   ({rows}, {inner}): max relative error of coef = {rel:.3e}')
    # every element is within 8e-6 of the reference (above) and |z| is 1 on average, so the norm is within 8e-6 relative even if
    # every element were off by the whole bound in the worst direction; the sum itself: a thread adds 4 squares (3 additions), the
    # wave 6 shuffle steps, the workgroup 3 more, the second launch at most 11 (3072 / 4 / 256 = 12 partials): 23 roundings of
    # 6e-8 = 1.4e-6, halved by the square root, + 1.2e-7 for the root and the division: 8e-6 + 0.7e-6 + 0.2e-6 < 2e-5
    assert rel <= 2e-5
    y2, coef2 = _randn(rows, inner, coef_eps=2.0)
    assert torch.equal(_as_int(coef), _as_int(coef2)) and torch.equal(_as_int(y), _as_int(y2))         # no atomics: same bits
    plain, _ = _randn(rows, inner)
    assert torch.equal(_as_int(y), _as_int(plain))


# ---------------------------------------------------------------------------------------------------------------- engines
CFG = {'initial_channels': 8, 'num_pre-post_process_blocks': 1, 'num_pre-post_process_cells': 2, 'num_scales': 3,
       'num_groups_per_scale': 2, 'is_adaptive': False, 'min_groups_per_scale': 1, 'num_cells_per_group': 1,
       'num_latent_per_group': 4, 'num_logistic_mixtures': 10, 'num_nf_cells': None}
RES = (3, 64, 64)
EOT, IMAGES = 2, 4
ROWS = EOT * IMAGES


@pytest.fixture(scope='module')
def nvae(tmp_path_factory):
    """the reduced NVAE defender of tests/test_api_gpu.py (input noise eps 2.0) at EoT 2"""
    d = tmp_path_factory.mktemp('noise_ckpt')
    torch.save(nvae_checkpoint(CFG, RES, seed=5), d / 'nvae.pt')
    torch.save({'state_dict': init_vgg_state_dict(100, 16, seed=6)}, d / 'vgg.pt')
    n_groups = len(build_spec(CFG, RES).groups)
    y = {'classifier_path': str(d / 'vgg.pt'), 'autoencoder_path': str(d / 'nvae.pt'),
         'interpolation_alphas': [round(i / (n_groups - 1), 3) for i in range(n_groups)],
         'alpha_attenuation': 0.7, 'initial_noise_eps': 2.0, 'gaussian_blur_input': False}
    with open(d / 'cfg.yaml', 'w') as f:
        yaml.safe_dump(y, f)
    args, model = load(Namespace(config=str(d / 'cfg.yaml'), experiment='ids', defense_type='ours', eot_steps=EOT, device=DEV))
    x = torch.rand(IMAGES, *RES, generator=torch.Generator().manual_seed(21)).to(DEV)
    yield model, x, str(d / 'cfg.yaml')
    model.model.seeded_noise(None)
    model.model.fixed_noise(None, None)


def _check_draws(eng, seed, draw, row0, scale=1.0):
    """check (1): every tensor the engine draws, against the reference at (seed, draw, its stream, row0)"""
    torch.cuda.synchronize()
    assert len(eng.eps) > 0
    for i, e in enumerate(eng.eps):
        ref = N.reference_randn(seed, draw, i, row0, e.shape[0], e[0].numel(), scale=scale)
        err = np.abs(e.flatten(1).cpu().numpy().astype(np.float64) - ref).max()
        assert err <= TOL * scale, (i, err)
    if eng.noise is not None:
        ref = N.reference_randn(seed, draw, N.STREAM_INPUT, row0, eng.noise.shape[0], eng.noise[0].numel())
        assert np.abs(eng.noise.flatten(1).cpu().numpy().astype(np.float64) - ref).max() <= TOL
        return ref
    return None


def test_nvae_defender_draws_logits_and_gradient(nvae):
    model, x, _ = nvae
    owner = model.model
    rng_gpu, rng_cpu = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    owner.seeded_noise(7)
    xd = x.clone().requires_grad_(True)
    rows1 = owner.forward_rows(xd, rep=EOT)
    (g1,) = torch.autograd.grad(rows1.sum(), [xd])
    eng = owner._engine(ROWS, EOT)
    # (1) the draws
    ref_noise = _check_draws(eng, 7, 0, 0)
    want = 2.0 / np.sqrt((ref_noise ** 2).sum(axis=1))
    assert np.abs(eng.noise_coef.cpu().numpy().astype(np.float64) / want - 1.0).max() <= 2e-5
    snap = owner._snapshot_noise(eng)
    # (2) the counter advances; the same (seed, draw) gives the same bits
    with torch.no_grad():
        rows2 = owner.forward_rows(xd, rep=EOT)
    assert owner._noise_draw == 2 and not torch.equal(rows1, rows2)
    owner.seeded_noise(7)
    rows3 = owner.forward_rows(xd, rep=EOT)
    assert torch.equal(rows3.detach(), rows1.detach())
    # (3) no torch generator was touched
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng_gpu) and torch.equal(torch.get_rng_state(), rng_cpu)
    # (4) the same draws as tensors through fixed_noise (which wins over the seed): torch's norm is the only difference
    owner.fixed_noise(snap[0], snap[1][0])
    rows4 = owner.forward_rows(xd, rep=EOT)
    (g4,) = torch.autograd.grad(rows4.sum(), [xd])
    owner.fixed_noise(None, None)
    e_l = (rows4 - rows1).abs().max().item() / rows1.abs().max().item()
    e_g = (g4 - g1).abs().max().item() / g1.abs().max().item()
    print(f'   seeded draws fed back through fixed_noise: logits {e_l:.2e}, input gradient {e_g:.2e} (of max |value|)')
    assert e_l <= 2e-5 and e_g <= 2e-5
    # (5) images 2..3 alone, told where their rows start, see the draws they saw in the four-image call
    owner.seeded_noise(7, draw=0, first_row=2 * EOT)
    with torch.no_grad():
        tail = owner.forward_rows(x[2:], rep=EOT)
    _check_draws(owner._engine(2 * EOT, EOT, forward_only=True), 7, 0, 2 * EOT)
    e_t = (tail - rows1[2 * EOT:].detach()).abs().max().item() / rows1.abs().max().item()
    print(f'   rows {2 * EOT}..{ROWS - 1} as a call of their own: logits {e_t:.2e} (of max |value|)')
    assert e_t <= 2e-5
    # the call's own first_row is added to the owner's
    owner.seeded_noise(7, draw=0, first_row=EOT)
    with torch.no_grad():
        tail2 = owner.forward_rows(x[2:], rep=EOT, first_row=EOT)
    assert torch.equal(tail2, tail)
    # one first row per image: images 3 and 0 in one call, not neighbours in the four-image call, each at its own rows
    owner.seeded_noise(7, draw=0, first_row=[3 * EOT, 0])
    with torch.no_grad():
        pair = owner.forward_rows(x[[3, 0]], rep=EOT)
    eng2 = owner._engine(2 * EOT, EOT, forward_only=True)
    torch.cuda.synchronize()
    for k, r0 in enumerate((3 * EOT, 0)):
        for i, e in enumerate(eng2.eps):
            ref = N.reference_randn(7, 0, i, r0, EOT, e[0].numel())
            assert np.abs(e[k * EOT:(k + 1) * EOT].flatten(1).cpu().numpy().astype(np.float64) - ref).max() <= TOL
        ref = N.reference_randn(7, 0, N.STREAM_INPUT, r0, EOT, eng2.noise[0].numel())
        assert np.abs(eng2.noise[k * EOT:(k + 1) * EOT].flatten(1).cpu().numpy().astype(np.float64) - ref).max() <= TOL
        want = 2.0 / np.sqrt((ref ** 2).sum(axis=1))
        assert np.abs(eng2.noise_coef[k * EOT:(k + 1) * EOT].cpu().numpy().astype(np.float64) / want - 1.0).max() <= 2e-5
    want_rows = torch.cat([rows1[3 * EOT:4 * EOT], rows1[:EOT]]).detach()
    e_p = (pair - want_rows).abs().max().item() / rows1.abs().max().item()
    print(f'   images 3 and 0 as one call with their own first rows: logits {e_p:.2e} (of max |value|)')
    assert e_p <= 2e-5
    with pytest.raises(ValueError):
        owner.seeded_noise(7, draw=0, first_row=[0])
        owner.forward_rows(x[:2], rep=EOT)
    owner.seeded_noise(None)


def test_trans_defender_draws_are_scaled(tmp_path):
    """the reduced Style-Transformer defender of tests/test_trans_gpu.py: eps is N(0, 0.8) (eps_std)"""
    from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
    tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
    gspec = build_stylegan_spec(64, width_div=8, style_dim=tspec.d_model)
    gsd = init_stylegan_state_dict(gspec, 2)
    csd = init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)
    avg = 0.3 * torch.randn(16, tspec.d_model, generator=torch.Generator().manual_seed(4))
    ck = {'state_dict': {**{'encoder.module.' + k: v for k, v in tsd.items()}, **{'decoder.module.' + k: v for k, v in gsd.items()}},
          'latent_avg': avg, 'opts': {'output_size': gspec.size, 'input_nc': 3, 'start_from_latent_avg': True, 'learn_in_w': False}}
    torch.save(ck, tmp_path / 'trans.pt')
    torch.save({'state_dict': csd}, tmp_path / 'resnext.pt')
    with open(tmp_path / 'cfg.yaml', 'w') as f:
        yaml.safe_dump({'classifier_path': str(tmp_path / 'resnext.pt'), 'autoencoder_path': str(tmp_path / 'trans.pt'),
                        'interpolation_alphas': [0.1 * (j % 5) for j in range(16)], 'alpha_attenuation': 0.5, 'initial_noise_eps': 0.0,
                        'gaussian_blur_input': True}, f)
    eot = 3
    args, model = load(Namespace(config=str(tmp_path / 'cfg.yaml'), experiment='cars', defense_type='ours', eot_steps=eot, device=DEV))
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(DEV).requires_grad_(True)
    model.model.seeded_noise(9, draw=5, first_row=12)
    out = model(x)
    eng = model.model._engine(eot, eot)
    assert eng.eps_std == pytest.approx(0.8) and eng.noise is None
    _check_draws(eng, 9, 5, 12, scale=eng.eps_std)
    assert torch.isfinite(out).all()
    model.model.seeded_noise(None)


def test_ndvae_defender_input_noise_keeps_its_constant_coefficient(tmp_path):
    """the reduced ND-VAE defender of tests/test_competitors_gpu.py: x + noise_std * N(0, 1) (noise_is_std)"""
    from gen_adversarial_amd.ndvae_spec import init_ndvae_state_dict
    cfg = {'x_channels': 3, 'encoding_channels': 4, 'pre_proc_groups': 2, 'scales': 1, 'groups': 2, 'cells': 1, 'input_dim': 64}
    torch.save(init_ndvae_state_dict(cfg, 31), tmp_path / 'ndvae.pt')
    torch.save({'state_dict': init_vgg_state_dict(100, 16, 32)}, tmp_path / 'vgg.pt')
    y = {'classifier_path': str(tmp_path / 'vgg.pt'), 'autoencoder_path': str(tmp_path / 'ndvae.pt'), 'noise_std': 0.05,
         'x_channels': 3, 'pre_proc_groups': 2, 'encoding_channels': 4, 'scales': 1, 'groups': 2, 'cells': 1}
    with open(tmp_path / 'cfg.yaml', 'w') as f:
        yaml.safe_dump(y, f)
    args, model = load(Namespace(config=str(tmp_path / 'cfg.yaml'), experiment='ids', defense_type='ND-VAE', eot_steps=2, device=DEV))
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).to(DEV).requires_grad_(True)
    model.model.seeded_noise(1 << 40, draw=1)
    out = model(x)
    eng = model.model._engine(4, 2)
    assert eng.noise_is_std and eng.noise is not None
    _check_draws(eng, 1 << 40, 1, 0)
    assert bool((eng.noise_coef == eng.noise_eps).all()) and eng.noise_eps == pytest.approx(0.05)
    assert torch.isfinite(out).all()
    model.model.seeded_noise(None)


def test_driver_with_a_noise_seed_repeats_itself(nvae, tmp_path):
    """experiments/seeded_defense.py --noise_seed 3 (the driver with seeded draws), twice, each in a fresh process: the same results.json"""
    _, _, cfg = nvae
    got = []
    for run in ('a', 'b'):
        cwd = tmp_path / run
        cwd.mkdir()
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        cmd = [sys.executable, '-m', 'gen_adversarial_amd.experiments.seeded_defense', '--synthetic', '3', '--eot_steps', str(EOT),
               '--defense_type', 'ours', '--experiment', 'ids', '--config', cfg, '--attack', 'pgd', '--batch_images', '2',
               '--schedule', 'dynamic', '--noise_seed', '3']
        p = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got.append(open(cwd / 'results' / 'cfg' / 'results.json').read())
    assert got[0] == got[1] and 'PGD' in got[0]


def _probe(batched):
    """an 'attack' that reports a number the draws decide: the largest EoT-mean logit of one more defender call"""
    def run(x, y, net):
        with torch.no_grad():
            top = net(x).max(dim=1).values
        return (torch.ones_like(top, dtype=torch.bool), top, x) if batched and x.shape[0] > 1 else (True, float(top[0]), x)
    run.batched = batched
    return run


def test_seeded_driver_results_do_not_depend_on_the_partition(nvae, tmp_path):
    """experiments/seeded_defense.run_worker in this process, on the defender of the fixture and two probe 'attacks' whose results
    are logits: what --noise_seed is for.  Same seed: the static and the dynamic schedule at one image per call give the same
    results.json bit for bit; a rank's r::W shard (images 1 and 3 of 4, one image per call) gives those images' rows bit for bit;
    at batches of two (where the calls, and so the draw numbers, are others than at one image per call) the shard's batch of images
    W apart gives what those images get as second images of the dynamic schedule's consecutive batches, within the 2e-5 of max
    |value| of the logit checks (they sit in other rows of the plan).  Another seed: other numbers."""
    from gen_adversarial_amd.experiments import seeded_defense as S
    model, x, _ = nvae
    y = torch.zeros(IMAGES, dtype=torch.long)
    attacks = {'one': _probe(False), 'many': _probe(True)}

    def run(name, seed, schedule, bi):
        args = Namespace(device=DEV, noise_seed=seed, batch_images=bi, schedule=schedule, attacks=attacks, results_folder=str(tmp_path))
        path = str(tmp_path / f'{name}.json')
        S.run_worker(0, 1, args, lambda a: (a, model), (x.cpu(), y), results_path=path)
        return open(path).read()
    static1, dynamic1 = run('s1', 3, 'static', 1), run('d1', 3, 'dynamic', 1)
    assert static1 == dynamic1
    assert run('s1_again', 3, 'static', 1) == static1 and run('other', 4, 'static', 1) != static1
    def table(text):                                              # results.json -> [attack (in the order of `attacks`), image]
        res = json.loads(text)
        return torch.tensor([res[k] for k in attacks])
    whole = table(static1)
    scale = whole.abs().max().item()
    shard = [1, 3]                                                # rank 1 of 2
    t1 = S.evaluate_seeded(model, attacks, x[shard], y[shard].to(DEV), lambda i: shard[i], 3, batch_images=1)
    assert torch.equal(t1[:, 1:].t(), whole[:, shard])
    t2 = S.evaluate_seeded(model, attacks, x[shard], y[shard].to(DEV), lambda i: shard[i], 3, batch_images=2)
    d2 = table(run('d2', 3, 'dynamic', 2))
    e_s = (t2[:, 1:].t() - d2[:, shard]).abs().max().item() / scale
    print(f'   batches of two: the static shard [1, 3] against batches [0, 1], [2, 3]: {e_s:.2e} (of max |value|)')
    assert e_s <= 2e-5
    assert model.model._noise_seed is None
