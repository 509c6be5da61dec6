"""
GPU: ga_nes_perturb / ga_nes_grad (csrc/nes.hip) against the float64 restatement of their contract
(gen_adversarial_amd/attacks/nes_ref.py), and NESAttack on a reduced NVAE + VGG defender.

Bounds.  z is ga_randn's normal, within 8e-6 of the float64 reference (tests/test_noise_gpu.py says why).
  perturb:  y = x +- sigma z: the error of z times sigma, plus one rounding each of the product and the sum, each at most 2^-24 of a
            number no larger than |x| + sigma |z|:   |y - ref| <= sigma 8e-6 + 2^-23 (|x| + sigma |z|).  The clamp is 1-Lipschitz.
  grad:     g = scale sum_i c_i z_i, `pairs` additions on the one path there is plus the roundings of one term and of the scale:
            |g - ref| <= |scale| [(pairs + 2) 2^-24 sum_i |c_i z_i| + 8e-6 sum_i |c_i|].
A misread sample or image index puts an unrelated normal in place of z: an error of order sigma, or of order |scale c|.
"""
import os
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
from gen_adversarial_amd.attacks import nes as A   # noqa: E402
from gen_adversarial_amd.attacks import nes_ref as R   # noqa: E402
from gen_adversarial_amd.experiments.load_defense import load   # noqa: E402
from gen_adversarial_amd.nvae_spec import build_spec, nvae_checkpoint   # noqa: E402
from gen_adversarial_amd.vgg_spec import init_vgg_state_dict   # noqa: E402

DEV = 'cuda:0'
GUARD = 64                       # floats of a NaN pattern behind every buffer
NAN_BITS = 0x7fc01234
SEED, DRAW = 0xDEADBEEF00000001, 0xFFFFFFF0
INNERS = [192, 12288, 1028]      # 3 x 8 x 8: fewer quads than one workgroup; 3 x 64 x 64; 257 quads: a partial last workgroup
SHAPES = [(inner, images, pairs) for inner in INNERS for images in (1, 3) for pairs in (1, 5)]
FAR = [900, 17, 5000]            # first rows of three images that are no neighbours


def _guarded(n):
    buf = torch.empty(n + GUARD, device=DEV, dtype=torch.float32)
    buf.view(torch.int32).fill_(NAN_BITS)
    return buf


def _intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == NAN_BITS).all())


def _rows_dev(image_row):
    return None if image_row is None else A._first_rows_device(image_row, DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _x(images, inner, seed=0):
    return torch.rand(images, inner, generator=torch.Generator().manual_seed(seed))


def _perturb(x, pairs, sigma, lo=1.0, hi=0.0, row0=0, image_row=None, seed=SEED, draw=DRAW):
    """x [images, inner] CPU fp32 -> y [images * pairs * 2, inner] on the CPU; asserts that nothing behind y was written"""
    images, inner = x.shape
    n = images * pairs * 2 * inner
    xd, y, rows = x.to(DEV), _guarded(n), _rows_dev(image_row)
    L.check(L.lib.ga_nes_perturb(xd.data_ptr(), y.data_ptr(), images, inner, pairs, seed, draw, N.STREAM_NES, row0,
                                 None if rows is None else rows.data_ptr(), sigma, lo, hi, _stream()), 'ga_nes_perturb')
    torch.cuda.synchronize()
    assert _intact(y, n), 'wrote past the end of y'
    return y[:n].view(images * pairs * 2, inner).cpu()


def _grad(c, images, inner, pairs, scale, row0=0, image_row=None, seed=SEED, draw=DRAW):
    n = images * inner
    cd, g, rows = c.to(DEV), _guarded(n), _rows_dev(image_row)
    L.check(L.lib.ga_nes_grad(cd.data_ptr(), g.data_ptr(), images, inner, pairs, seed, draw, N.STREAM_NES, row0,
                              None if rows is None else rows.data_ptr(), scale, _stream()), 'ga_nes_grad')
    torch.cuda.synchronize()
    assert _intact(g, n), 'wrote past the end of g'
    return g[:n].view(images, inner).cpu()


def _perturb_bound(x, z, pairs, sigma):
    """[images * pairs * 2, inner]: sigma 8e-6 + 2^-23 (|x| + sigma |z|)"""
    b = sigma * 8e-6 + 2.0 ** -23 * (np.abs(x.numpy().astype(np.float64))[:, None, :] + sigma * np.abs(z))      # [images, pairs, inner]
    return np.repeat(b[:, :, None, :], 2, axis=2).reshape(-1, x.shape[1])


def _as_int(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('sigma', [0.25, 1e-3])
@pytest.mark.parametrize('inner, images, pairs', SHAPES)
def test_perturb_against_the_float64_restatement(inner, images, pairs, sigma):
    x = _x(images, inner)
    z = R.directions(images, inner, pairs, SEED, DRAW, row0=40)
    bound = _perturb_bound(x, z, pairs, sigma)
    worst = 0.0
    for lo, hi in ((1.0, 0.0), (0.0, 1.0)):                                       # clamp off, clamp on
        y = _perturb(x, pairs, sigma, lo, hi, row0=40)
        ref = R.reference_perturb(x.numpy(), pairs, SEED, DRAW, row0=40, sigma=sigma, lo=lo, hi=hi)
        ratio = (np.abs(y.numpy().astype(np.float64) - ref) / bound).max()
        worst = max(worst, ratio)
        if lo <= hi:
            assert y.min() >= 0.0 and y.max() <= 1.0
            if sigma == 0.25:
                assert (y == 0.0).any() and (y == 1.0).any()                       # the clamp had something to do
    print(f'   perturb ({images} x {inner}, {pairs} pairs, sigma {sigma}): worst |y - ref| / bound = {worst:.3f}')
    assert worst <= 1.0


@pytest.mark.parametrize('inner, images, pairs', SHAPES)
def test_grad_against_the_float64_restatement(inner, images, pairs):
    scale = 1.0 / (2.0 * 1e-3 * pairs)
    c = torch.randn(images * pairs, generator=torch.Generator().manual_seed(1))
    g = _grad(c, images, inner, pairs, scale, image_row=FAR[:images])
    c64 = c.numpy().astype(np.float64)
    ref = R.reference_grad(c64, images, inner, pairs, SEED, DRAW, image_row=FAR[:images], scale=scale)
    z = R.directions(images, inner, pairs, SEED, DRAW, image_row=FAR[:images])
    ca = np.abs(c64).reshape(images, pairs)
    bound = scale * ((pairs + 2) * 2.0 ** -24 * np.einsum('bi,bie->be', ca, np.abs(z)) + 8e-6 * ca.sum(axis=1)[:, None])
    ratio = (np.abs(g.numpy().astype(np.float64) - ref) / bound).max()
    print(f'   grad ({images} x {inner}, {pairs} pairs): worst |g - ref| / bound = {ratio:.3f}')
    assert ratio <= 1.0


def test_a_misread_index_breaks_the_bounds_by_orders_of_magnitude():
    """references that take c of the wrong sample, c of the wrong image, or the rows of the wrong image"""
    images, inner, pairs, scale = 3, 1028, 5, 0.7
    c = torch.randn(images * pairs, generator=torch.Generator().manual_seed(1))
    g = _grad(c, images, inner, pairs, scale, image_row=FAR).numpy().astype(np.float64)
    c64 = c.numpy().astype(np.float64).reshape(images, pairs)
    z = R.directions(images, inner, pairs, SEED, DRAW, image_row=FAR)
    bound = scale * ((pairs + 2) * 2.0 ** -24 * np.einsum('bi,bie->be', np.abs(c64), np.abs(z)) + 8e-6 * np.abs(c64).sum(axis=1)[:, None])
    wrong = {'sample': c64[:, ::-1], 'image': c64[[1, 2, 0]]}
    for name, cw in wrong.items():
        ref = R.reference_grad(cw.ravel(), images, inner, pairs, SEED, DRAW, image_row=FAR, scale=scale)
        ratio = (np.abs(g - ref) / bound).max()
        print(f'   grad against a reference with the wrong {name}: {ratio:.1e} of the bound')
        assert ratio >= 1e3
    ref = R.reference_grad(c64.ravel(), images, inner, pairs, SEED, DRAW, image_row=[FAR[1], FAR[2], FAR[0]], scale=scale)
    assert (np.abs(g - ref) / bound).max() >= 1e3
    x, sigma = _x(images, inner), 0.25
    y = _perturb(x, pairs, sigma, image_row=FAR).numpy().astype(np.float64)
    pb = _perturb_bound(x, z, pairs, sigma)
    shifted = R.reference_perturb(x.numpy(), pairs, SEED, DRAW, image_row=[r + 1 for r in FAR], sigma=sigma)      # sample i + 1 for i
    swapped = R.reference_perturb(x.numpy(), pairs, SEED, DRAW, image_row=FAR, sigma=-sigma)                      # the signs the other way
    for name, ref in (('sample', shifted), ('sign', swapped)):
        ratio = (np.abs(y - ref) / pb).max()
        print(f'   perturb against a reference with the wrong {name}: {ratio:.1e} of the bound')
        assert ratio >= 1e3


def test_an_image_does_not_depend_on_the_launch():
    """bitwise: an image in a 3-image launch and alone; the image_row array and the row0 it spells out"""
    inner, pairs, sigma, scale = 1028, 5, 0.25, 0.3
    x = _x(3, inner)
    c = torch.randn(3 * pairs, generator=torch.Generator().manual_seed(2))
    y3 = _perturb(x, pairs, sigma, 0.0, 1.0, image_row=FAR).view(3, pairs * 2, inner)
    g3 = _grad(c, 3, inner, pairs, scale, image_row=FAR)
    for b in range(3):
        y1 = _perturb(x[b:b + 1], pairs, sigma, 0.0, 1.0, image_row=FAR[b:b + 1])
        g1 = _grad(c[b * pairs:(b + 1) * pairs], 1, inner, pairs, scale, image_row=FAR[b:b + 1])
        assert torch.equal(_as_int(y3[b]), _as_int(y1)) and torch.equal(_as_int(g3[b:b + 1]), _as_int(g1))
        assert torch.equal(_as_int(y1), _as_int(_perturb(x[b:b + 1], pairs, sigma, 0.0, 1.0, row0=FAR[b])))
        assert torch.equal(_as_int(g1), _as_int(_grad(c[b * pairs:(b + 1) * pairs], 1, inner, pairs, scale, row0=FAR[b])))
    rows = [70 + b * pairs for b in range(3)]
    assert torch.equal(_as_int(_perturb(x, pairs, sigma, row0=70)), _as_int(_perturb(x, pairs, sigma, image_row=rows)))
    assert torch.equal(_as_int(_grad(c, 3, inner, pairs, scale, row0=70)), _as_int(_grad(c, 3, inner, pairs, scale, image_row=rows)))
    assert torch.equal(_as_int(g3), _as_int(_grad(c, 3, inner, pairs, scale, image_row=FAR)))                      # no atomics: same bits


def test_rows_with_the_high_bit_set():
    """the last `pairs` rows there are: no sign extension of the row, from row0 and from the device array alike"""
    inner, pairs, sigma = 192, 5, 0.25
    top = (1 << 32) - pairs
    x = _x(1, inner)
    y = _perturb(x, pairs, sigma, row0=top)
    assert torch.equal(_as_int(y), _as_int(_perturb(x, pairs, sigma, image_row=[top])))
    z = N.reference_randn(SEED, DRAW, N.STREAM_NES, top, pairs, inner)[None]
    ref = R.reference_perturb(x.numpy(), pairs, SEED, DRAW, row0=top, sigma=sigma)
    assert (np.abs(y.numpy().astype(np.float64) - ref) / _perturb_bound(x, z, pairs, sigma)).max() <= 1.0
    c = torch.randn(pairs, generator=torch.Generator().manual_seed(3))
    g = _grad(c, 1, inner, pairs, 1.0, row0=top)
    assert torch.equal(_as_int(g), _as_int(_grad(c, 1, inner, pairs, 1.0, image_row=[top])))
    c64 = c.numpy().astype(np.float64)
    bound = (pairs + 2) * 2.0 ** -24 * (np.abs(c64) @ np.abs(z[0])) + 8e-6 * np.abs(c64).sum()
    assert (np.abs(g.numpy()[0] - c64 @ z[0]) <= bound).all()
    assert L.lib.ga_nes_perturb(x.to(DEV).data_ptr(), _guarded(16).data_ptr(), 1, inner, pairs, SEED, DRAW, N.STREAM_NES, top + 1, None, sigma,
                                1.0, 0.0, _stream()) == L.GA_E_BADARG


@pytest.mark.parametrize('sigma', [0.25, 1e-3])
def test_the_directions_are_ga_randns(sigma):
    """(y+ - y-) / (2 sigma) with the clamp off is ga_randn(scale = 1) at the same counters, within the roundings of the two sums:
    2^-22 (|x| / sigma + |z|)"""
    images, inner, pairs, row0 = 3, 1028, 5, 123
    x = _x(images, inner)
    y = _perturb(x, pairs, sigma, row0=row0).numpy().astype(np.float64).reshape(images, pairs, 2, inner)
    z = torch.empty(images * pairs, inner, device=DEV)
    L.check(L.lib.ga_randn(z.data_ptr(), images * pairs, inner, SEED, DRAW, N.STREAM_NES, row0, 1.0, 0, None, 0.0, None, 0, _stream()), 'ga_randn')
    z = z.cpu().numpy().astype(np.float64).reshape(images, pairs, inner)
    got = (y[:, :, 0] - y[:, :, 1]) / (2.0 * np.float64(np.float32(sigma)))
    bound = 2.0 ** -22 * (np.abs(x.numpy().astype(np.float64))[:, None, :] / sigma + np.abs(z))
    ratio = (np.abs(got - z) / bound).max()
    print(f'   sigma {sigma}: worst |(y+ - y-) / (2 sigma) - ga_randn| / bound = {ratio:.3f}')
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the attack
CFG = {'initial_channels': 8, 'num_pre-post_process_blocks': 1, 'num_pre-post_process_cells': 2, 'num_scales': 3,
       'num_groups_per_scale': 2, 'is_adaptive': False, 'min_groups_per_scale': 1, 'num_cells_per_group': 1,
       'num_latent_per_group': 4, 'num_logistic_mixtures': 10, 'num_nf_cells': None}
RES = (3, 64, 64)
EOT, IMAGES, PAIRS = 2, 2, 4


@pytest.fixture(scope='module')
def nvae(tmp_path_factory):
    """the reduced NVAE + VGG defender of tests/test_noise_gpu.py (input noise eps 2.0) at EoT 2, with seeded draws"""
    d = tmp_path_factory.mktemp('nes_ckpt')
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
    yield args, model, x
    model.model.seeded_noise(None)


class _Recorder:
    """`net` with every call's input, output and grad mode kept"""

    def __init__(self, net):
        self.net, self.model, self.eot_steps, self.calls = net, net.model, net.eot_steps, []

    def __call__(self, x):
        out = self.net(x)
        self.calls.append((x.clone(), out.clone(), torch.is_grad_enabled()))
        return out


def _attack(**kw):
    return A.NESAttack(**{**dict(norm='Linf', eps=8.0 / 255.0, step_size=2.0 / 255.0, steps=2, pairs=PAIRS, sigma=1e-3, seed=9), **kw})


def _labels(model, x):
    model.model.seeded_noise(7)
    with torch.no_grad():
        return model(x).argmax(dim=1)


def test_device_queries_are_the_numpy_backends(nvae):
    """every query batch of a device run, replayed by the numpy backend from the x_adv the run itself checked"""
    args, model, x = nvae
    y = _labels(model, x)
    owner = model.model
    before = set(owner._engines)
    attack, net = _attack(), _Recorder(model)
    attack.image_index = torch.tensor([5, 2])
    owner.seeded_noise(7)
    success, bound, adv = attack(x, y, net)
    torch.cuda.synchronize()
    owner.seeded_noise(None)
    assert all(not grad_on for _, _, grad_on in net.calls)                            # queries under no_grad
    made = set(owner._engines) - before
    assert all(k[-1] == 'forward_only' for k in made) and all(k[-1] == 'forward_only' for k in owner._engines if k[0] > IMAGES * EOT)
    assert attack.queries == sum(c[0].shape[0] for c in net.calls)
    act, calls, replayed, worst = torch.arange(IMAGES), list(net.calls), 0, 0.0
    for t in range(attack.steps + 1):
        xa, logits, _ = calls.pop(0)                                                  # the check of x_adv[act]
        assert xa.shape[0] == act.numel()
        keep = (logits.argmax(dim=1) == y[act.to(DEV)]).cpu()
        act, xa = act[keep], xa[keep.to(DEV)]
        if act.numel() == 0 or t == attack.steps:
            break
        q, _, _ = calls.pop(0)                                                        # query_images None: one call per estimate
        rows = [int(attack.image_index[b]) * PAIRS for b in act]
        x64 = xa.flatten(1).cpu()
        ref = R.reference_perturb(x64.numpy(), PAIRS, 9, t, image_row=rows, sigma=1e-3, lo=0.0, hi=1.0)
        cpu = A.perturb(x64.double(), PAIRS, 9, t, rows, 1e-3)                        # the CPU backend itself
        assert np.array_equal(cpu.numpy(), ref)
        z = R.directions(act.numel(), x64.shape[1], PAIRS, 9, t, image_row=rows)
        ratio = (np.abs(q.flatten(1).cpu().numpy().astype(np.float64) - ref) / _perturb_bound(x64, z, PAIRS, 1e-3)).max()
        worst, replayed = max(worst, ratio), replayed + 1
        assert ratio <= 1.0, (t, ratio)
    assert not calls
    print(f'   {replayed} query batches replayed, worst |query - numpy| / bound = {worst:.3f}; success {success.tolist()}')
    assert replayed >= 1, 'the defender misclassified every clean image: nothing was queried'
    assert (adv >= 0).all() and (adv <= 1).all() and ((adv - x).abs().amax() <= 8.0 / 255.0 + 1e-7)


def test_the_same_seed_twice_gives_the_same_attack(nvae):
    args, model, x = nvae
    y = _labels(model, x)
    out = []
    for _ in range(2):
        model.model.seeded_noise(7)
        out.append(_attack(steps=3, query_images=1, random_start=True)(x, y, model))
    model.model.seeded_noise(None)
    for a, b in zip(*out):
        assert torch.equal(a, b)
    model.model.seeded_noise(7)
    one = _attack(steps=3, query_images=1)(x[:1], y[:1], model)
    model.model.seeded_noise(None)
    assert isinstance(one[0], bool) and isinstance(one[1], float)


def test_the_seeded_driver_writes_the_nes_column_and_repeats_itself(nvae, tmp_path):
    """--attack nes through experiments/seeded_defense.run_worker on 2 synthetic images"""
    from gen_adversarial_amd.experiments import seeded_defense as S
    from gen_adversarial_amd.experiments import test_defense as drv
    args, model, _ = nvae
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli = S.parse_args(['--noise_seed', '3', '--synthetic', '2', '--eot_steps', str(EOT), '--defense_type', 'ours', '--experiment', 'ids',
                            '--config', args.config, '--attack', 'nes', '--batch_images', '2'])
    finally:
        os.chdir(cwd)
    assert cli.attack == 'nes' and S.RESULT_KEYS['nes'] == 'NES'
    assert isinstance(args.nes, A.NESAttack) and args.nes.norm == 'Linf' and args.nes.eps == 8.0 / 255.0 and args.nes.step_size == 2.0 / 255.0
    data = drv.synthetic_dataset(2, 64, 100)
    seen = []

    class Spy(A.NESAttack):
        def __call__(self, image, gt_label, net):
            seen.append(self.image_index.tolist())
            return super().__call__(image, gt_label, net)

    def run(name, seed, bi):
        nes = Spy(eps=8.0 / 255.0, step_size=2.0 / 255.0, steps=2, pairs=PAIRS, seed=1)
        a = Namespace(device=DEV, noise_seed=seed, batch_images=bi, schedule='static', attacks={'nes': nes}, results_folder=str(tmp_path))
        path = str(tmp_path / f'{name}.json')
        res = S.run_worker(0, 1, a, lambda a_: (a_, model), data, results_path=path)
        assert 'NES' in res and len(res['NES']) == 2 and 'Clean' in res
        return open(path).read()
    first = run('a', 3, 2)
    assert seen == [[0, 1]]
    assert run('b', 3, 2) == first
    run('c', 3, 1)
    assert seen[2:] == [[0], [1]]                                                     # dataset indices, image by image
    assert model.model._noise_seed is None
