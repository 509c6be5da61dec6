"""CPU: the NES attack's contract (include/ga_ops.h, ga_nes_perturb / ga_nes_grad) as gen_adversarial_amd/attacks/nes_ref.py restates it
on top of noise.reference_randn, the entry points' declarations and argument checks (which return before anything touches a GPU),
the estimator on a linear loss, and NESAttack on a float64 toy classifier through the numpy backend."""
import ctypes as C

import numpy as np
import pytest
import torch

from gen_adversarial_amd import _lib as L
from gen_adversarial_amd import noise as N
from gen_adversarial_amd.attacks import nes_ref as R
from gen_adversarial_amd.attacks.nes import NESAttack, margin_loss

V = C.c_void_p
P_ARGS = ['x', 'y', 'images', 'inner', 'pairs', 'seed', 'draw', 'tensor', 'row0', 'image_row', 'sigma', 'lo', 'hi', 'stream']
G_ARGS = ['c', 'g', 'images', 'inner', 'pairs', 'seed', 'draw', 'tensor', 'row0', 'image_row', 'scale', 'stream']


def test_entry_points_are_declared_exported_and_bound():
    assert 'ga_nes_perturb' in L.EXPORTS and 'ga_nes_grad' in L.EXPORTS
    p, g = L.lib.ga_nes_perturb, L.lib.ga_nes_grad
    assert p.restype is C.c_int and g.restype is C.c_int
    assert p.argtypes == [V, V, C.c_long, C.c_long, C.c_long, C.c_ulong, C.c_uint, C.c_uint, C.c_ulong, V, C.c_float, C.c_float, C.c_float, V]
    assert g.argtypes == [V, V, C.c_long, C.c_long, C.c_long, C.c_ulong, C.c_uint, C.c_uint, C.c_ulong, V, C.c_float, V]
    assert C.sizeof(L.Op) == L.lib.ga_sizeof_op() == 288 and len(L._H.ops) == 30 and L.ABI_VERSION == 8       # no plan op, no new ABI
    assert N.STREAM_NES == L.GA_RANDN_STREAM_NES == (1 << 31) + 1 != N.STREAM_INPUT


def _perturb(**kw):
    a = dict(x=4096, y=8192, images=2, inner=8, pairs=3, seed=1, draw=0, tensor=N.STREAM_NES, row0=0, image_row=None, sigma=0.1, lo=0.0,
             hi=1.0, stream=None)           # well-formed (never launched: every case below is refused)
    a.update(kw)
    return L.lib.ga_nes_perturb(*(a[k] for k in P_ARGS))


def _grad(**kw):
    a = dict(c=4096, g=8192, images=2, inner=8, pairs=3, seed=1, draw=0, tensor=N.STREAM_NES, row0=0, image_row=None, scale=1.0, stream=None)
    a.update(kw)
    return L.lib.ga_nes_grad(*(a[k] for k in G_ARGS))


COMMON = [
    (dict(images=0), 'GA_E_BADARG'),
    (dict(images=-1), 'GA_E_BADARG'),
    (dict(inner=0), 'GA_E_BADARG'),
    (dict(pairs=0), 'GA_E_BADARG'),
    (dict(pairs=-2), 'GA_E_BADARG'),
    (dict(row0=(1 << 32) - 5), 'GA_E_BADARG'),                        # row0 + images * pairs = 2^32 + 1
    (dict(row0=1 << 63), 'GA_E_BADARG'),
    (dict(pairs=1 << 32), 'GA_E_BADARG'),                             # images * pairs = 2^33
    (dict(inner=6), 'GA_E_UNSUPPORTED'),                              # inner % 4 != 0
]


@pytest.mark.parametrize('kw, code', COMMON + [
    (dict(x=None), 'GA_E_BADARG'),
    (dict(y=None), 'GA_E_BADARG'),
    (dict(x=4100), 'GA_E_ALIGN'),                                     # 16-byte loads
    (dict(y=8200), 'GA_E_ALIGN'),                                     # 16-byte stores
])
def test_perturb_rejects_bad_arguments_without_a_gpu(kw, code):
    assert _perturb(**kw) == getattr(L, code) < 0


@pytest.mark.parametrize('kw, code', COMMON + [
    (dict(c=None), 'GA_E_BADARG'),
    (dict(g=None), 'GA_E_BADARG'),
    (dict(g=8200), 'GA_E_ALIGN'),
])
def test_grad_rejects_bad_arguments_without_a_gpu(kw, code):
    assert _grad(**kw) == getattr(L, code) < 0


# ---------------------------------------------------------------------------------------------------------------- the restatement
SEED, DRAW = 0xDEADBEEF00000001, 7


def test_perturb_rows_are_x_plus_minus_sigma_z_clamped():
    images, inner, pairs, sigma, row0 = 3, 12, 5, 0.25, 40
    x = np.random.default_rng(0).random((images, inner))
    free = R.reference_perturb(x, pairs, SEED, DRAW, row0=row0, sigma=sigma)                     # lo > hi: no clamp
    clamped = R.reference_perturb(x, pairs, SEED, DRAW, row0=row0, sigma=sigma, lo=0.0, hi=1.0)
    assert free.shape == clamped.shape == (images * pairs * 2, inner) and free.dtype == np.float64
    assert free.min() < 0.0 and free.max() > 1.0                                                  # the clamp has something to do
    for b in range(images):
        z = N.reference_randn(SEED, DRAW, N.STREAM_NES, row0 + b * pairs, pairs, inner)
        for i in range(pairs):
            for s, sign in ((0, 1.0), (1, -1.0)):
                want = x[b] + sign * sigma * z[i]
                row = (b * pairs + i) * 2 + s
                assert np.array_equal(free[row], want) and np.array_equal(clamped[row], np.clip(want, 0.0, 1.0))
    other = R.reference_perturb(x, pairs, SEED, DRAW, tensor=N.STREAM_INPUT, row0=row0, sigma=sigma)
    assert not np.array_equal(other, free)


def test_grad_is_the_explicit_float64_sum():
    images, inner, pairs, row0 = 3, 12, 5, 40
    c = np.random.default_rng(1).standard_normal(images * pairs)
    g = R.reference_grad(c, images, inner, pairs, SEED, DRAW, row0=row0, scale=0.5)
    assert g.shape == (images, inner) and g.dtype == np.float64
    for b in range(images):
        z = N.reference_randn(SEED, DRAW, N.STREAM_NES, row0 + b * pairs, pairs, inner)
        want = np.zeros(inner)
        for i in range(pairs):
            want += c[b * pairs + i] * z[i]
        assert np.abs(g[b] - 0.5 * want).max() <= 1e-14 * np.abs(want).max()
    swapped = R.reference_grad(c.reshape(images, pairs)[::-1].ravel(), images, inner, pairs, SEED, DRAW, row0=row0, scale=0.5)
    assert np.abs(swapped - g).max() > 0.1                                                        # c belongs to its image


def test_image_row_against_the_row0_default():
    images, inner, pairs, row0 = 3, 8, 4, 17
    x = np.random.default_rng(2).random((images, inner))
    c = np.random.default_rng(3).standard_normal(images * pairs)
    rows = [row0 + b * pairs for b in range(images)]
    assert np.array_equal(R.reference_perturb(x, pairs, 5, 1, row0=row0), R.reference_perturb(x, pairs, 5, 1, image_row=rows))
    assert np.array_equal(R.reference_grad(c, images, inner, pairs, 5, 1, row0=row0), R.reference_grad(c, images, inner, pairs, 5, 1, image_row=rows))
    # an image keeps its rows wherever it stands in the call
    far = [900, 17, 5000]
    y3 = R.reference_perturb(x, pairs, 5, 1, image_row=far).reshape(images, pairs * 2, inner)
    y1 = R.reference_perturb(x[1:2], pairs, 5, 1, image_row=far[1:2])
    assert np.array_equal(y3[1], y1) and np.array_equal(y1, R.reference_perturb(x[1:2], pairs, 5, 1, row0=17))
    for bad in (dict(image_row=[0, 1]), dict(image_row=[0, 4, (1 << 32) - 3]), dict(row0=(1 << 32) - 11)):
        with pytest.raises(ValueError):
            R.reference_perturb(x, pairs, 5, 1, **bad)
    assert R.reference_perturb(x, pairs, 5, 1, row0=(1 << 32) - 12).shape == (24, inner)


def test_estimator_points_along_the_gradient_of_a_linear_loss():
    """L(x) = w.x: the loss differences are exactly 2 sigma w.z_i, so g = (1/n) sum_i (w.z_i) z_i, whose cosine with w is about
    sqrt(n / (n + d + 1)) = sqrt(256 / 305) = 0.916 for n = 256 directions in d = 48 dimensions.
    Observed at seed 0, draw 0: cos = 0.9204 (1.005 of the expectation); asserted: >= 0.75 of the expectation."""
    inner, pairs, sigma = 48, 256, 1e-3
    w = np.random.default_rng(0).standard_normal(inner)
    x = np.full((1, inner), 0.5)
    y = R.reference_perturb(x, pairs, 0, 0, sigma=sigma)
    loss = y @ w
    c = loss[0::2] - loss[1::2]
    g = R.reference_grad(c, 1, inner, pairs, 0, 0, scale=1.0 / (2.0 * sigma * pairs))[0]
    cos = float(g @ w / np.linalg.norm(g) / np.linalg.norm(w))
    expect = np.sqrt(pairs / (pairs + inner + 1.0))
    print(f'   cos(g, w) = {cos:.4f}, expectation {expect:.4f}, ratio {cos / expect:.3f}')
    assert cos >= 0.75 * expect


# ---------------------------------------------------------------------------------------------------------------- the attack
CLASSES, RES = 4, (3, 4, 4)


class _Linear:
    """a float64 linear classifier on 3 x 4 x 4 images that records its query batches"""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.w = torch.randn(CLASSES, 48, generator=g, dtype=torch.float64)
        self.seen, self.grad_modes = [], []

    def logits(self, x):
        return x.flatten(1) @ self.w.t()

    def __call__(self, x):
        self.seen.append(x.clone())
        self.grad_modes.append(torch.is_grad_enabled())
        return self.logits(x)


def _images(n=3):
    x = 0.25 + 0.5 * torch.rand(n, *RES, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    return x, _Linear().logits(x).argmax(dim=1)


# eps: the margins of the three images are a few tenths and |w| is of order 1 per pixel, so a step of 0.05 per pixel along sign(g)
# moves a logit difference by about 0.05 * 48 * E|w1 - w2| > 2: 0.1 (Linf) and 0.1 * sqrt(48) / 2 = 0.35 (L2) cross every boundary
@pytest.mark.parametrize('norm, eps, step', [('Linf', 0.1, 0.025), ('L2', 0.35, 0.1)])
def test_attack_on_a_toy_classifier(norm, eps, step):
    x, y = _images()
    kw = dict(norm=norm, eps=eps, step_size=step, steps=12, pairs=16, sigma=1e-3, seed=5)
    index = torch.tensor([6, 2, 11])

    def run(xs, ys, idx, **over):
        a, net = NESAttack(**{**kw, **over}), _Linear()
        a.image_index = idx
        return a(xs, ys, net), net

    (succ, bound, adv), net = run(x, y, index)
    assert net.grad_modes and not any(net.grad_modes)                            # every query under no_grad
    assert (net.logits(x).argmax(dim=1) == y).all()                              # clean images are classified correctly
    assert succ.dtype == torch.bool and succ.all() and adv.dtype == torch.float64
    assert (adv >= 0.0).all() and (adv <= 1.0).all()
    d = (adv - x).flatten(1)
    size = d.abs().amax(dim=1) if norm == 'Linf' else d.norm(dim=1)
    assert (size <= eps + 1e-12).all() and torch.equal(size, bound) and (bound > 0).all()
    assert (net.logits(adv).argmax(dim=1) != y).all()
    # each image equals its own one-image run at the same index: B = 1 returns Python scalars
    for b in range(3):
        (s1, b1, a1), _ = run(x[b:b + 1], y[b:b + 1], index[b:b + 1])
        assert isinstance(s1, bool) and isinstance(b1, float)
        assert s1 == bool(succ[b]) and abs(b1 - float(bound[b])) <= 1e-12 and (a1[0] - adv[b]).abs().max() <= 1e-12
    # other chunking of the queries: the same attack
    (s2, b2, a2), net2 = run(x, y, index, query_images=1)
    assert torch.equal(s2, succ) and (a2 - adv).abs().max() <= 1e-12 and len(net2.seen) > len(net.seen)
    # the same seed twice: identical; another seed: other queries
    (s3, b3, a3), net3 = run(x, y, index)
    assert torch.equal(s3, succ) and torch.equal(b3, bound) and torch.equal(a3, adv)
    assert len(net3.seen) == len(net.seen) and all(torch.equal(p, q) for p, q in zip(net3.seen, net.seen))
    _, net4 = run(x, y, index, seed=6)
    assert net4.seen[1].shape == net.seen[1].shape and not torch.equal(net4.seen[1], net.seen[1])
    # the first estimate's queries are the restatement's, at draw 0 and rows index * pairs
    want = R.reference_perturb(x.flatten(1).numpy(), 16, 5, 0, image_row=[16 * int(i) for i in index], sigma=1e-3, lo=0.0, hi=1.0)
    assert np.array_equal(net.seen[1].flatten(1).numpy(), want)
    # default index: arange(B)
    a = NESAttack(**kw)
    net5 = _Linear()
    a(x, y, net5)
    want0 = R.reference_perturb(x.flatten(1).numpy(), 16, 5, 0, row0=0, sigma=1e-3, lo=0.0, hi=1.0)
    assert np.array_equal(net5.seen[1].flatten(1).numpy(), want0) and a.queries == sum(s.shape[0] for s in net5.seen)


def test_random_start_and_ce_loss_stay_inside_the_ball():
    x, y = _images()
    for norm, eps in (('Linf', 0.05), ('L2', 0.2)):
        a, net = NESAttack(norm=norm, eps=eps, step_size=eps / 4, steps=3, pairs=8, loss='ce', seed=1, random_start=True), _Linear()
        succ, bound, adv = a(x, y, net)
        start = net.seen[0]
        d = (start - x).flatten(1)
        size = d.abs().amax(dim=1) if norm == 'Linf' else d.norm(dim=1)
        assert (size > 0).all() and (size <= eps + 1e-12).all() and (bound <= eps + 1e-12).all()
        # sample 0 of every image (rows b * pairs) at the start's own draw: uniform in the cube, or a uniform direction on the sphere
        z = torch.from_numpy(np.stack([N.reference_randn(1, 0xFFFFFFFF, N.STREAM_NES, b * 8, 1, 48)[0] for b in range(3)]))
        want = eps * torch.erf(z / 2.0 ** 0.5) if norm == 'Linf' else eps * z / z.norm(dim=1, keepdim=True)
        assert (d - want).abs().max() <= 1e-12              # x in [0.25, 0.75]: the clamp to [0, 1] has nothing to do
        if norm == 'Linf':
            assert (d.abs() < 0.9 * eps).float().mean() > 0.8          # inside the cube, not on its faces
        a2, net2 = NESAttack(norm=norm, eps=eps, step_size=eps / 4, steps=3, pairs=8, loss='ce', seed=1, random_start=True), _Linear()
        a2(x, y, net2)
        assert torch.equal(net2.seen[0], start)
    with pytest.raises(ValueError):
        NESAttack(norm='L1')
    with pytest.raises(ValueError):
        a = NESAttack()
        a.image_index = torch.tensor([0])
        a(x, y, _Linear())


def test_margin_loss():
    z = torch.tensor([[1.0, 3.0, 2.0], [5.0, 0.0, 1.0]])
    assert margin_loss(z, torch.tensor([1, 1])).tolist() == [-1.0, 5.0]


def test_the_seeded_driver_owns_the_nes_choice(tmp_path, monkeypatch):
    """--attack nes is parsed by experiments/seeded_defense.py itself (test_defense's parser never sees it), which also names the column"""
    from gen_adversarial_amd.experiments import seeded_defense as S
    from gen_adversarial_amd.experiments import test_defense as drv
    monkeypatch.chdir(tmp_path)                                   # parse_args creates ./results/<config>/
    base = ['--noise_seed', '3', '--config', 'x/cfg.yaml', '--experiment', 'ids']
    assert S.parse_args(base + ['--attack', 'nes']).attack == 'nes'
    assert S.parse_args(base + ['--attack', 'pgd']).attack == 'pgd' and S.parse_args(base).attack is None
    with pytest.raises(SystemExit):
        S.parse_args(base + ['--attack', 'no-such-attack'])
    assert S.RESULT_KEYS['nes'] == 'NES' and S.RESULT_KEYS['pgd'] == drv.RESULT_KEYS['pgd']
