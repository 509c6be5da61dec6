"""CPU: Square Attack's contract (include/ga_ops.h, ga_square_linf / ga_square_l2) as gen_adversarial_amd/attacks/square_ref.py restates
it, the entry points' declarations and argument checks (which return before anything touches a GPU), the schedules, SquareAttack on
a float64 toy classifier through the numpy backend, and AutoAttack with and without its Square stage."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from gen_adversarial_amd import _lib as L
from gen_adversarial_amd import noise as N
from gen_adversarial_amd.attacks import square_ref as R
from gen_adversarial_amd.attacks.l2_attacks import AutoAttack
from gen_adversarial_amd.attacks.square import SquareAttack, propose

V = C.c_void_p
LINF_ARGS = ['x_orig', 'x_adv', 'y', 'images', 'C', 'H', 'W', 's', 'seed', 'draw', 'tensor', 'row0', 'image_row', 'eps', 'lo', 'hi', 'stream']
L2_ARGS = LINF_ARGS[:3] + ['eta'] + LINF_ARGS[3:]
SEED, DRAW = 0xDEADBEEF00000001, 7


def test_entry_points_are_declared_exported_and_bound():
    assert 'ga_square_linf' in L.EXPORTS and 'ga_square_l2' in L.EXPORTS
    a, b = L.lib.ga_square_linf, L.lib.ga_square_l2
    tail = [C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulong, C.c_uint, C.c_uint, C.c_ulong, V, C.c_float, C.c_float, C.c_float, V]
    assert a.restype is C.c_int and b.restype is C.c_int
    assert a.argtypes == [V, V, V] + tail and b.argtypes == [V, V, V, V] + tail
    assert C.sizeof(L.Op) == L.lib.ga_sizeof_op() == 288 and len(L._H.ops) == 30 and L.ABI_VERSION == 8       # no plan op, no new ABI
    assert N.STREAM_SQUARE == L.GA_RANDN_STREAM_SQUARE == (1 << 31) + 2 and len({N.STREAM_SQUARE, N.STREAM_NES, N.STREAM_INPUT}) == 3


def _call(fn, names, **kw):
    a = dict(x_orig=4096, x_adv=8192, y=12288, eta=16384, images=2, C=3, H=8, W=8, s=3, seed=1, draw=0, tensor=N.STREAM_SQUARE, row0=0,
             image_row=None, eps=0.5, lo=0.0, hi=1.0, stream=None)          # well-formed (never launched: every case below is refused)
    a.update(kw)
    return fn(*(a[k] for k in names))


BAD = [
    (dict(images=0), 'GA_E_BADARG'),
    (dict(images=-1), 'GA_E_BADARG'),
    (dict(C=0), 'GA_E_BADARG'),
    (dict(H=0), 'GA_E_BADARG'),
    (dict(W=-3), 'GA_E_BADARG'),
    (dict(s=0), 'GA_E_BADARG'),
    (dict(s=9), 'GA_E_BADARG'),                                       # s > min(H, W)
    (dict(H=6, W=10, s=7), 'GA_E_BADARG'),
    (dict(row0=(1 << 32) - 1), 'GA_E_BADARG'),                        # row0 + images = 2^32 + 1
    (dict(row0=1 << 63), 'GA_E_BADARG'),
    (dict(C=33), 'GA_E_UNSUPPORTED'),                                 # one sign bit per channel
    (dict(C=32, H=8192, W=8192, s=3), 'GA_E_UNSUPPORTED'),            # C H W = 2^31
    (dict(x_orig=None), 'GA_E_BADARG'),
    (dict(x_adv=None), 'GA_E_BADARG'),
    (dict(y=None), 'GA_E_BADARG'),
]


@pytest.mark.parametrize('kw, code', BAD)
def test_linf_rejects_bad_arguments_without_a_gpu(kw, code):
    assert _call(L.lib.ga_square_linf, LINF_ARGS, **kw) == getattr(L, code) < 0


@pytest.mark.parametrize('kw, code', BAD + [(dict(eta=None), 'GA_E_BADARG')])
def test_l2_rejects_bad_arguments_without_a_gpu(kw, code):
    assert _call(L.lib.ga_square_l2, L2_ARGS, **kw) == getattr(L, code) < 0


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _pair(images, C, H, W, eps, seed=0, dtype=np.float32):
    """(x_orig, x_adv) with |x_adv - x_orig| <= eps elementwise and L2 norm <= eps per image, inside [0, 1]"""
    g = np.random.default_rng(seed)
    x = g.random((images, C, H, W))
    d = g.uniform(-1.0, 1.0, size=x.shape)
    d *= eps * 0.9 / np.sqrt((d ** 2).sum(axis=(1, 2, 3), keepdims=True))
    return x.astype(dtype), np.clip(x + d, 0.0, 1.0).astype(dtype)


@pytest.mark.parametrize('H, W', [(8, 8), (6, 10), (5, 7)])
def test_windows_stay_inside_the_image(H, W):
    for s in (1, 2, min(H, W)):
        rows = [0, 17, (1 << 32) - 1, 5000] + list(range(100, 164))
        for draw in (0, 1, 0xFFFFFFFE):
            w = R.windows(len(rows), H, W, s, SEED, draw, image_row=rows)
            for k, n in (('h1', H), ('w1', W), ('h2', H), ('w2', W)):
                assert w[k].min() >= 0 and (w[k] + s).max() <= n
            if s == min(H, W) and H <= W:
                assert (w['h1'] == 0).all() and (w['h2'] == 0).all()
            if s == 1:
                assert len(set(zip(w['h1'].tolist(), w['w1'].tolist()))) > len(rows) // 3           # the positions do vary
    a = R.windows(3, H, W, 2, SEED, 4, image_row=[9, 3, 6])
    for b, r in enumerate([9, 3, 6]):                                                               # an image keeps its choices anywhere
        one = R.windows(1, H, W, 2, SEED, 4, row0=r)
        assert all(a[k][b] == one[k][0] for k in a)
    with pytest.raises(ValueError):
        R.windows(1, H, W, min(H, W) + 1, SEED, 0)
    with pytest.raises(ValueError):
        R.windows(1, H, W, 2, SEED, 0, row0=1 << 32)


def test_pos_is_the_high_word_of_the_product():
    """window positions spelled out from the raw words: (word * n) >> 32"""
    H, W, s = 9, 13, 4
    w = R.windows(2, H, W, s, SEED, DRAW, row0=40)
    for b in range(2):
        words = [N.philox4x32_10(np.array([c0, 40 + b, N.STREAM_SQUARE, DRAW]), (SEED & 0xFFFFFFFF, SEED >> 32)) for c0 in (0, 1)]
        assert int(w['h1'][b]) == (int(words[0][0]) * (H - s + 1)) >> 32 and int(w['w1'][b]) == (int(words[0][1]) * (W - s + 1)) >> 32
        assert int(w['h2'][b]) == (int(words[1][0]) * (H - s + 1)) >> 32 and int(w['w2'][b]) == (int(words[1][1]) * (W - s + 1)) >> 32
        assert int(w['signs'][b]) == int(words[0][2]) and bool(w['transposed'][b]) == bool(int(words[0][3]) & 1)


@pytest.mark.parametrize('H, W, s', [(8, 8, 1), (8, 8, 3), (8, 8, 8), (6, 10, 5), (5, 7, 2)])
def test_linf_proposal_changes_one_window_and_stays_in_the_cube(H, W, s):
    eps = 0.05
    x, xa = _pair(3, 3, H, W, eps)
    rows = [11, 4, 900]
    y = R.reference_linf(x, xa, s, SEED, DRAW, image_row=rows, eps=eps)
    assert y.dtype == np.float32 and y.shape == x.shape
    win = R.windows(3, H, W, s, SEED, DRAW, image_row=rows)
    for b in range(3):
        h, w = int(win['h1'][b]), int(win['w1'][b])
        mask = np.zeros((H, W), dtype=bool)
        mask[h:h + s, w:w + s] = True
        assert np.array_equal(y[b][:, ~mask], xa[b][:, ~mask])
        for ch in range(3):
            sg = np.float32(eps) if (int(win['signs'][b]) >> ch) & 1 else -np.float32(eps)
            assert np.array_equal(y[b, ch][mask], np.clip(x[b, ch][mask] + sg, np.float32(0), np.float32(1)))
    assert y.min() >= 0.0 and y.max() <= 1.0 and np.abs(y.astype(np.float64) - x).max() <= eps * (1 + 1e-6)


@pytest.mark.parametrize('H, W, s', [(8, 8, 3), (8, 8, 7), (6, 10, 5), (16, 16, 5)])
def test_l2_proposal_stays_in_the_ball(H, W, s):
    eps = 0.5
    x, xa = _pair(4, 3, H, W, eps, seed=1)
    xa[3] = x[3]                                                       # an image that has not moved yet
    parts = []
    y = R.reference_l2(x, xa, R.eta(s), SEED, DRAW, row0=5, eps=eps, parts=parts)
    assert y.dtype == np.float64 and y.min() >= 0.0 and y.max() <= 1.0
    n = np.sqrt(((y - x) ** 2).sum(axis=(1, 2, 3)))
    assert (n <= eps * (1 + 1e-6)).all() and (n > 0.5 * eps).all()
    for b, p in enumerate(parts):
        outside = ~p['union']
        assert np.array_equal(p['d2'][:, outside], p['d'][:, outside]) and abs(p['n_d2'] - eps) <= 1e-9 * eps      # the whole budget is spent
        only2 = p['union'].copy()
        only2[p['h1']:p['h1'] + s, p['w1']:p['w1'] + s] = False
        assert (p['d2'][:, only2] == 0).all()                          # window 2 is emptied, window 1 wins where they overlap
        # every channel of window 1 gets the norm the formula gives it
        got = np.sqrt((p['d2'][:, p['h1']:p['h1'] + s, p['w1']:p['w1'] + s] ** 2).sum(axis=(1, 2)))
        assert np.allclose(got, p['target'], rtol=1e-9, atol=1e-15)
        one = R.reference_l2(x[b:b + 1], xa[b:b + 1], R.eta(s), SEED, DRAW, row0=5 + b, eps=eps)
        assert np.array_equal(one[0], y[b])                            # an image alone: the same bits


@pytest.mark.parametrize('s', [2, 3, 5, 7, 8, 21, 63])
def test_eta_has_unit_norm_and_antisymmetric_halves(s):
    e = R.eta(s)
    assert e.dtype == np.float32 and e.shape == (s, s)
    assert abs(np.sqrt((e.astype(np.float64) ** 2).sum()) - 1.0) <= 1e-6
    assert (e[:s // 2] > 0).all() and (e[s // 2:] < 0).all()
    if s % 2 == 0:
        assert np.array_equal(e[:s // 2], -e[s // 2:])
    if s % 2:
        assert np.array_equal(e, e[:, ::-1])                           # odd sides (all the L2 schedule uses): left-right symmetric


def test_side_and_p_schedule_at_their_break_points():
    assert [R.p_schedule(0.8, it, 10000) for it in (0, 10, 11, 50, 51, 200, 201, 500, 501, 1000, 1001, 2000, 2001, 4000, 4001, 6000, 6001,
                                                     8000, 8001, 9999)] == \
        [0.8, 0.8, 0.4, 0.4, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05, 0.025, 0.025, 0.0125, 0.0125, 0.00625, 0.00625, 0.003125, 0.003125, 0.0015625,
         0.0015625]
    assert R.p_schedule(0.8, 5, 5000) == 0.8 and R.p_schedule(0.8, 6, 5000) == 0.4 and R.p_schedule(0.8, 4001, 5000) == 0.8 / 512
    assert R.side(0.8, 64, 64, 'Linf') == 57 and R.side(1.0, 64, 64, 'Linf') == 64 and R.side(1e-6, 64, 64, 'Linf') == 1
    assert R.side(1.0, 6, 10, 'Linf') == 6                                                  # never wider than the image
    assert R.side(0.8, 64, 64, 'L2') == 57 and R.side(1.0, 64, 64, 'L2') == 63 and R.side(1e-6, 64, 64, 'L2') == 3
    assert R.side(0.0625, 64, 64, 'L2') == 17                                               # 16 made odd
    assert R.side(1.0, 8, 8, 'L2') == 7 and R.side(1.0, 6, 10, 'L2') == 5 and R.side(1.0, 4, 4, 'L2') == 3
    with pytest.raises(ValueError):
        R.side(0.5, 3, 3, 'L2')


# ---------------------------------------------------------------------------------------------------------------- the attack
CLASSES, RES = 4, (3, 8, 8)


class _Linear:
    """a float64 linear classifier on 3 x 8 x 8 images, applied image by image (an image's logits are then bitwise those of a one-image
    call, whatever the host's matrix kernels do for other batch sizes); records its query batches"""

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.w = torch.randn(CLASSES, 192, generator=g, dtype=torch.float64)
        self.seen, self.grad_modes = [], []

    def logits(self, x):
        return torch.stack([self.w @ xi.flatten() for xi in x])

    def __call__(self, x):
        self.seen.append(x.clone())
        self.grad_modes.append(torch.is_grad_enabled())
        return self.logits(x)


def _images(n=4):
    x = 0.25 + 0.5 * torch.rand(n, *RES, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    return x, _Linear().logits(x).argmax(dim=1)


# eps: the margins of the clean images are 12 to 16 and |w| is of order 1 per pixel; 0.2 per pixel along the right signs moves a logit
# difference by 0.2 * 192 * E|w1 - w2| = 43, and an L2 budget of 3 (0.22 per pixel on average, inside [0, 1] for x in [0.25, 0.75])
# about as far: a random search that keeps improvements gets there well inside 300 queries
@pytest.mark.parametrize('norm, eps', [('Linf', 0.2), ('L2', 3.0)])
def test_attack_on_a_toy_classifier(norm, eps):
    x, y = _images()
    kw = dict(norm=norm, eps=eps, n_queries=300, p_init=0.3, seed=5)
    index = torch.tensor([6, 2, 11, 40])

    def run(xs, ys, idx, **over):
        a, net = SquareAttack(**{**kw, **over}), _Linear()
        a.image_index = idx
        return a(xs, ys, net), net, a

    (succ, bound, adv), net, atk = run(x, y, index)
    assert net.grad_modes and not any(net.grad_modes)                            # every query under no_grad
    assert (net.logits(x).argmax(dim=1) == y).all()                              # clean images are classified correctly
    assert succ.dtype == torch.bool and succ.all() and adv.dtype == torch.float64
    assert (adv >= 0.0).all() and (adv <= 1.0).all()
    d = (adv - x).flatten(1)
    size = d.abs().amax(dim=1) if norm == 'Linf' else d.norm(dim=1)
    assert (size <= eps * (1 + 1e-9)).all() and torch.equal(size, bound) and (bound > 0).all()
    assert (net.logits(adv).argmax(dim=1) != y).all()
    assert atk.queries == sum(s.shape[0] for s in net.seen) <= 300 * 4
    sizes = [s.shape[0] for s in net.seen]
    assert sizes[0] == 4 and min(sizes) < 4                                      # images finished at different times and left the calls
    # each image is bitwise its own one-image run at the same index: B = 1 returns Python scalars
    for b in range(4):
        (s1, b1, a1), _, _ = run(x[b:b + 1], y[b:b + 1], index[b:b + 1])
        assert isinstance(s1, bool) and isinstance(b1, float)
        assert s1 == bool(succ[b]) and b1 == float(bound[b]) and torch.equal(a1[0], adv[b])
    # the same seed twice: identical; another seed: other proposals
    (s3, b3, a3), net3, _ = run(x, y, index)
    assert torch.equal(s3, succ) and torch.equal(b3, bound) and torch.equal(a3, adv)
    assert len(net3.seen) == len(net.seen) and all(torch.equal(p, q) for p, q in zip(net3.seen, net.seen))
    _, net4, _ = run(x, y, index, seed=6)
    assert not torch.equal(net4.seen[0], net.seen[0])
    # the first proposal is the restatement's, at draw 0 and rows `index`, from the start the attack itself queried
    s0 = atk.side(0, 8, 8)
    start = net.seen[0]
    keep = (net.logits(start).argmax(dim=1) == y).nonzero().flatten()
    rows = [int(index[b]) for b in keep]
    if norm == 'Linf':
        want = R.reference_linf(x[keep].numpy(), start[keep].numpy(), s0, 5, 0, image_row=rows, eps=eps)
    else:
        want = R.reference_l2(x[keep].numpy(), start[keep].numpy(), R.eta(s0), 5, 0, image_row=rows, eps=eps)
    assert np.array_equal(net.seen[1].numpy(), want)
    assert np.array_equal(propose(norm, x[keep], start[keep], s0, 5, 0, rows, eps, torch.from_numpy(R.eta(s0)).double()).numpy(), want)


def test_the_start_is_stripes_or_tiles_of_norm_eps():
    x, y = _images()
    for norm, eps in (('Linf', 0.05), ('L2', 0.4)):
        a, net = SquareAttack(norm=norm, eps=eps, n_queries=1, loss='ce', seed=1), _Linear()
        succ, bound, adv = a(x, y, net)
        assert len(net.seen) == 1 and a.queries == 4
        d = net.seen[0] - x                                            # x in [0.25, 0.75]: the clamp to [0, 1] has nothing to do
        z = np.stack([N.reference_randn(1, 0xFFFFFFFF, N.STREAM_SQUARE, b, 1, 192)[0] for b in range(4)]).reshape(4, 3, 8, 8)
        sign = torch.from_numpy(np.where(z >= 0, 1.0, -1.0))
        if norm == 'Linf':
            assert (d - eps * sign[:, :, :1, :]).abs().max() <= 1e-15
        else:
            assert (d.flatten(1).norm(dim=1) - eps).abs().max() <= 1e-12
            e = torch.from_numpy(R.eta(2)).double()
            tile = d[:, :, 2:4, 4:6]
            want = sign[:, :, 2:3, 4:5] * e
            assert (tile / tile.flatten(2).norm(dim=2)[..., None, None] - want).abs().max() <= 1e-7      # the fp32 table's norm is 1 within 1e-7
    with pytest.raises(ValueError):
        SquareAttack(norm='L1')
    with pytest.raises(ValueError):
        SquareAttack(n_queries=0)
    with pytest.raises(ValueError):
        a = SquareAttack()
        a.image_index = torch.tensor([0])
        a(x, y, _Linear())


def test_the_seeded_driver_owns_the_square_choice(tmp_path, monkeypatch):
    """--attack square is parsed by experiments/seeded_defense.py itself (test_defense's parser never sees it), which also names the column"""
    from gen_adversarial_amd.experiments import seeded_defense as S
    from gen_adversarial_amd.experiments import test_defense as drv
    monkeypatch.chdir(tmp_path)                                   # parse_args creates ./results/<config>/
    base = ['--noise_seed', '3', '--config', 'x/cfg.yaml', '--experiment', 'ids']
    assert S.parse_args(base + ['--attack', 'square']).attack == 'square' and 'square' in S.OWN_ATTACKS
    assert S.parse_args(base + ['--attack', 'nes']).attack == 'nes' and S.parse_args(base + ['--attack', 'pgd']).attack == 'pgd'
    assert S.RESULT_KEYS['square'] == 'SQUARE' and 'square' not in drv.RESULT_KEYS


# ---------------------------------------------------------------------------------------------------------------- AutoAttack
def _toy_net(seed=0, n_classes=6):
    """the toy net of tests/test_attacks_cpu.py (the goldens of tests/golden/attacks_toy.npz were made on it)"""
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.SiLU(), torch.nn.AvgPool2d(2),
                              torch.nn.Conv2d(8, 8, 3, padding=1), torch.nn.SiLU(), torch.nn.Flatten(),
                              torch.nn.Linear(8 * 8 * 8, n_classes))
    return net.eval()


def _short(aa):
    for atk in aa.ce + aa.dlr:
        atk.__init__(n_iter=10, rho=0.75, max_bound=atk.max_bound, ce_loss=not (atk.criterion == atk.dlr_loss))
    aa.fab.n_iter = 6
    return aa


def test_autoattack_default_is_unchanged_and_the_square_stage_is_never_worse():
    gold = load_golden('attacks_toy.npz')
    net = _toy_net()
    images, labels = torch.from_numpy(gold['images']), torch.from_numpy(gold['labels'])
    plain = _short(AutoAttack())
    assert plain.square == []
    torch.manual_seed(321)
    s, b, a = plain(images[:1].clone(), labels[:1].clone(), net)                # the golden of the reference's own AutoAttack
    assert bool(s) == bool(gold['aa_success']) and float(b) == pytest.approx(float(gold['aa_bound']), rel=1e-4)
    np.testing.assert_allclose(a.numpy(), gold['aa_adv'], atol=2e-5)
    torch.manual_seed(321)
    s0, b0, a0 = _short(AutoAttack())(images.clone(), labels.clone(), net)
    torch.manual_seed(321)
    sq = _short(AutoAttack(with_square=True, square_queries=40))
    assert [q.eps for q in sq.square] == [0.5, 1.0, 4.0] and all(q.norm == 'L2' and q.n_queries == 40 for q in sq.square)
    s1, b1, a1 = sq(images.clone(), labels.clone(), net)
    assert sq.square[0].queries > 0                                              # the stage ran
    for i in range(images.shape[0]):
        assert bool(s1[i]) or not bool(s0[i])
        if bool(s0[i]):
            assert float(b1[i]) <= float(b0[i])
        if bool(s1[i]):
            assert net(a1[i:i + 1]).argmax(dim=1).item() != int(labels[i])
