"""
GPU: ga_square_linf / ga_square_l2 (csrc/square.hip) against the restatement of their contract
(gen_adversarial_amd/attacks/square_ref.py), and SquareAttack on a reduced NVAE + VGG defender.

Linf: one fp32 addition and a clamp per rewritten element, a copy elsewhere: the fp32 restatement must give the same bits.

L2 bound (u = 2^-24, first order in u, the total doubled for the products of errors a first-order count drops).  With
T = ceil(H W / 256) and Tw = ceil(s^2 / 256) terms per thread and channel, a sum of the kernel is a per-thread chain, 6 butterfly
levels and 3 additions of the waves' partials, then a chain over the C channels where the formula sums over channels:
  pass-1 sums (n_img^2, n_win^2, n_1^2): longest path L1 = C T + C + 12 additions of non-negative terms, each term d^2 with d one
      subtraction and one product (3u):  relative error k1 = (L1 + 3) u.
  den1 = 1e-12 + sqrt(n_1^2): relative r = k1 / 2 + 2u.        old = d / den1: |old| (r + 2u).
  new = +-eta + old (the sum may cancel, so absolutely):  a_new = |old| (r + 2u) + u |new|.
  norm of new[ch] and its denominator: |a_new[ch]|_2 + |new[ch]| ((Tw + 10) / 2 + 2) u      (triangle inequality + the sum's path).
  spare = max(eps^2 - n_img^2, 0) / C:  (eps^2 u + n_img^2 k1) / C + 2u spare  — absolute, so an image with no spare budget is covered;
  target^2 = spare + n_win^2: that + n_win^2 k1 + u target^2;   target: min(err / target, sqrt(err)) + u target.
  scale = target / den: err(target) / den + target err(den) / den^2 + u scale.     d' = scale new: err(scale) |new| + scale a_new + u |d'|.
  |d'|^2 = (sum outside the union) + (sum over window 1 of d'^2): k1 on the first, 2 |d'| err(d') + (C Tw + 14) u d'^2 on the second;
  f = eps / (1e-12 + |d'|): relative err(|d'|) / |d'| + 3u.
  y = x_orig + d' f:  f err(d') + |d' f| (rel(f) + u) + u |y|;  outside the windows err(d') = u |d|;  the clamp is 1-Lipschitz.
A misread window, sign, image row or orientation moves whole windows by about eps / s: orders of magnitude above this.
Observed on an MI355X (profiles/square_attack_gpu.log): worst |y - ref| / bound 0.456 over the op cases (3 x 64 x 64, s = 63), 0.292 in the
attack-level replay; the misread references stand at 4e5 to 1.5e8 of the bound.
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
from gen_adversarial_amd.attacks import square as A   # noqa: E402
from gen_adversarial_amd.attacks import square_ref as R   # noqa: E402
from gen_adversarial_amd.attacks.nes import _first_rows_device, margin_loss   # noqa: E402
from gen_adversarial_amd.experiments.load_defense import load   # noqa: E402
from gen_adversarial_amd.nvae_spec import build_spec, nvae_checkpoint   # noqa: E402
from gen_adversarial_amd.vgg_spec import init_vgg_state_dict   # noqa: E402

DEV = 'cuda:0'
GUARD = 64                       # floats of a NaN pattern behind every buffer
NAN_BITS = 0x7fc01234
SEED = 0xDEADBEEF00000001
U = 2.0 ** -24
FAR = [900, (1 << 31) + 17, 5000]                 # rows of three images that are no neighbours, one with the high bit set
LINF_SIDES = {(3, 8, 8): [1, 3, 8], (3, 6, 10): [5], (3, 64, 64): [3, 21, 64]}
L2_SIDES = {(3, 8, 8): [3, 7], (3, 6, 10): [5], (3, 64, 64): [3, 21, 63]}
LINF_CASES = [(shape, s, images) for shape, sides in LINF_SIDES.items() for s in sides for images in (1, 3)]
L2_CASES = [(shape, s, images) for shape, sides in L2_SIDES.items() for s in sides for images in (1, 3)]


def _guarded(n):
    buf = torch.empty(n + GUARD, device=DEV, dtype=torch.float32)
    buf.view(torch.int32).fill_(NAN_BITS)
    return buf


def _behind(t):
    """a device copy of t with the NaN pattern behind it"""
    buf = _guarded(t.numel())
    buf[:t.numel()].copy_(t.flatten())
    return buf


def _intact(buf, n):
    return bool((buf.view(torch.int32)[n:] == NAN_BITS).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_int(t):
    return t.contiguous().view(torch.int32)


def _pair(images, shape, eps, fill, seed=0):
    """(x_orig, x_adv) fp32 on the CPU, |x_adv - x_orig|_2 = fill * eps per image as well as fp32 allows; x_orig in [0, 1], so the clamp
    of y has something to do"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(images, *shape, generator=g)
    d = torch.rand(images, *shape, generator=g) * 2 - 1
    d = d * (fill * eps / d.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
    return x, x + d


def _kinds(win, b, H, W, s):
    h1, w1, h2, w2 = (int(win[k][b]) for k in ('h1', 'w1', 'h2', 'w2'))
    k = {'identical'} if (h1, w1) == (h2, w2) else {'overlapping'} if abs(h1 - h2) < s and abs(w1 - w2) < s else {'disjoint'}
    if 0 in (h1, w1, h2, w2) or H in (h1 + s, h2 + s) or W in (w1 + s, w2 + s):
        k.add('border')
    k.add('transposed' if win['transposed'][b] else 'upright')
    return k


def _draws(images, H, W, s):
    """chosen on the CPU from square_ref.windows: the first draws that show a kind of window pair no earlier draw of this case showed"""
    seen, out = set(), []
    for draw in range(48):
        win = R.windows(images, H, W, s, SEED, draw, image_row=FAR[:images])
        new = set().union(*(_kinds(win, b, H, W, s) for b in range(images))) - seen
        if new:
            seen |= new
            out.append(draw)
    return out, seen


def _linf(x, xa, s, draw, eps, rows=None, row0=0, lo=0.0, hi=1.0):
    images, C, H, W = x.shape
    n = x.numel()
    xo, xd, y = _behind(x), _behind(xa), _guarded(n)
    r = None if rows is None else _first_rows_device(rows, DEV)
    L.check(L.lib.ga_square_linf(xo.data_ptr(), xd.data_ptr(), y.data_ptr(), images, C, H, W, s, SEED, draw, N.STREAM_SQUARE, row0,
                                 None if r is None else r.data_ptr(), eps, lo, hi, _stream()), 'ga_square_linf')
    torch.cuda.synchronize()
    assert _intact(y, n) and _intact(xo, n) and _intact(xd, n), 'wrote past the end of a buffer'
    return y[:n].view(x.shape).cpu()


def _l2(x, xa, table, draw, eps, rows=None, row0=0, lo=0.0, hi=1.0):
    images, C, H, W = x.shape
    n, s = x.numel(), table.shape[0]
    xo, xd, y, e = _behind(x), _behind(xa), _guarded(n), _behind(torch.from_numpy(table))
    r = None if rows is None else _first_rows_device(rows, DEV)
    L.check(L.lib.ga_square_l2(xo.data_ptr(), xd.data_ptr(), y.data_ptr(), e.data_ptr(), images, C, H, W, s, SEED, draw, N.STREAM_SQUARE, row0,
                               None if r is None else r.data_ptr(), eps, lo, hi, _stream()), 'ga_square_l2')
    torch.cuda.synchronize()
    assert _intact(y, n) and _intact(xo, n) and _intact(xd, n) and _intact(e, s * s), 'wrote past the end of a buffer'
    return y[:n].view(x.shape).cpu()


def _l2_bound(x, p, s, eps):
    """the module docstring's bound for one image: x [C, H, W] float64, p the restatement's intermediates -> [C, H, W]"""
    C, H, W = x.shape
    T, Tw = -(-H * W // 256), -(-s * s // 256)
    k1 = (C * T + C + 12 + 3) * U
    r = k1 / 2 + 2 * U
    old, new, h1, w1 = p['old'], p['new'], p['h1'], p['w1']
    a_new = np.abs(old) * (r + 2 * U) + U * np.abs(new)
    e_den = np.sqrt((a_new ** 2).sum(axis=(1, 2))) + p['n_new'] * ((Tw + 10) / 2 + 2) * U
    den = 1e-12 + p['n_new']
    spare = max(eps * eps - p['n_img2'], 0.0) / C
    e_t2 = (eps * eps * U + p['n_img2'] * k1) / C + 2 * U * spare + p['n_win2'] * k1 + U * p['target'] ** 2
    e_t = np.minimum(e_t2 / np.maximum(p['target'], 1e-300), np.sqrt(e_t2)) + U * p['target']
    e_scale = e_t / den + p['target'] * e_den / den ** 2 + U * p['scale']
    d2 = p['d2']
    e_d2 = U * np.abs(d2)                                                             # outside the windows: the subtraction
    win1 = d2[:, h1:h1 + s, w1:w1 + s]
    e_w = e_scale[:, None, None] * np.abs(new) + p['scale'][:, None, None] * a_new + U * np.abs(win1)
    e_d2[:, h1:h1 + s, w1:w1 + s] = e_w
    n_out = float((p['d'][:, ~p['union']] ** 2).sum())
    e_E = n_out * k1 + float((2 * np.abs(win1) * e_w).sum()) + (C * Tw + 14) * U * float((win1 ** 2).sum())
    rel_f = e_E / (2 * p['n_d2'] ** 2) + U + 3 * U
    y = x + d2 * p['f']
    return 2.0 * (p['f'] * e_d2 + np.abs(d2 * p['f']) * (rel_f + U) + U * np.abs(y))


def _l2_ratio(y, x, xa, table, draw, eps, rows):
    """worst |y - restatement| / bound over the launch"""
    parts = []
    ref = R.reference_l2(x.numpy(), xa.numpy(), table, SEED, draw, image_row=rows, eps=eps, parts=parts)
    s = table.shape[0]
    bound = np.stack([_l2_bound(x[b].numpy().astype(np.float64), parts[b], s, eps) for b in range(x.shape[0])])
    return float((np.abs(y.numpy().astype(np.float64) - ref) / bound).max()), parts


@pytest.mark.parametrize('shape, s, images', LINF_CASES)
def test_linf_has_the_bits_of_the_fp32_restatement(shape, s, images):
    C, H, W = shape
    eps = float(np.float32(0.05))
    x, xa = _pair(images, shape, 0.5, 0.9)
    draws, seen = _draws(images, H, W, s)
    for draw in draws + [0xFFFFFFFE]:
        for lo, hi in ((0.0, 1.0), (1.0, 0.0)):                                           # clamp on, clamp off
            y = _linf(x, xa, s, draw, eps, rows=FAR[:images], lo=lo, hi=hi)
            ref = R.reference_linf(x.numpy(), xa.numpy(), s, SEED, draw, image_row=FAR[:images], eps=eps, lo=lo, hi=hi)
            assert torch.equal(_as_int(y), _as_int(torch.from_numpy(ref))), (draw, lo)
            assert not torch.equal(y, xa)
        if s < min(H, W):
            other = R.reference_linf(x.numpy(), xa.numpy(), s, SEED, draw, image_row=[r + 1 for r in FAR[:images]], eps=eps)
            assert not np.array_equal(other, ref)                                          # the image row matters
    if shape == (3, 8, 8):                                                                 # W % 4 == 0 at pointers that are not 16-byte aligned
        n = x.numel()
        xo, xd, yb = _guarded(n + 1), _guarded(n + 1), _guarded(n + 1)
        xo[1:n + 1].copy_(x.flatten())
        xd[1:n + 1].copy_(xa.flatten())
        rows = _first_rows_device(FAR[:images], DEV)
        L.check(L.lib.ga_square_linf(xo[1:].data_ptr(), xd[1:].data_ptr(), yb[1:].data_ptr(), images, C, H, W, s, SEED, 5, N.STREAM_SQUARE, 0,
                                     rows.data_ptr(), eps, 0.0, 1.0, _stream()), 'ga_square_linf')
        torch.cuda.synchronize()
        assert _intact(yb, n + 1) and yb.view(torch.int32)[0].item() == NAN_BITS
        ref = R.reference_linf(x.numpy(), xa.numpy(), s, SEED, 5, image_row=FAR[:images], eps=eps)
        assert torch.equal(_as_int(yb[1:n + 1].cpu().view(x.shape)), _as_int(torch.from_numpy(ref)))


def test_the_chosen_l2_draws_show_every_kind_of_window_pair():
    seen = set()
    for shape, s, images in L2_CASES:
        seen |= _draws(images, shape[1], shape[2], s)[1]
    assert {'identical', 'overlapping', 'disjoint', 'border', 'transposed', 'upright'} <= seen


@pytest.mark.parametrize('shape, s, images', L2_CASES)
def test_l2_against_the_float64_restatement(shape, s, images):
    C, H, W = shape
    eps = float(np.float32(0.5))
    table = R.eta(s)
    draws, _ = _draws(images, H, W, s)
    worst, spent = 0.0, False
    for fill in (0.9, 1.0, 0.0):                       # inside the ball; on the sphere: no spare budget; x_adv = x_orig
        x, xa = _pair(images, shape, eps, fill, seed=int(fill * 10))
        for draw in draws:
            y = _l2(x, xa, table, draw, eps, rows=FAR[:images])
            ratio, parts = _l2_ratio(y, x, xa, table, draw, eps, FAR[:images])
            worst = max(worst, ratio)
            if fill == 1.0:
                assert all(max(eps * eps - p['n_img2'], 0.0) <= 1e-6 * eps * eps for p in parts)      # the zero-budget case occurs
                spent = True
            n = (y.double() - x.double()).flatten(1).norm(dim=1)
            assert (n <= eps * (1 + 1e-5)).all() and y.min() >= 0.0 and y.max() <= 1.0
    print(f'   l2 ({images} x {shape}, s {s}, draws {draws}): worst |y - ref| / bound = {worst:.3f}')
    assert spent and worst <= 1.0


def test_a_misread_choice_breaks_the_l2_bound_by_orders_of_magnitude(monkeypatch):
    """references that take another image's row, the opposite signs, the other orientation, or a window one pixel off"""
    shape, s, images, eps, draw = (3, 64, 64), 21, 3, float(np.float32(0.5)), 3
    table = R.eta(s)
    x, xa = _pair(images, shape, eps, 0.9)
    y = _l2(x, xa, table, draw, eps, rows=FAR)
    ratio, parts = _l2_ratio(y, x, xa, table, draw, eps, FAR)
    assert ratio <= 1.0
    bound = np.stack([_l2_bound(x[b].numpy().astype(np.float64), parts[b], s, eps) for b in range(images)])
    y64 = y.numpy().astype(np.float64)
    honest = R.windows

    def shifted(*a, **kw):
        w = honest(*a, **kw)
        w['w1'] = np.where(w['w1'] > 0, w['w1'] - 1, w['w1'] + 1)
        return w
    wrong = {'image row': lambda: R.reference_l2(x.numpy(), xa.numpy(), table, SEED, draw, image_row=[FAR[1], FAR[2], FAR[0]], eps=eps),
             'sign': lambda: R.reference_l2(x.numpy(), xa.numpy(), -table, SEED, draw, image_row=FAR, eps=eps),
             'orientation': lambda: R.reference_l2(x.numpy(), xa.numpy(), table.T.copy(), SEED, draw, image_row=FAR, eps=eps)}
    for name, ref in wrong.items():
        r = float((np.abs(y64 - ref()) / bound).max())
        print(f'   l2 against a reference with the wrong {name}: {r:.1e} of the bound')
        assert r >= 1e3
    monkeypatch.setattr(R, 'windows', shifted)
    r = float((np.abs(y64 - R.reference_l2(x.numpy(), xa.numpy(), table, SEED, draw, image_row=FAR, eps=eps)) / bound).max())
    print(f'   l2 against a reference with the wrong window: {r:.1e} of the bound')
    assert r >= 1e3
    monkeypatch.setattr(R, 'windows', honest)
    yl = _linf(x, xa, s, draw, 0.05, rows=FAR)
    monkeypatch.setattr(R, 'windows', shifted)
    assert not np.array_equal(yl.numpy(), R.reference_linf(x.numpy(), xa.numpy(), s, SEED, draw, image_row=FAR, eps=0.05))


@pytest.mark.parametrize('shape, s', [((3, 8, 8), 3), ((3, 6, 10), 5), ((3, 64, 64), 21)])
def test_an_image_does_not_depend_on_the_launch(shape, s):
    """bitwise: an image alone and in a batch of 3 at any position; the image_row array and the row0 it spells out"""
    eps, draw = 0.5, 2
    table = R.eta(s)
    x, xa = _pair(3, shape, eps, 0.9)
    alone = [(_linf(x[b:b + 1], xa[b:b + 1], s, draw, 0.05, rows=FAR[b:b + 1]), _l2(x[b:b + 1], xa[b:b + 1], table, draw, eps, rows=FAR[b:b + 1]))
             for b in range(3)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        rows = [FAR[b] for b in order]
        yl, y2 = _linf(x[order], xa[order], s, draw, 0.05, rows=rows), _l2(x[order], xa[order], table, draw, eps, rows=rows)
        for pos, b in enumerate(order):
            assert torch.equal(_as_int(yl[pos]), _as_int(alone[b][0][0])) and torch.equal(_as_int(y2[pos]), _as_int(alone[b][1][0]))
    assert torch.equal(_as_int(_l2(x, xa, table, draw, eps, row0=70)), _as_int(_l2(x, xa, table, draw, eps, rows=[70, 71, 72])))
    assert torch.equal(_as_int(_linf(x, xa, s, draw, 0.05, row0=70)), _as_int(_linf(x, xa, s, draw, 0.05, rows=[70, 71, 72])))
    top = (1 << 32) - 1                                                                  # the last row there is: no sign extension
    assert torch.equal(_as_int(_l2(x[:1], xa[:1], table, draw, eps, row0=top)), _as_int(_l2(x[:1], xa[:1], table, draw, eps, rows=[top])))


def test_bad_arguments_return_their_codes_without_a_launch():
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    y, e = _guarded(192), torch.zeros(9, device=DEV)

    def linf(C=3, H=8, W=8, s=3, images=1, row0=0, xo=x.data_ptr()):
        return L.lib.ga_square_linf(xo, x.data_ptr(), y.data_ptr(), images, C, H, W, s, SEED, 0, N.STREAM_SQUARE, row0, None, 0.1, 0.0, 1.0, _stream())

    def l2(C=3, H=8, W=8, s=3, images=1, row0=0, eta=e.data_ptr()):
        return L.lib.ga_square_l2(x.data_ptr(), x.data_ptr(), y.data_ptr(), eta, images, C, H, W, s, SEED, 0, N.STREAM_SQUARE, row0, None, 0.1, 0.0,
                                  1.0, _stream())
    for f in (linf, l2):
        assert f(s=0) == f(s=9) == f(images=0) == f(H=0) == f(row0=1 << 32) == L.GA_E_BADARG
        assert f(C=33) == L.GA_E_UNSUPPORTED
    assert linf(xo=None) == l2(eta=None) == L.GA_E_BADARG
    torch.cuda.synchronize()
    assert _intact(y, 0)                                                                  # nothing was launched: y is untouched


# ---------------------------------------------------------------------------------------------------------------- the attack
CFG = {'initial_channels': 8, 'num_pre-post_process_blocks': 1, 'num_pre-post_process_cells': 2, 'num_scales': 3,
       'num_groups_per_scale': 2, 'is_adaptive': False, 'min_groups_per_scale': 1, 'num_cells_per_group': 1,
       'num_latent_per_group': 4, 'num_logistic_mixtures': 10, 'num_nf_cells': None}
RES = (3, 64, 64)
EOT, IMAGES = 2, 2


@pytest.fixture(scope='module')
def nvae(tmp_path_factory):
    """the reduced NVAE + VGG defender of tests/test_noise_gpu.py (input noise eps 2.0) at EoT 2, with seeded draws"""
    d = tmp_path_factory.mktemp('square_ckpt')
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


def _labels(model, x):
    model.model.seeded_noise(7)
    with torch.no_grad():
        return model(x).argmax(dim=1)


@pytest.mark.parametrize('norm, eps', [('Linf', 8.0 / 255.0), ('L2', 0.5)])
def test_device_proposals_are_the_numpy_backends(nvae, norm, eps):
    """every proposal batch of a short device run, replayed by the numpy restatement from the iterate the run itself held"""
    args, model, x = nvae
    y = _labels(model, x)
    attack, net = A.SquareAttack(norm=norm, eps=eps, n_queries=6, p_init=0.1, seed=9), _Recorder(model)
    attack.image_index = torch.tensor([5, 2])
    model.model.seeded_noise(7)
    success, bound, adv = attack(x, y, net)
    torch.cuda.synchronize()
    model.model.seeded_noise(None)
    assert all(not grad_on for _, _, grad_on in net.calls) and attack.queries == sum(c[0].shape[0] for c in net.calls)
    eps32 = float(np.float32(eps))
    calls = list(net.calls)
    x_adv, logits, _ = calls.pop(0)
    x_adv = x_adv.clone()
    best = margin_loss(logits, y).clone()
    act = (logits.argmax(dim=1) == y).nonzero().flatten()
    replayed, worst = 0, 0.0
    for it in range(attack.n_queries - 1):
        if act.numel() == 0:
            break
        q, logits, _ = calls.pop(0)
        assert q.shape[0] == act.numel()
        s = attack.side(it, 64, 64)
        rows = [int(attack.image_index[b]) for b in act]
        xo, xa = x[act].cpu(), x_adv[act].cpu()
        if norm == 'Linf':
            ref = R.reference_linf(xo.numpy(), xa.numpy(), s, 9, it, image_row=rows, eps=eps32)
            assert torch.equal(_as_int(q.cpu()), _as_int(torch.from_numpy(ref)))
            assert np.array_equal(A.propose(norm, xo, xa, s, 9, it, rows, eps32).numpy(), ref)          # the CPU backend itself
        else:
            parts = []
            ref = R.reference_l2(xo.numpy(), xa.numpy(), R.eta(s), 9, it, image_row=rows, eps=eps32, parts=parts)
            bnd = np.stack([_l2_bound(xo[b].numpy().astype(np.float64), parts[b], s, eps32) for b in range(len(rows))])
            ratio = float((np.abs(q.cpu().numpy().astype(np.float64) - ref) / bnd).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (it, ratio)
        replayed += 1
        loss = margin_loss(logits, y[act])
        wrong = logits.argmax(dim=1) != y[act]
        take = (loss > best[act]) | wrong
        x_adv[act[take]] = q[take]
        best[act[take]] = loss[take]
        act = act[~wrong]
    assert not calls
    print(f'   {norm}: {replayed} proposal batches replayed, worst |proposal - numpy| / bound = {worst:.3f}; success {success.tolist()}')
    assert replayed >= 1, 'the defender misclassified every starting point: nothing was proposed'
    d = (adv - x).flatten(1)
    assert (adv >= 0).all() and (adv <= 1).all()
    assert (d.abs().amax(dim=1) <= eps + 1e-6).all() if norm == 'Linf' else (d.norm(dim=1) <= eps * (1 + 1e-5)).all()


def test_the_same_seed_twice_gives_the_same_attack(nvae):
    args, model, x = nvae
    y = _labels(model, x)
    out = []
    for _ in range(2):
        model.model.seeded_noise(7)
        out.append(A.SquareAttack(norm='L2', eps=0.5, n_queries=5, seed=9)(x, y, model))
    model.model.seeded_noise(None)
    for a, b in zip(*out):
        assert torch.equal(a, b)
    model.model.seeded_noise(7)
    one = A.SquareAttack(norm='Linf', eps=8.0 / 255.0, n_queries=3, seed=9)(x[:1], y[:1], model)
    model.model.seeded_noise(None)
    assert isinstance(one[0], bool) and isinstance(one[1], float)


def test_the_seeded_driver_writes_the_square_column_and_repeats_itself(nvae, tmp_path):
    """--attack square through experiments/seeded_defense.run_worker on 2 synthetic images"""
    from gen_adversarial_amd.experiments import seeded_defense as S
    from gen_adversarial_amd.experiments import test_defense as drv
    args, model, _ = nvae
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli = S.parse_args(['--noise_seed', '3', '--synthetic', '2', '--eot_steps', str(EOT), '--defense_type', 'ours', '--experiment', 'ids',
                            '--config', args.config, '--attack', 'square', '--batch_images', '2'])
    finally:
        os.chdir(cwd)
    assert cli.attack == 'square' and S.RESULT_KEYS['square'] == 'SQUARE'
    assert isinstance(args.square, A.SquareAttack) and args.square.norm == 'L2' and args.square.eps == 0.5 and args.square.n_queries == 5000
    data = drv.synthetic_dataset(2, 64, 100)
    seen = []

    class Spy(A.SquareAttack):
        def __call__(self, image, gt_label, net):
            seen.append(self.image_index.tolist())
            return super().__call__(image, gt_label, net)

    def run(name, seed, bi):
        sq = Spy(norm='L2', eps=0.5, n_queries=4, seed=1)
        a = Namespace(device=DEV, noise_seed=seed, batch_images=bi, schedule='static', attacks={'square': sq}, results_folder=str(tmp_path))
        path = str(tmp_path / f'{name}.json')
        res = S.run_worker(0, 1, a, lambda a_: (a_, model), data, results_path=path)
        assert 'SQUARE' in res and len(res['SQUARE']) == 2 and 'Clean' in res
        return open(path).read()
    first = run('a', 3, 2)
    assert seen == [[0, 1]]
    assert run('b', 3, 2) == first
    run('c', 3, 1)
    assert seen[2:] == [[0], [1]]                                                     # dataset indices, image by image
    assert model.model._noise_seed is None
