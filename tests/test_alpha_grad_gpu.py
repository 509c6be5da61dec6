"""
GPU: d loss / d alpha from the backward pass (the first-order tool).
  1. ga_sampler_mix mode 2 and ga_latent_mix backward == 2 against the header's formulas in float64, bound from the kernels' own
     summation trees; pad channels poisoned; only the op's own output column written;
  2. bits: run to run, and a row alone vs in a batch; refusals without a launch;
  3. an alpha_grad engine gives bitwise the logits and dx of a plain engine (three reduced defenders), also from HIP graphs;
  4. MLVGMDefenseModel.loss_and_alpha_grad against the oracle's gradient of the same loss, given the engine's decisions;
  5. one small step against the gradient does not raise the engine's own loss.
Reduced defenders, inputs and pinned draws: tests/alpha_search_cases.py (third candidate); oracle side: tests/alpha_grad_cases.py.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from gen_adversarial_amd import _lib as L   # noqa: E402
import opref   # noqa: E402
from alpha_grad_cases import LABELS, REFERENCES   # noqa: E402
from alpha_search_cases import B, CASES, E   # noqa: E402

DEV = 'cuda:0'
TYPES = ['vgg-11', 'resnet-50', 'resnext-50']
U = 2.0 ** -24              # unit roundoff of fp32
SENTINEL = -77.0


def dev(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def padded(t, ld, fill=1e30):
    """[..., C] float32 array -> device tensor of channel pitch ld, the pad channels poisoned"""
    out = torch.full(t.shape[:-1] + (ld,), fill, device=DEV)
    out[..., :t.shape[-1]] = dev(t)
    return out


# ---------------------------------------------------------------------------------------------------------------- sampler, mode 2
# (N, q_rep, h, NL, ldq = ldz, ldp or None): 80 terms per row (less than one workgroup), 320 (no multiple of 256), 1024
SAMPLER_CASES = [(3, 1, 2, 20, 24, None), (4, 2, 4, 20, 24, 48), (2, 1, 16, 4, 8, 8)]
ALPHA_LD, ALPHA_COL = 5, 3


def sampler_c(T):
    """additions on the longest path of sampler_alpha_grad_kernel's summation tree (tests/opref.py holds the count)"""
    return opref.sampler_alpha_c(T)


def sampler_data(case, seed):
    N, q_rep, h, NL, ld, ldp = case
    rng = np.random.RandomState(seed)
    mq = (2 * rng.randn(N // q_rep, h, h, NL)).astype(np.float32)
    p = None if ldp is None else np.concatenate([2 * rng.randn(N, h, h, NL), rng.randn(N, h, h, NL)], axis=3).astype(np.float32)
    eps = rng.randn(N, NL, h, h).astype(np.float32)                                # NCHW
    dz = rng.randn(N, h, h, NL).astype(np.float32)
    return mq, p, eps, dz


def sampler_terms64(case, mq, p, eps, dz, temp):
    """the header's formula (tests/opref.py) on the float32 inputs in float64: [N, h * w * NL] terms"""
    N, q_rep, h, NL, _, ldp = case
    t64 = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
    mq64 = opref.rep_rows(t64(mq), q_rep)
    mp = None if p is None else t64(p[..., :NL])
    ls = torch.zeros_like(mq64) if p is None else t64(p[..., NL:])
    term = opref.sampler_alpha_terms(mq64, mp, ls, t64(eps).permute(0, 2, 3, 1), t64(dz), temp)
    return term.reshape(N, -1).numpy()


def sampler_desc(case, mq_d, p_d, eps_d, dz_d, table, eps_nchw, temp, N=None, q_rep=None):
    _, qr, h, NL, ld, ldp = case
    d = L.SamplerDesc()
    d.mu_q, d.ldq, d.eps, d.eps_nchw, d.dz, d.ldz = mq_d.data_ptr(), ld, eps_d.data_ptr(), eps_nchw, dz_d.data_ptr(), ld
    if p_d is not None:
        d.p, d.ldp = p_d.data_ptr(), ldp
    d.N, d.h, d.w, d.NL, d.temp, d.q_rep = (case[0] if N is None else N), h, h, NL, temp, (qr if q_rep is None else q_rep)
    d.backward, d.mode, d.z, d.alpha_ld, d.alpha_col = 1, 2, table.data_ptr(), ALPHA_LD, ALPHA_COL
    d.alpha, d.one_minus_alpha = 0.25, 0.75                                        # must not be read
    return d


@pytest.mark.parametrize('eps_nchw', [0, 1])
@pytest.mark.parametrize('case', SAMPLER_CASES, ids=['80terms_first_group', '320terms_q_rep2', '1024terms'])
def test_sampler_alpha_cotangent_against_float64(case, eps_nchw):
    N, q_rep, h, NL, ld, ldp = case
    temp = 0.6
    mq, p, eps, dz = sampler_data(case, 3)
    terms = sampler_terms64(case, mq, p, eps, dz, temp)
    ref, mag = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    c = sampler_c(terms.shape[1])
    mq_d, dz_d = padded(mq, ld), padded(dz, ld)
    p_d = None if p is None else padded(p, ldp)
    eps_d = dev(eps if eps_nchw else eps.transpose(0, 2, 3, 1))
    table = torch.full((N, ALPHA_LD), SENTINEL, device=DEV)
    d = sampler_desc(case, mq_d, p_d, eps_d, dz_d, table, eps_nchw, temp)
    L.run(d)
    got = table.cpu().double().numpy()
    keep = [j for j in range(ALPHA_LD) if j != ALPHA_COL]
    assert (got[:, keep] == SENTINEL).all()                                        # only column 3 changes
    err = np.abs(got[:, ALPHA_COL] - ref)
    print(f'   sampler mode 2 {case} eps_nchw={eps_nchw}: c = {c}, max err / (c u sum|term|) = {(err / (c * U * mag)).max():.3f} '
          f'(max err {err.max():.3e}, sum|term| up to {mag.max():.3e})')
    assert np.isfinite(got).all() and (err <= c * U * mag).all()                   # pad channels (1e30) were not seen
    # bits: the same launch again, and every row alone (its own one-row launch, q_rep folded into the mu_q pointer)
    again = torch.full((N, ALPHA_LD), SENTINEL, device=DEV)
    d.z = again.data_ptr()
    L.run(d)
    assert torch.equal(again, table)
    for r in range(N):
        one = torch.full((1, ALPHA_LD), SENTINEL, device=DEV)
        d1 = sampler_desc(case, mq_d[r // q_rep:], None if p_d is None else p_d[r:], eps_d[r:], dz_d[r:], one, eps_nchw, temp, N=1, q_rep=1)
        L.run(d1)
        assert torch.equal(one[0, ALPHA_COL], table[r, ALPHA_COL]), r


def test_sampler_alpha_cotangent_refusals():
    case = SAMPLER_CASES[1]
    mq, p, eps, dz = sampler_data(case, 4)
    table = torch.full((case[0], ALPHA_LD), SENTINEL, device=DEV)
    args = (padded(mq, case[4]), padded(p, case[5]), dev(eps), padded(dz, case[4]))

    def rc(**kw):
        d = sampler_desc(case, *args, table, 1, 0.6)
        for k, v in kw.items():
            setattr(d, k, v)
        return L.lib.ga_sampler_mix(ctypes.byref(d), 0)
    assert rc() == L.GA_OK
    torch.cuda.synchronize()
    table.fill_(SENTINEL)
    for kw in ({'act_rep': 2}, {'z': None}, {'dz': None}, {'alpha_col': -1}, {'alpha_col': ALPHA_LD}, {'backward': 0}):
        assert rc(**kw) == L.GA_E_BADARG, kw
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all())                                          # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- latent mix, backward 2
def latent_c(D):
    """additions on the longest path of latent_alpha_grad_kernel (tests/opref.py holds the count)"""
    return opref.latent_alpha_c(D)


@pytest.mark.parametrize('with_avg', [False, True])
@pytest.mark.parametrize('shape', [(6, 3, 5, 8), (2, 1, 18, 512)], ids=['two_quads', 'J18_D512'])
def test_latent_alpha_cotangent_against_float64(shape, with_avg):
    R, rep, J, D = shape
    rng = np.random.RandomState(5)
    codes = rng.randn(R // rep, J, D).astype(np.float32)
    avg = rng.randn(J, D).astype(np.float32) if with_avg else None
    styles = rng.randn(R, J, D).astype(np.float32)
    dout = rng.randn(R, J, D).astype(np.float32)
    t64 = lambda v: None if v is None else torch.from_numpy(v).double()
    terms = opref.latent_alpha_terms(t64(codes), t64(avg), t64(styles), t64(dout), rep).numpy()
    ref, mag, c = terms.sum(axis=2), np.abs(terms).sum(axis=2), latent_c(D)
    cd, sd, dd = dev(codes), dev(styles), dev(dout)
    ad = dev(avg) if with_avg else None

    def desc(out, r0=0, rows=R, rp=rep):
        m = L.LatentMixDesc()
        m.codes, m.styles, m.dout, m.out = cd[r0 // rep:].data_ptr(), sd[r0:].data_ptr(), dd[r0:].data_ptr(), out.data_ptr()
        m.avg = ad.data_ptr() if with_avg else None
        m.R, m.J, m.D, m.rep, m.backward = rows, J, D, rp, 2                        # alpha NULL, alpha_ld 0: not read
        return m
    out = torch.full((R, J), SENTINEL, device=DEV)
    L.run(desc(out))
    got = out.cpu().double().numpy()
    err = np.abs(got - ref)
    print(f'   latent mix backward 2 {shape} avg={with_avg}: c = {c}, max err / (c u sum|term|) = {(err / (c * U * mag)).max():.3f} '
          f'(max err {err.max():.3e})')
    assert (err <= c * U * mag).all()
    again = torch.full((R, J), SENTINEL, device=DEV)
    L.run(desc(again))
    assert torch.equal(again, out)
    for r in range(R):                                                              # a row alone: the same bits
        one = torch.full((1, J), SENTINEL, device=DEV)
        L.run(desc(one, r0=r, rows=1, rp=1))
        assert torch.equal(one[0], out[r]), r


# ---------------------------------------------------------------------------------------------------------------- engines
@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import AlphaEvaluator
    built = {}

    def get(classifier_type):
        if classifier_type not in built:
            c = CASES[classifier_type](str(tmp_path_factory.mktemp('alpha_grad_' + classifier_type.replace('-', '_'))))
            c.ev = AlphaEvaluator(c.args, DEV, images=c.x, labels=torch.tensor(LABELS), batch_images=B)
            c.model = c.ev.defense_model.model
            c.model.image_size = c.res
            c.model.interpolation_alphas = c.engine_alphas(2)
            built[classifier_type] = c
        return built[classifier_type]
    return get


@pytest.mark.parametrize('classifier_type', TYPES)
def test_alpha_grad_engine_moves_nothing_else(cases, classifier_type):
    c = cases(classifier_type)
    rows = B * E
    plain = c.model._make_engine(rows, E, True)
    grad = c.model._make_engine(rows, E, True, alpha_grad=True)
    assert plain.alpha_grad_rows is None and tuple(grad.alpha_grad_rows.shape) == (rows, c.n)
    assert plain.fwd.names == grad.fwd.names and len(grad.bwd) - len(plain.bwd) == (c.n if classifier_type == 'vgg-11' else 1)
    cot = torch.randn(plain.logits.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    for eng in (plain, grad):
        eng.set_alphas(c.engine_alphas(2))
        eng.x_in.copy_(c.x.to(DEV))
        for dst, src in zip(eng.eps, c.draws_of(2)):
            dst.copy_(src.to(DEV))
        eng.forward()
        eng.dlogits.view_as(eng.logits).copy_(cot)
        eng.backward()
    torch.cuda.synchronize()
    assert torch.equal(plain.logits, grad.logits) and torch.equal(plain.dx, grad.dx)
    assert plain.dx.abs().max().item() > 0
    table = grad.alpha_grads().clone()
    assert torch.isfinite(table).all() and table.abs().max().item() > 0
    if classifier_type == 'vgg-11':             # the ops sit in the plan like any other: captured graphs replay them
        grad.alpha_grad_rows.fill_(SENTINEL)
        grad.enable_graphs()
        grad.forward()
        grad.backward()
        torch.cuda.synchronize()
        assert torch.equal(grad.alpha_grads(), table) and torch.equal(plain.dx, grad.dx)
        grad.disable_graphs()


def _api(c, alphas):
    c.model.interpolation_alphas = list(alphas)
    c.model.fixed_noise([d.to(DEV) for d in c.draws_of(2)], None)
    try:
        loss, dalpha = c.model.loss_and_alpha_grad(c.x.to(DEV), torch.tensor(LABELS), rep=E)
    finally:
        c.model.fixed_noise(None, None)
    return loss.double().cpu(), dalpha.double().cpu()


@pytest.mark.parametrize('classifier_type', TYPES)
def test_loss_and_alpha_grad_against_the_oracle(cases, classifier_type):
    """dalpha [B, n] of the API against the oracle's gradient of the same loss (tests/alpha_grad_cases.py), the oracle evaluated with the
    decisions the engine took (oracle/kinks.py replay, as tests/gradcheck.py does for input gradients); bound: that helper's 1e-3
    of max |dalpha|"""
    from gradcheck import engine_candidates
    from oracle import kinks as K
    c = cases(classifier_type)
    alphas = c.engine_alphas(2)
    loss, got = _api(c, alphas)
    eng = c.model._engine(B * E, E, True, alpha_grad=True)         # the engine that call ran on, its activations still in place
    assert loss.shape == (B,) and got.shape == (B, c.n)
    small = [t.detach() for t in getattr(eng, 'small_kinks', [])]
    small = [t.repeat_interleave(eng.rows // t.shape[0], dim=0) if (t.shape[0] != eng.rows and eng.rows % t.shape[0] == 0) else t
             for t in small]
    with K.replaying(engine_candidates(eng), small=[t.float().cpu() for t in small]) as rp:
        ref_loss, ref = REFERENCES[classifier_type](c.x, alphas, c.draws_of(2), torch.tensor(LABELS), E)
    big = [u for u in rp.unmatched if torch.Size(u[1]).numel() >= 48]
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item() / max(scale, 1e-30)
    print(f'   {classifier_type}: loss {loss.tolist()} (oracle {ref_loss.tolist()}), max |dalpha| {scale:.3e}, dalpha err {err:.2e} of it; '
          f'{rp.summary()}; unmatched sites of >= 48 decisions: {big[:8]}')
    assert not big, big
    assert rp.matched >= 1
    assert scale >= 1e-4 * ref_loss.max().item()                    # not a comparison of two zeros
    assert err <= 1e-3


def test_a_step_against_the_gradient_does_not_raise_the_loss(cases):
    c = cases('vgg-11')
    a = np.asarray(c.engine_alphas(2), dtype=np.float64)
    loss0, g = _api(c, a.tolist())
    g = g.sum(dim=0).numpy()                                       # gradient of the summed loss
    step = 1e-2 / np.abs(g).max()
    a1 = np.clip(a - step * g, 0.0, 1.0)
    loss1, _ = _api(c, a1.tolist())
    print(f'   summed loss {loss0.sum().item():.6f} -> {loss1.sum().item():.6f} after a step of {step:.3e} against the gradient '
          f'(first-order estimate {-(g * (a - a1)).sum():.3e})')
    assert not np.array_equal(a, a1)
    assert loss1.sum().item() <= loss0.sum().item()
