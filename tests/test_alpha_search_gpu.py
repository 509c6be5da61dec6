"""
GPU: the candidate-batched alpha search (SURVEY.md §8 row f2 for K candidates per engine pass).
  1. ga_sampler_mix / ga_latent_mix with a per-row alpha table, forward and backward, against the header's formulas in float64;
  2. table vs scalar alphas on the same engine shape: bitwise, for the three defenders;
  3. K = 3 candidates x B = 2 images x EoT 2 in one pass vs one call per candidate with that candidate's slice of the draws;
  4. the same against the CPU oracle, one oracle call per candidate; verdicts equal on every image;
  5. AlphaEvaluator.objective_many = the mean of those verdicts; input noise is refused.
Reduced defenders, inputs and pinned draws: tests/alpha_search_cases.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from gen_adversarial_amd import _lib as L   # noqa: E402
import opref   # noqa: E402
from alpha_search_cases import B, CASES, E, K, candidate_rows   # noqa: E402

DEV = 'cuda:0'
TYPES = ['vgg-11', 'resnet-50', 'resnext-50']


def _close64(got, ref, tol, what):
    """the comparison of tests/test_ops_gpu.py::test_sampler (close(), :37-41): max err <= tol * max(1, max |ref|), tol = 1e-6"""
    got = got.detach().cpu().double().numpy()
    err, scale = np.abs(got - ref).max(), max(1.0, np.abs(ref).max())
    print(f'   {what}: max err {err:.3e} of {scale:.3e} (bound {tol * scale:.3e})')
    assert err <= tol * scale, what


@pytest.mark.parametrize('first', [False, True])
def test_sampler_with_per_row_alphas(first):
    """q_rep = 3 rows per mu_q row, latent pitch 8 for 6 channels, eps in NCHW, a table of 3 column pairs of which the op reads
    pair 1; row n's z and cotangents use row n's (alpha, 1 - alpha)"""
    N, h, NL, LD, temp, q_rep, ncol, col = 6, 4, 6, 8, 0.6, 3, 3, 1
    rng = np.random.RandomState(1)
    mq = (3 * rng.randn(N // q_rep, h, h, NL)).astype(np.float32)                   # NHWC
    p = None if first else (3 * rng.randn(N, h, h, 2 * NL)).astype(np.float32)
    eps = rng.randn(N, NL, h, h).astype(np.float32)                                # NCHW
    cot = rng.randn(N, h, h, NL).astype(np.float32)
    alpha = rng.rand(N, ncol)
    alpha[0, col], alpha[1, col] = 0.0, 1.0
    table = np.stack([alpha.astype(np.float32), (1.0 - alpha).astype(np.float32)], axis=2).reshape(N, 2 * ncol)
    # float64 reference (tests/opref.py) on the float32 inputs, with the pair the kernel reads
    t64 = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
    a, om = (t64(table[:, 2 * col + i]).view(N, 1, 1, 1) for i in (0, 1))
    mq64 = opref.rep_rows(t64(mq), q_rep)
    mp = None if first else t64(p[..., :NL])
    ls = torch.zeros_like(mq64) if first else t64(p[..., NL:])
    e64 = t64(eps).permute(0, 2, 3, 1)
    z_ref = opref.sampler_mix(mq64, mp, ls, e64, a, om, temp).numpy()
    denc, dmp_ref, dls_ref = (v.numpy() for v in opref.sampler_mix_bwd(mq64, mp, ls, e64, t64(cot), a, om, temp))

    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
    mqd = torch.full((N // q_rep, h, h, LD), 7.0, device=DEV)
    mqd[..., :NL] = dev(mq)
    z = torch.full((N, h, h, LD), -3.0, device=DEV)
    td, ed = dev(table), dev(eps)
    d = L.SamplerDesc()
    d.mu_q, d.ldq, d.eps, d.eps_nchw, d.z, d.ldz = mqd.data_ptr(), LD, ed.data_ptr(), 1, z.data_ptr(), LD
    if not first:
        pd = dev(p)
        d.p, d.ldp = pd.data_ptr(), 2 * NL
    d.N, d.h, d.w, d.NL, d.temp, d.q_rep = N, h, h, NL, temp, q_rep
    d.alpha, d.one_minus_alpha = 0.5, 0.5                                          # must not be read
    d.alpha_rows, d.alpha_ld, d.alpha_col = td.data_ptr(), 2 * ncol, col
    L.run(d)
    _close64(z[..., :NL], z_ref, 1e-6, 'sampler fwd, per-row alphas')
    assert bool((z[..., NL:] == -3.0).all())
    cd = torch.full((N, h, h, LD), 7.0, device=DEV)
    cd[..., :NL] = dev(cot)
    rows = torch.full((N, h, h, LD), -9.0, device=DEV)
    dp = torch.empty(N, h, h, 2 * NL, device=DEV)
    d.backward, d.dz, d.dmu_q_rows = 1, cd.data_ptr(), rows.data_ptr()
    if not first:
        d.dp = dp.data_ptr()
    L.run(d)
    _close64(rows[..., :NL], denc, 1e-6, 'sampler dmu_q_rows, per-row alphas')
    assert bool((rows[..., NL:] == -9.0).all())
    if not first:
        _close64(dp, np.concatenate([dmp_ref, dls_ref], axis=3), 1e-6, 'sampler dp, per-row alphas')
    # act_rep = 2 cotangents per forward row: the table is indexed by the forward row
    Kc = 2
    cot2 = rng.randn(N * Kc, h, h, NL).astype(np.float32)
    cd2 = torch.zeros(N * Kc, h, h, LD, device=DEV)
    cd2[..., :NL] = dev(cot2)
    rows2 = torch.zeros(N * Kc, h, h, LD, device=DEV)
    dp2 = torch.empty(N * Kc, h, h, 2 * NL, device=DEV)
    d.N, d.act_rep, d.dz, d.dmu_q_rows = N * Kc, Kc, cd2.data_ptr(), rows2.data_ptr()
    if not first:
        d.dp = dp2.data_ptr()
    L.run(d)
    rep2 = lambda t: None if t is None else opref.rep_rows(t, Kc)
    denc2 = opref.sampler_mix_bwd(rep2(mq64), rep2(mp), rep2(ls), rep2(e64), t64(cot2), rep2(a), rep2(om), temp)[0].numpy()
    _close64(rows2[..., :NL], denc2, 1e-6, 'sampler dmu_q_rows, act_rep 2')


def test_latent_mix_with_per_row_alphas():
    """rep = 3 rows per code row, a table pitch of 7 for J = 5; bound per element (two-term fp32 lerp, no transcendental):
    4 * 2^-24 * (|1 - a| |codes + avg| + |a| |styles|) forward, (rep + 1) roundings of the same kind for dcodes"""
    R, J, D, rep, ld = 6, 5, 8, 3, 7
    rng = np.random.RandomState(2)
    codes = rng.randn(R // rep, J, D).astype(np.float32)
    avg = rng.randn(J, D).astype(np.float32)
    styles = rng.randn(R, J, D).astype(np.float32)
    dout = rng.randn(R, J, D).astype(np.float32)
    table = np.full((R, ld), 9.0, dtype=np.float32)
    table[:, :J] = rng.rand(R, J).astype(np.float32)
    table[0, 0], table[1, 0] = 0.0, 1.0
    a = table[:, :J].astype(np.float64).reshape(R, J, 1)
    ca = np.repeat(codes.astype(np.float64), rep, axis=0) + avg.astype(np.float64)
    t64 = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
    ref = opref.latent_mix_rows(t64(codes), t64(avg), t64(styles), t64(table[:, :J]), rep).numpy()
    bound = 4 * 2.0 ** -24 * (np.abs(1.0 - a) * np.abs(ca) + np.abs(a) * np.abs(styles.astype(np.float64)))
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
    cd, ad, sd, dd, td = dev(codes), dev(avg), dev(styles), dev(dout), dev(table)
    out = torch.zeros(R, J, D, device=DEV)
    m = L.LatentMixDesc()
    m.codes, m.avg, m.styles, m.alpha, m.out = cd.data_ptr(), ad.data_ptr(), sd.data_ptr(), td.data_ptr(), out.data_ptr()
    m.R, m.J, m.D, m.rep, m.alpha_ld = R, J, D, rep, ld
    L.run(m)
    err = np.abs(out.cpu().double().numpy() - ref)
    print(f'   latent_mix fwd, per-row alphas: max err {err.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}')
    assert (err <= bound).all()
    term = (1.0 - a) * dout.astype(np.float64)
    ref_d = opref.latent_mix_rows_bwd(t64(dout), t64(table[:, :J]), rep).numpy()
    bound_d = (rep + 1) * 2.0 ** -24 * np.abs(term).reshape(R // rep, rep, J, D).sum(axis=1)
    dcodes = torch.zeros(R // rep, J, D, device=DEV)
    m.backward, m.dout, m.dcodes = 1, dd.data_ptr(), dcodes.data_ptr()
    L.run(m)
    err = np.abs(dcodes.cpu().double().numpy() - ref_d)
    print(f'   latent_mix bwd, per-row alphas: max err {err.max():.3e}, max err / bound {(err / np.maximum(bound_d, 1e-300)).max():.3f}')
    assert (err <= bound_d).all()


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import AlphaEvaluator
    built = {}

    def get(classifier_type):
        if classifier_type not in built:
            c = CASES[classifier_type](str(tmp_path_factory.mktemp('alpha_' + classifier_type.replace('-', '_'))))
            c.ev = AlphaEvaluator(c.args, DEV, images=c.x, labels=torch.zeros(B, dtype=torch.long), batch_images=B)
            c.model = c.ev.defense_model.model
            c.model.image_size = c.res
            built[classifier_type] = c
        return built[classifier_type]
    return get


def _batched(c, want_purified=False):
    """the K candidates x B images x E replicas in ONE pass under the pinned draws: logits [K, B * E, classes] (candidate-major)"""
    c.model.fixed_noise([d.to(DEV) for d in c.draws], None)
    try:
        out = c.model.forward_candidates(c.x.to(DEV), c.cand.double() * c.attenuation, rep=E, preds_only=not want_purified)
    finally:
        c.model.fixed_noise(None, None)
    logits = out[0] if want_purified else out
    lg = logits.permute(1, 0, 2, 3).reshape(K, B * E, -1).cpu()
    return (lg, out[1]) if want_purified else lg


@pytest.mark.parametrize('classifier_type', TYPES)
def test_table_of_equal_rows_is_bitwise_the_scalar_alphas(cases, classifier_type):
    """same plan, same arithmetic, and the table stores the pair the scalar descriptor fields hold: logits and purified image equal
    bit for bit.  Both engines forward-only, B * K * E rows, K * E rows per image."""
    c = cases(classifier_type)
    alphas = c.engine_alphas(2)
    rows, rep = B * K * E, K * E
    tab = c.model._engine(rows, rep, True, alpha_rows=True)
    plain = c.model._make_engine(rows, rep, True, need_backward=False)
    assert tab.alpha_table is not None and plain.alpha_table is None and tab.enc_rows == plain.enc_rows == B
    assert tab.fwd.names == plain.fwd.names
    plain.set_alphas(alphas)
    got = []
    for eng, fill in ((tab, lambda: tab.set_alpha_rows([alphas] * K)), (plain, lambda: None), (tab, lambda: tab.set_alphas(alphas))):
        fill()
        eng.x_in.copy_(c.x.to(DEV))
        for dst, src in zip(eng.eps, c.draws):
            dst.copy_(src.to(DEV))
        eng.forward()
        got.append((eng.logits.clone(), eng.purified.clone() if eng.purified is not None else eng.purified_nchw()))
    for lg, pur in (got[0], got[2]):
        assert torch.equal(lg, got[1][0]) and torch.equal(pur, got[1][1])
    assert got[1][0].abs().max().item() > 0


@pytest.mark.parametrize('classifier_type', TYPES)
def test_candidates_in_one_pass_match_one_call_each_and_the_oracle(cases, classifier_type):
    c = cases(classifier_type)
    ref = c.oracle_logits()                                           # [K, B * E, classes], one oracle call per candidate
    tol = c.tol(ref)
    # condition of the comparison, on the oracle side: no verdict near a tie, so no image has to be left out
    margin = c.min_margin()
    print(f'   {classifier_type}: logit tolerance {tol:.2e}, smallest top-2 margin of the oracle EoT means {margin:.3e}')
    assert margin >= 10 * tol
    got = _batched(c)
    old = list(c.model.interpolation_alphas)
    try:
        for k in range(K):
            c.model.interpolation_alphas = c.engine_alphas(k)
            c.model.fixed_noise([d.to(DEV) for d in c.draws_of(k)], None)
            with torch.no_grad():
                one = c.model.forward_rows(c.x.to(DEV), rep=E).cpu().view(B * E, -1)
            e_one, e_ref = (got[k] - one).abs().max().item(), (got[k] - ref[k]).abs().max().item()
            print(f'   candidate {k}: batched vs its own call {e_one:.2e}, batched vs oracle {e_ref:.2e}, own call vs oracle '
                  f'{(one - ref[k]).abs().max().item():.2e}')
            assert e_one < tol and e_ref < tol
    finally:
        c.model.interpolation_alphas = old
        c.model.fixed_noise(None, None)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])      # the candidates are distinct functions
    verdicts = got.view(K, B, E, -1).mean(dim=2).argmax(dim=2) == c.labels().view(1, -1)
    assert torch.equal(verdicts, c.verdicts())                                      # every image, every candidate


@pytest.mark.parametrize('classifier_type', TYPES)
def test_objective_many_is_the_mean_of_the_oracle_verdicts(cases, classifier_type):
    c = cases(classifier_type)
    want = c.verdicts()                                               # bool [K, B]
    c.ev.labels = c.labels().to(DEV)
    c.model.fixed_noise([d.to(DEV) for d in c.draws], None)
    try:
        hits = c.ev.per_image_verdicts_many(c.cand, candidates_per_pass=K)
        acc = c.ev.objective_many(c.cand, candidates_per_pass=K)
        assert c.ev.default_candidates_per_pass() >= 1
    finally:
        c.model.fixed_noise(None, None)
    assert hits.dtype == np.bool_ and hits.shape == (K, B) and hits.tolist() == want.tolist()
    assert acc.shape == (K,) and np.array_equal(acc, want.float().mean(dim=1).numpy())
    # fresh draws, one candidate per pass and the default: same shapes, accuracies in range
    for cpp in (1, None):
        a = c.ev.objective_many(c.cand, candidates_per_pass=cpp)
        assert a.shape == (K,) and ((0.0 <= a) & (a <= 1.0)).all()


@pytest.mark.parametrize('classifier_type', TYPES)
def test_input_noise_is_refused(cases, classifier_type):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import DEFENDERS
    c = cases(classifier_type)
    noisy = DEFENDERS[classifier_type][1](c.model.classifier, c.args.autoencoder_path, [0.] * c.n, alpha_attenuation=c.attenuation,
                                          initial_noise_eps=2.0, device=DEV)
    with pytest.raises(ValueError, match='initial_noise_eps'):
        noisy.forward_candidates(c.x.to(DEV), c.cand, rep=E)
    with pytest.raises(ValueError, match='input noise'):
        noisy._make_engine(B * K * E, K * E, True, need_backward=False, alpha_rows=True)
    assert not noisy._engines                                          # nothing was built
