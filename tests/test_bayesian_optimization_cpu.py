"""
No GPU: the Gaussian-process surrogate (experiments/alpha_learning/gp.py) and the Bayesian optimisation of the alphas built on it
(bayesian_optimization.py), against textbook formulas evaluated independently in numpy float64, central differences, and the
existing random search on a stub evaluator whose accuracy is a known function of the alphas.
"""
import contextlib
import io
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from gen_adversarial_amd.experiments.alpha_learning import gp as G

DT = torch.float64


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=DT)


def _np_kernel(A, B, ls):
    d = (A[:, None, :] - B[None, :, :]) / ls
    return np.exp(-0.5 * (d ** 2).sum(axis=2))


# ---------------------------------------------------------------------------------------------------------------- 1. posterior
N1, D1, NOISE1, LS1 = 12, 4, 1e-3, (0.3, 0.5, 1.0, 2.0)


def _posterior_case(mean):
    X, y, Xs = _rand(N1, D1, seed=1), 3.0 + 2.0 * torch.randn(N1, generator=torch.Generator().manual_seed(2), dtype=DT), _rand(20, D1, seed=3)
    gp = G.GP(X, y, LS1, NOISE1, mean)
    mu, var = gp.posterior(Xs)
    m, s = gp.standardize
    assert abs(m - y.mean().item()) < 1e-14 and abs(s - y.std().item()) < 1e-14
    return gp, X.numpy(), ((y - m) / s).numpy(), Xs.numpy(), ((mu - m) / s).numpy(), (var / s ** 2).numpy()


@pytest.mark.parametrize('mean', [0.0, 0.3])
def test_posterior_is_the_textbook_formula(mean):
    """k*^T (K + s2 I)^-1 (z - m) + m and k** - k*^T (K + s2 I)^-1 k* by numpy's solve, on the standardised scale.  Both sides
    float64 with cond(K + s2 I) <= n / s2 = 1.2e4: rounding near 1e-12, bound 1e-8."""
    _, X, z, Xs, mu, var = _posterior_case(mean)
    ls = np.asarray(LS1)
    K, Ks = _np_kernel(X, X, ls) + NOISE1 * np.eye(N1), _np_kernel(Xs, X, ls)
    ref_mu = mean + Ks @ np.linalg.solve(K, z - mean)
    ref_var = 1.0 - np.einsum('ij,ji->i', Ks, np.linalg.solve(K, Ks.T))
    e_mu, e_var = np.abs(mu - ref_mu).max(), np.abs(var - ref_var).max()
    print(f'   posterior vs numpy: mean {e_mu:.2e}, variance {e_var:.2e} (bound 1e-8); cond {np.linalg.cond(K):.2e}')
    assert e_mu <= 1e-8 and e_var <= 1e-8
    assert ref_var.min() > 1e-6 and np.abs(ref_mu).max() > 0.1              # the comparison is not of zeros


def test_posterior_agrees_with_sklearn_where_it_is_installed():
    gpr = pytest.importorskip('sklearn.gaussian_process')
    _, X, z, Xs, mu, var = _posterior_case(0.0)
    model = gpr.GaussianProcessRegressor(kernel=gpr.kernels.RBF(length_scale=np.asarray(LS1)), alpha=NOISE1, optimizer=None).fit(X, z)
    ref_mu, ref_sd = model.predict(Xs, return_std=True)
    assert np.abs(mu - ref_mu).max() <= 1e-8 and np.abs(var - ref_sd ** 2).max() <= 1e-8


def test_targets_that_are_all_equal_get_a_unit_standard_deviation():
    gp = G.GP(_rand(4, 2, seed=1), torch.full((4,), 0.25, dtype=DT), (1.0, 1.0), 1e-2)
    assert gp.standardize == (0.25, 1.0)
    mu, var = gp.posterior(_rand(3, 2, seed=2))
    assert torch.allclose(mu, torch.full((3,), 0.25, dtype=DT), atol=1e-12) and bool((var > 0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. MAP gradient
def test_map_objective_gradient_matches_central_differences():
    """every hyper-parameter (d log-lengthscales, log-noise, mean), h = 1e-5, relative 1e-5 per component"""
    n, d, h = 10, 3, 1e-5
    gp = G.GP(_rand(n, d, seed=4), torch.sin(4.0 * _rand(n, d, seed=4)[:, 0]) + _rand(n, seed=5), (0.4, 0.9, 1.7), 2e-2, 0.2)
    theta = gp.theta.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(gp.map_objective(theta), [theta])
    for i in range(d + 2):
        e = torch.zeros(d + 2, dtype=DT)
        e[i] = h
        fd = (gp.map_objective(gp.theta + e).item() - gp.map_objective(gp.theta - e).item()) / (2 * h)
        print(f'   d/dtheta[{i}]: autograd {grad[i].item():+.10e}, central differences {fd:+.10e}')
        assert abs(grad[i].item() - fd) <= 1e-5 * abs(fd) and abs(fd) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- 3. condition_on
def test_condition_on_equals_the_model_on_one_more_point():
    """same hyper-parameters — the standardisation pair belongs to them: they are expressed on its scale — and n + 1 points"""
    n, d = 9, 3
    X, y = _rand(n + 1, d, seed=6), _rand(n + 1, seed=7)
    base = G.GP(X[:n], y[:n], (0.5, 0.8, 1.2), 5e-3, -0.1)
    cond = base.condition_on(X[n], y[n])
    full = G.GP(X, y, (0.5, 0.8, 1.2), 5e-3, -0.1, standardize=base.standardize)
    assert cond.n == n + 1 and base.n == n and cond.best_f == base.best_f == y[:n].min().item()
    Xs = _rand(15, d, seed=8)
    for a, b in zip(cond.posterior(Xs), full.posterior(Xs)):
        assert (a - b).abs().max().item() <= 1e-9
    # and without the constructor's `standardize` argument: numpy on the n + 1 points, targets on the scale of the first n
    m, s = y[:n].mean().item(), y[:n].std().item()
    ls, z = np.asarray((0.5, 0.8, 1.2)), ((y - m) / s).numpy()
    K, Ks = _np_kernel(X.numpy(), X.numpy(), ls) + 5e-3 * np.eye(n + 1), _np_kernel(Xs.numpy(), X.numpy(), ls)
    ref_mu = m + s * (-0.1 + Ks @ np.linalg.solve(K, z + 0.1))
    ref_var = s ** 2 * (1.0 - np.einsum('ij,ji->i', Ks, np.linalg.solve(K, Ks.T)))
    mu, var = cond.posterior(Xs)
    assert np.abs(mu.numpy() - ref_mu).max() <= 1e-9 and np.abs(var.numpy() - ref_var).max() <= 1e-9
    # and it changed the model: the new point is now explained
    assert abs(cond.posterior(X[n:])[0].item() - y[n].item()) < abs(base.posterior(X[n:])[0].item() - y[n].item())


# ---------------------------------------------------------------------------------------------------------------- 4. the fit
def test_fit_finds_the_one_dimension_that_matters():
    X = _rand(30, 5, seed=9)
    y = torch.sin(6.0 * X[:, 0])
    gp = G.GP.fit(X, y, seed=0)
    ls = gp.lengthscale.tolist()
    start = gp.map_objective(G.prior_mode_theta(5)).item()
    print(f'   lengthscales {[round(v, 3) for v in ls]}, noise {gp.noise.item():.2e}, MAP objective {gp.map_objective().item():.3f} (start {start:.3f})')
    assert all(ls[0] < v for v in ls[1:])
    assert gp.map_objective().item() <= start
    assert gp.map_objective().item() < start                # and L-BFGS moved: `<=` alone holds for a fit that returns its start


# ---------------------------------------------------------------------------------------------------------------- 5. EI
def _ei_numpy(mu, sigma, best_f):
    z = (best_f - mu) / sigma
    return sigma * (z * 0.5 * (1.0 + math.erf(z / math.sqrt(2.0))) + math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))


def test_expected_improvement_is_the_analytic_form():
    """|z| <= 4, where math.erf's own rounding (1.1e-16 on Phi) puts the reference within 5e-16 sigma: bound 1e-13 sigma, five
    orders below the smallest value compared (z Phi + phi = 7e-6 at z = -4)"""
    best_f = 0.3
    for sigma in (1e-3, 0.05, 1.0, 7.0):
        for z in np.linspace(-4.0, 4.0, 33):
            mu = best_f - z * sigma
            got = G.expected_improvement(torch.tensor([mu], dtype=DT), torch.tensor([sigma], dtype=DT), best_f).item()
            assert abs(got - _ei_numpy(mu, sigma, best_f)) <= 1e-13 * sigma, (sigma, z)


def test_expected_improvement_is_nonnegative_and_tends_to_the_plain_improvement():
    mu = torch.tensor([-2.0, -0.5, 0.0, 0.29, 0.3, 0.31, 1.0, 50.0], dtype=DT)
    for sigma in (10.0, 1.0, 1e-2, 1e-5, 1e-9, 1e-15, 1e-30, 0.0):
        ei = G.expected_improvement(mu, torch.full_like(mu, sigma), 0.3)
        assert bool(torch.isfinite(ei).all()) and bool((ei >= 0).all()), sigma
        if sigma <= 1e-5:       # 0 <= EI - max(u, 0) <= sigma phi(0)
            assert ((ei - (0.3 - mu).clamp_min(0.0)).abs() <= 0.4 * sigma + 1e-16).all(), sigma


def test_expected_improvement_input_gradient_matches_central_differences():
    """lengthscales >= 0.3 and EI <= 1 keep the third derivatives below ~1e3: truncation h^2 / 6 * 1e3 = 2e-8 at h = 1e-5, rounding
    1e-11; bound 1e-6 absolute on components that reach 1e-2"""
    n, d, h = 10, 3, 1e-5
    X = _rand(n, d, seed=10)
    gp = G.GP(X, ((X - 0.4) ** 2).sum(dim=1), (0.3, 0.6, 0.9), 1e-3)
    Xs = _rand(6, d, seed=11).requires_grad_(True)
    (grad,) = torch.autograd.grad(gp.expected_improvement(Xs).sum(), [Xs])
    worst = 0.0
    for i in range(6):
        for j in range(d):
            e = torch.zeros(6, d, dtype=DT)
            e[i, j] = h
            with torch.no_grad():
                fd = (gp.expected_improvement(Xs + e)[i] - gp.expected_improvement(Xs - e)[i]).item() / (2 * h)
            worst = max(worst, abs(grad[i, j].item() - fd))
    print(f'   EI input gradient: max |autograd - central differences| {worst:.2e} (bound 1e-6), max |grad| {grad.abs().max().item():.2e}')
    assert worst <= 1e-6 and grad.abs().max().item() >= 1e-2


# ---------------------------------------------------------------------------------------------------------------- 6. propose
@pytest.fixture(scope='module')
def fitted():
    X = _rand(12, 6, seed=12)
    return G.GP.fit(X, ((X - 0.35) ** 2).sum(dim=1), seed=0)


@pytest.mark.parametrize('seed', [0, 7])
def test_propose(fitted, seed):
    one, four = fitted.propose(1, seed=seed), fitted.propose(4, seed=seed)
    assert one.shape == (1, 6) and four.shape == (4, 6) and four.dtype == DT
    assert bool(((four >= 0.0) & (four <= 1.0)).all())
    raw = torch.quasirandom.SobolEngine(6, scramble=True, seed=seed).draw(32, dtype=DT)
    ei_raw, ei_got = fitted.expected_improvement(raw).max().item(), fitted.expected_improvement(one).item()
    print(f'   seed {seed}: EI at the proposal {ei_got:.4e}, best of the 32 raw samples {ei_raw:.4e}')
    assert ei_got >= ei_raw > 0.0
    assert ei_got > ei_raw                      # and the refinement climbed: `>=` alone holds for one that returns its best start
    assert torch.equal(four, fitted.propose(4, seed=seed))                      # same seed, same points
    assert torch.equal(four[0], one[0])                                         # the first of a batch is the q = 1 proposal
    dist = torch.cdist(four, four) + 10.0 * torch.eye(4, dtype=DT)
    assert dist.min().item() > 1e-3


# ---------------------------------------------------------------------------------------------------------------- 7 - 9. the script
A_STAR = torch.tensor([0.9, 0.1, 0.8, 0.2, 0.7, 0.3])


class _Bowl:
    """d = 6, accuracy(a) = 1 - |a - a*|^2 / 6, no noise; only what the script needs of an evaluator"""

    def __init__(self):
        self.defense_model = Namespace(model=Namespace(interpolation_alphas=[0.0] * 6))
        self.calls = []

    def objective_many(self, alphas, candidates_per_pass=None):
        assert isinstance(alphas, torch.Tensor) and alphas.dtype == torch.float32
        self.calls.append((alphas.clone(), candidates_per_pass))
        return (1.0 - (alphas - A_STAR).pow(2).sum(dim=1) / 6.0).numpy()


def _run(tmp_path, steps, q, seed, ev):
    from gen_adversarial_amd.experiments.alpha_learning import bayesian_optimization as B
    args = Namespace(n_optimization_steps=steps, candidates_per_round=q, seed=seed, results_folder=str(tmp_path))
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = B.main(args, evaluator=ev)
    return res, out.getvalue()


@pytest.mark.parametrize('q', [1, 5])
@pytest.mark.parametrize('seed', [0, 1, 2, 3, 4])
def test_the_optimiser_beats_random_search_with_the_same_number_of_evaluations(tmp_path, seed, q):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import random_search
    _, rnd = random_search(_Bowl(), 30, seed=seed)
    (_, acc), _ = _run(tmp_path, 25, q, seed, _Bowl())
    print(f'   seed {seed}, q {q}: Bayesian optimisation {acc.max():.5f}, random search {rnd.max():.5f}')
    assert acc.shape == (30, 1) and acc.max() >= rnd.max()


def test_entry_point_files_calls_and_order(tmp_path):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import get_best_combination, get_cosine_alphas, get_linear_alphas
    ev = _Bowl()
    (alphas, acc), printed = _run(tmp_path, 10, 4, 0, ev)
    a, c = np.load(f'{tmp_path}/alphas.npy'), np.load(f'{tmp_path}/accuracies.npy')
    assert a.shape == (15, 6) and c.shape == (15, 1) and a.dtype == c.dtype == np.float32
    assert np.array_equal(a, alphas) and np.array_equal(c, acc)
    cos, lin = get_cosine_alphas(6), get_linear_alphas(6)
    init = torch.tensor([cos, lin, [0.5] * 6, [1 - v for v in lin], [1 - v for v in cos]])
    assert np.array_equal(a[:5], init.numpy())
    assert [(tuple(x.shape), cpp) for x, cpp in ev.calls] == [((5, 6), 5), ((4, 6), 4), ((4, 6), 4), ((2, 6), 2)]
    assert np.array_equal(a, torch.cat([x for x, _ in ev.calls]).numpy())       # stored = handed to the evaluator, in order
    assert np.array_equal(c[:, 0], (1.0 - (torch.from_numpy(a) - A_STAR).pow(2).sum(dim=1) / 6.0).numpy())     # accuracies, not 1 - them
    assert np.array_equal(get_best_combination(str(tmp_path)), a[c[:, 0].argmax()])
    assert (a >= 0.0).all() and (a <= 1.0).all()
    assert 'best alphas:' in printed and f'{c.max()}' in printed


def test_arguments_and_shim(tmp_path):
    from gen_adversarial_amd.experiments.alpha_learning import bayesian_optimization as B
    import src.experiments.alpha_learning.bayesian_optimization as shim
    assert shim.main is B.main and shim.parse_args is B.parse_args
    argv = ['--adv_images_path', 'x', '--n_optimization_steps', '95', '--classifier_path', 'c', '--classifier_type', 'vgg-11',
            '--autoencoder_path', 'a', '--autoencoder_name', 'nvae', '--results_folder', str(tmp_path)]
    args = B.parse_args(argv)
    assert args.results_folder == f'{tmp_path}/nvae_vgg-11/bayesian_optimization/' and os.path.isdir(args.results_folder)
    assert (args.n_optimization_steps, args.seed, args.candidates_per_round, args.batch_images) == (95, 0, None, 8)
    assert (args.adv_images_path, args.classifier_path, args.autoencoder_path, args.autoencoder_name) == ('x', 'c', 'a', 'nvae')
    more = B.parse_args(argv + ['--seed', '3', '--candidates_per_round', '4', '--batch_images', '2'])
    assert (more.seed, more.candidates_per_round, more.batch_images) == (3, 4, 2)
    with pytest.raises(SystemExit):
        B.parse_args([v for v in argv if v not in ('--n_optimization_steps', '95')])
    with pytest.raises(SystemExit):
        B.parse_args(argv[:6] + ['--classifier_type', 'alexnet'] + argv[8:])
