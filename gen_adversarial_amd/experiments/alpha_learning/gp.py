"""
The surrogate of the Bayesian optimisation of the alphas (bayesian_optimization.py): a small exact Gaussian process in float64 on
the CPU, torch only.  It stands where the reference has BoTorch's `SingleTaskGP` + `fit_gpytorch_mll` + `ExpectedImprovement` +
`optimize_acqf` (src/experiments/alpha_learning/bayesian_optimization.py:79-99).  It is this project's own surrogate: the same kind
of model and the same counts (32 raw samples, 8 restarts), not a reproduction of BoTorch's numbers.

Model: constant mean, ARD squared-exponential kernel without an output scale over inputs in [0,1]^d, homoskedastic Gaussian noise,
targets standardised to zero mean and unit variance (standard deviation 1 when all targets are equal).  The hyper-parameters — d
log-lengthscales, the log of the noise variance above its floor of 1e-6, the mean — live on the standardised scale and are fitted by
MAP: exact marginal log-likelihood + LogNormal(sqrt 2 + ln(d) / 2, sqrt 3) on every lengthscale + LogNormal(-4, 1) on the noise
variance, L-BFGS (strong Wolfe) from the prior modes and from a few seeded random starts, the best kept.

A model is at most ~200 points in at most 24 dimensions: every kernel matrix is built from plain differences and factored once.
"""
from __future__ import annotations

import math

import torch

RAW_SAMPLES, NUM_RESTARTS = 32, 8       # optimize_acqf(raw_samples=32, num_restarts=8), bayesian_optimization.py:93-99
NOISE_FLOOR = 1e-6
NOISE_PRIOR = (-4.0, 1.0)
_DT = torch.float64
_SQRT2, _SQRT_2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def _t64(a) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.detach().to('cpu', _DT)
    return torch.as_tensor(a, dtype=_DT)                # Python floats go to double directly, not through float32


def lengthscale_prior(d: int):
    """(mu, sigma) of the LogNormal prior on every lengthscale: grows with sqrt(d), so few points in many dimensions fit smoothly"""
    return _SQRT2 + 0.5 * math.log(d), math.sqrt(3.0)


def lognormal_log_prob(x: torch.Tensor, mu: float, sigma: float) -> torch.Tensor:
    lx = torch.log(x)
    return -lx - math.log(sigma * _SQRT_2PI) - (lx - mu) ** 2 / (2.0 * sigma ** 2)


def ard_se_kernel(A: torch.Tensor, B: torch.Tensor, lengthscale: torch.Tensor) -> torch.Tensor:
    """[n, d], [m, d] -> [n, m]: exp(-1/2 sum_j ((a_j - b_j) / l_j)^2)"""
    diff = (A / lengthscale).unsqueeze(1) - (B / lengthscale).unsqueeze(0)
    return torch.exp(-0.5 * diff.pow(2).sum(dim=2))


def pack(lengthscale, noise, mean) -> torch.Tensor:
    """(lengthscales [d], noise variance, mean) -> theta [d + 2]"""
    ls, nz = _t64(lengthscale).reshape(-1), _t64(noise).reshape(1)
    if not bool((nz > NOISE_FLOOR).all()):
        raise ValueError(f'the noise variance must exceed its floor of {NOISE_FLOOR}')
    return torch.cat([ls.log(), (nz - NOISE_FLOOR).log(), _t64(mean).reshape(1)])


def unpack(theta: torch.Tensor, d: int):
    return theta[:d].exp(), NOISE_FLOOR + theta[d].exp(), theta[d + 1]


def prior_mode_theta(d: int) -> torch.Tensor:
    """the modes exp(mu - sigma^2) of the two priors, mean 0"""
    mu, sigma = lengthscale_prior(d)
    return pack(torch.full((d,), math.exp(mu - sigma ** 2)), math.exp(NOISE_PRIOR[0] - NOISE_PRIOR[1] ** 2), 0.0)


def neg_log_posterior(theta: torch.Tensor, X: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """the MAP objective to minimise: -(log N(z; mean, K + noise I) + log priors), z the standardised targets"""
    n, d = X.shape
    ls, noise, mean = unpack(theta, d)
    L = torch.linalg.cholesky(ard_se_kernel(X, X, ls) + noise * torch.eye(n, dtype=_DT))
    r = (z - mean).unsqueeze(1)
    mll = -0.5 * (r * torch.cholesky_solve(r, L)).sum() - L.diagonal().log().sum() - 0.5 * n * math.log(2.0 * math.pi)
    return -(mll + lognormal_log_prob(ls, *lengthscale_prior(d)).sum() + lognormal_log_prob(noise, *NOISE_PRIOR))


def normal_cdf(z: torch.Tensor) -> torch.Tensor:
    return 0.5 * torch.special.erfc(-z / _SQRT2)


def normal_pdf(z: torch.Tensor) -> torch.Tensor:
    return torch.exp(-0.5 * z * z) / _SQRT_2PI


def expected_improvement(mean: torch.Tensor, sigma: torch.Tensor, best_f) -> torch.Tensor:
    """E max(best_f - f, 0) for f ~ N(mean, sigma^2) = sigma (z Phi(z) + phi(z)), z = (best_f - mean) / sigma.  Below z = -1 the sum
    cancels; there it is phi(z) (1 + z Phi(z) / phi(z)) with the Mills ratio Phi / phi = sqrt(pi / 2) erfcx(-z / sqrt 2)."""
    sigma = sigma.clamp_min(1e-30)
    z = (best_f - mean) / sigma
    zp, zn = z.clamp_min(-1.0), z.clamp_max(-1.0)               # each branch sees only arguments it is finite for
    body = zp * normal_cdf(zp) + normal_pdf(zp)
    tail = normal_pdf(zn) * (1.0 + zn * math.sqrt(math.pi / 2.0) * torch.special.erfcx(-zn / _SQRT2))
    return sigma * torch.where(z < -1.0, tail.clamp_min(0.0), body)


class GP:
    """exact GP on (X [n, d] in [0,1]^d, y [n]) with the given hyper-parameters (standardised scale); `GP.fit` finds them.
    `standardize` = (offset, scale) of the targets, by default their mean and standard deviation: `condition_on` keeps the pair of
    the model it extends, since the hyper-parameters are expressed on that scale."""

    def __init__(self, X, y, lengthscale=None, noise=None, mean=0.0, standardize=None, best_f=None, theta=None):
        self.X, self.y = _t64(X), _t64(y).reshape(-1)
        if self.X.dim() != 2 or self.X.shape[0] != self.y.shape[0] or self.y.shape[0] == 0:
            raise ValueError(f'X [n, d] and y [n] expected, got {tuple(self.X.shape)} and {tuple(self.y.shape)}')
        self.n, self.d = self.X.shape
        self.theta = pack(lengthscale, noise, mean) if theta is None else _t64(theta).reshape(-1)      # theta: the packed form, as is
        if self.theta.shape[0] != self.d + 2:
            raise ValueError(f'{self.d} lengthscales expected')
        self.y_mean, self.y_std = standardize_constants(self.y) if standardize is None else (float(standardize[0]), float(standardize[1]))
        self.best_f = float(self.y.min()) if best_f is None else float(best_f)
        self.lengthscale, self.noise, self.mean = unpack(self.theta, self.d)
        self.z = (self.y - self.y_mean) / self.y_std
        self.L = torch.linalg.cholesky(ard_se_kernel(self.X, self.X, self.lengthscale) + self.noise * torch.eye(self.n, dtype=_DT))
        self.weights = torch.cholesky_solve((self.z - self.mean).unsqueeze(1), self.L).squeeze(1)        # (K + noise I)^-1 (z - mean)

    @property
    def standardize(self):
        return self.y_mean, self.y_std

    def map_objective(self, theta: torch.Tensor = None) -> torch.Tensor:
        """the MAP objective of this model's data at `theta` (default: its own hyper-parameters); differentiable in theta"""
        return neg_log_posterior(self.theta if theta is None else theta, self.X, self.z)

    @classmethod
    def fit(cls, X, y, seed: int = 0, random_starts: int = 2, max_iter: int = 50) -> 'GP':
        X, y = _t64(X), _t64(y).reshape(-1)
        m, s = standardize_constants(y)
        z = (y - m) / s
        d = X.shape[1]
        g = torch.Generator().manual_seed(seed)
        start = prior_mode_theta(d)
        starts = [start] + [start + torch.cat([torch.randn(d + 1, generator=g, dtype=_DT), torch.zeros(1, dtype=_DT)])
                            for _ in range(random_starts)]
        best, best_val = start, math.inf
        for t0 in starts:
            theta = t0.clone().requires_grad_(True)
            opt = torch.optim.LBFGS([theta], lr=1.0, max_iter=max_iter, tolerance_grad=1e-5, tolerance_change=1e-9,
                                    line_search_fn='strong_wolfe')

            def closure():
                opt.zero_grad()
                loss = neg_log_posterior(theta, X, z)
                loss.backward()
                return loss
            try:
                val0 = float(neg_log_posterior(t0, X, z))
                if val0 < best_val:                 # a start itself is a candidate: the result is never worse than the prior modes
                    best, best_val = t0, val0
                with torch.enable_grad():
                    opt.step(closure)
                val = float(neg_log_posterior(theta.detach(), X, z))
            except torch.linalg.LinAlgError:        # K + noise I does not factor here, or the line search left where it does: next start
                continue
            if val < best_val:
                best, best_val = theta.detach().clone(), val
        return cls(X, y, theta=best)

    @torch.no_grad()
    def condition_on(self, x, y) -> 'GP':
        """the model with the observation (x [d], y) appended; hyper-parameters, standardisation and best_f stay"""
        X = torch.cat([self.X, _t64(x).reshape(1, self.d)])
        return GP(X, torch.cat([self.y, _t64(y).reshape(1)]), theta=self.theta, standardize=self.standardize, best_f=self.best_f)

    def posterior(self, X):
        """X [m, d] -> (mean [m], variance [m]) of the latent function, in the units of y; differentiable in X"""
        X = X.to(_DT) if isinstance(X, torch.Tensor) else _t64(X)
        Ks = ard_se_kernel(X, self.X, self.lengthscale)                                  # [m, n]
        v = torch.linalg.solve_triangular(self.L, Ks.t(), upper=False)                   # L^-1 k*
        var = (1.0 - v.pow(2).sum(dim=0)).clamp_min(1e-30)
        return self.y_mean + self.y_std * (self.mean + Ks @ self.weights), self.y_std ** 2 * var

    def expected_improvement(self, X, best_f=None) -> torch.Tensor:
        """analytic EI for minimisation at X [m, d]; best_f defaults to the smallest target the model was built on"""
        mean, var = self.posterior(X)
        return expected_improvement(mean, var.sqrt(), self.best_f if best_f is None else best_f)

    def _best_point(self, raw: torch.Tensor, best_f: float) -> torch.Tensor:
        """the NUM_RESTARTS best of the raw samples by EI, refined together by L-BFGS through x = sigmoid(u); the best of starts and
        refined points (so never worse than the best raw sample)"""
        with torch.no_grad():
            ei_raw = self.expected_improvement(raw, best_f)
        starts = raw[ei_raw.topk(min(NUM_RESTARTS, raw.shape[0])).indices]
        scale = float(ei_raw.max())
        if not scale > 0.0:                         # EI is flat zero over the samples: nothing to climb
            return starts[0]
        u = torch.logit(starts.clamp(1e-6, 1.0 - 1e-6)).requires_grad_(True)
        opt = torch.optim.LBFGS([u], lr=1.0, max_iter=30, tolerance_grad=1e-6, tolerance_change=1e-9, line_search_fn='strong_wolfe')

        def closure():
            opt.zero_grad()
            loss = -self.expected_improvement(torch.sigmoid(u), best_f).sum() / scale      # the starts do not interact: a sum
            loss.backward()
            return loss
        with torch.enable_grad():
            opt.step(closure)
        with torch.no_grad():
            cand = torch.cat([starts, torch.sigmoid(u.detach())])
            ei = torch.nan_to_num(self.expected_improvement(cand, best_f), nan=-1.0)
        return cand[ei.argmax()]

    def propose(self, q: int = 1, seed: int = 0, best_f: float = None) -> torch.Tensor:
        """q points [q, d] in [0,1]^d to evaluate next.  Each is the EI maximiser from 32 fresh points of one seeded Sobol sequence;
        after a point is chosen the model is conditioned on its own posterior mean there (Kriging believer: no refit, best_f
        unchanged) and asked again, so the first point of a batch is the q = 1 proposal."""
        best_f = self.best_f if best_f is None else float(best_f)
        sobol = torch.quasirandom.SobolEngine(self.d, scramble=True, seed=seed)
        model, points = self, []
        for i in range(q):
            x = model._best_point(sobol.draw(RAW_SAMPLES, dtype=_DT), best_f)
            points.append(x)
            if i + 1 < q:
                with torch.no_grad():
                    model = model.condition_on(x, model.posterior(x.unsqueeze(0))[0][0])
        return torch.stack(points)


def standardize_constants(y: torch.Tensor):
    """(mean, standard deviation) of the targets; 1 for the deviation when they are all equal (or there is one)"""
    s = float(y.std()) if float(y.max()) > float(y.min()) else 1.0
    return float(y.mean()), s
