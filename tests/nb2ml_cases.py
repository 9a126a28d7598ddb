"""CPU oracle of the NB2 dispersion estimate and of the count log-likelihoods (numpy / scipy /
mpmath; no GPU).  Shared by tests/test_nb2ml_cpu.py and the GPU tests of the same feature.

With integer counts y, mu = exp(eta), x = kappa mu and nb2_cases.loss = l_k:

    log p(y) = -l_k(y, eta) + S(y, k) - lgamma(y + 1),   S = sum_{j < y} log1p(k j)
    d/dk log p = S'(y, k) + mu^2 g(x) - y mu / (1 + x),   S' = sum_{j < y} j / (1 + k j),
    g(x) = (log1p(x) - x / (1 + x)) / x^2 = 1/2 - 2x/3 + 3x^2/4 - ...

The likelihoods come from scipy.stats (nbinom / poisson logpmf, the Bernoulli form); the score is
evaluated in np.longdouble in the form above; the profile maximiser is scipy's brentq in ln kappa;
``fit_ml`` alternates it with nb2_cases.fit_nb2_newton, once run to |d ln kappa| <= 1e-13 without
rounding ("exact") and once with the product's float32 rounding and stop rule.
"""
from functools import lru_cache

import numpy as np
import scipy.optimize
import scipy.stats

import nb2_cases as N

KAPPA_LO, KAPPA_HI = 2.0 ** -20, 2.0 ** 10
START_LO, START_HI = 2.0 ** -6, 2.0 ** 6
ML_TOL, ML_MAX_ROUNDS = 2.0 ** -20, 25
LD = np.longdouble


def tail(y, m=None):
    """T[j] = sum_i m_i [y_i > j], j = 0 .. max y - 1 (float64; exact integers)."""
    y = np.asarray(y)
    h = np.bincount(y.astype(np.int64), weights=None if m is None else np.asarray(m, float))
    return np.cumsum(h[::-1])[::-1][1:].astype(np.float64)


# ------------------------------------------------------------------------------ likelihoods
def ll_nb2_rows(kappa, y, eta):
    return scipy.stats.nbinom.logpmf(y, 1.0 / kappa, 1.0 / (1.0 + kappa * np.exp(eta)))


def ll_poisson_rows(y, eta):
    return scipy.stats.poisson.logpmf(y, np.exp(eta))


def ll_binomial_rows(y, eta):
    return y * eta - N.softplus(eta)


def ll_nb2_tail(kappa, y, eta, m=None):
    """Summed NB2 log-likelihood in the tail-histogram form (float64)."""
    w = 1.0 if m is None else np.asarray(m, float)
    T = tail(y, m)
    j = np.arange(T.size, dtype=np.float64)
    return float(-np.sum(w * N.loss(kappa, y, eta))
                 + np.sum(T * (np.log1p(kappa * j) - np.log(j + 1.0))))


def ll_poisson_tail(y, eta, m=None):
    w = 1.0 if m is None else np.asarray(m, float)
    T = tail(y, m)
    return float(-np.sum(w * (np.exp(eta) - y * eta)) - np.sum(T * np.log(np.arange(T.size) + 1.0)))


# ------------------------------------------------------------------------------ the score
def g_ld(x):
    """g(x) in longdouble: a 40-term series below 1/8, the closed form above."""
    x = np.asarray(x, dtype=LD)
    small = x < LD(0.125)
    xs = np.where(small, x, LD(0))
    acc = np.zeros_like(xs)
    for k in range(39, -1, -1):
        acc = acc * xs + LD((-1) ** k) * LD(k + 1) / LD(k + 2)
    xl = np.where(small, LD(1), x)
    big = (np.log1p(xl) - xl / (1 + xl)) / (xl * xl)
    return np.where(small, acc, big)


def score_terms(kappa, y, eta, m=None):
    """Per-row terms of the eta-dependent sums, longdouble, from float64 (or f32) inputs:
    (y eta, (y + 1/k) log1p(k mu), mu^2 g(k mu), y mu / (1 + k mu)), each times m."""
    k = LD(kappa)
    y = np.asarray(y, dtype=LD)
    e = np.asarray(eta, dtype=LD)
    w = LD(1) if m is None else np.asarray(m, dtype=LD)
    mu = np.exp(e)
    x = k * mu
    small = x < LD(0.125)
    # mu^2 g: the series side forms mu^2 (mu < 1 / (8 k)), the other (..) / k^2 -- no overflow
    xl = np.where(small, LD(1), x)
    t_big = (np.log1p(xl) - xl / (1 + xl)) / (k * k)
    mus = np.where(small, mu, LD(0))
    t_small = mus * mus * g_ld(np.where(small, x, LD(0)))
    return (w * y * e, w * (y + 1 / k) * np.log1p(x), w * np.where(small, t_small, t_big),
            w * y * mu / (1 + x))


def eta_sums(kappa, y, eta, m=None):
    """(sum m (y eta - (y + 1/k) log1p(k mu)), sum m (mu^2 g - y mu / (1 + k mu))) and the sums
    of the terms' magnitudes, longdouble."""
    a, b, c, d = score_terms(kappa, y, eta, m)
    return ((a - b).sum(), (c - d).sum()), (np.abs(a).sum() + np.abs(b).sum(),
                                           np.abs(c).sum() + np.abs(d).sum())


def score(kappa, y, eta, m=None):
    """d/dk of the summed log-likelihood at fixed eta, longdouble, cancellation-free."""
    T = tail(y, m).astype(LD)
    j = np.arange(T.size, dtype=LD)
    return (T * j / (1 + LD(kappa) * j)).sum() + eta_sums(kappa, y, eta, m)[0][1]


def score_digamma(kappa, y, eta):
    """The textbook form in float64 (scipy digamma): loses digits towards the Poisson limit."""
    from scipy.special import digamma
    mu = np.exp(eta)
    return float(np.sum(-(digamma(y + 1 / kappa) - digamma(1 / kappa)) / kappa ** 2 + y / kappa
                        + np.log1p(kappa * mu) / kappa ** 2
                        - (y + 1 / kappa) * mu / (1 + kappa * mu)))


def score_mp(kappa, y, eta, dps=50):
    """The same textbook form at ``dps`` digits (mpmath)."""
    import mpmath as mp
    with mp.workdps(dps):
        k = mp.mpf(float(kappa))
        tot = mp.mpf(0)
        for yi, ei in zip(y, eta):
            yi, mu = mp.mpf(float(yi)), mp.exp(mp.mpf(float(ei)))
            tot += (-(mp.digamma(yi + 1 / k) - mp.digamma(1 / k)) / k ** 2 + yi / k
                    + mp.log1p(k * mu) / k ** 2 - (yi + 1 / k) * mu / (1 + k * mu))
        return tot


# ------------------------------------------------------------------------------ the profile
def kappa_profile(y, eta, m=None):
    """(kappa, at_bound): the root of the score over ln kappa in [ln 2^-20, ln 2^10] by brentq;
    score <= 0 at the lower end (no over-dispersion) or >= 0 at the upper end: that bound."""
    if score(KAPPA_LO, y, eta, m) <= 0:
        return KAPPA_LO, True
    if score(KAPPA_HI, y, eta, m) >= 0:
        return KAPPA_HI, True
    th = scipy.optimize.brentq(lambda t: float(score(np.exp(t), y, eta, m)), np.log(KAPPA_LO),
                               np.log(KAPPA_HI), xtol=1e-15, rtol=4 * np.finfo(float).eps)
    return float(np.exp(th)), False


def moment_kappa(y):
    """(s^2 - ybar) / ybar^2 (population variance), clipped to [2^-6, 2^6]."""
    ym = float(np.mean(y))
    k = (float(np.var(y)) - ym) / (ym * ym) if ym > 0 else START_LO
    return float(min(max(k, START_LO), START_HI)) if np.isfinite(k) else START_LO


def fit_ml(X, y, alpha, exact, fit_intercept=True):
    """The alternation: fit at kappa_fit (nb2_cases.fit_nb2_newton, warm-started), kappa* =
    kappa_profile at that fit's predictor, until |ln kappa* - ln kappa_fit| <= tol.
    ``exact``: no rounding, tol 1e-13, up to 200 rounds.  Otherwise the product's rule: kappa_fit
    rounded to float32, tol 2^-20, at most 25 rounds.
    Returns dict(kappa (the value of the last fit), kappa_star, w, b, rounds, converged,
    at_bound)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    tol, rounds = (1e-13, 200) if exact else (ML_TOL, ML_MAX_ROUNDS)
    kappa = moment_kappa(y)
    coef0 = None
    converged = False
    for rnd in range(1, rounds + 1):
        kfit = kappa if exact else N.k32(kappa)
        w, b = N.fit_nb2_newton(X, y, alpha, kfit, fit_intercept, coef0=coef0)
        kappa, at_bound = kappa_profile(y, X @ w + b)
        if abs(np.log(kappa) - np.log(kfit)) <= tol:
            converged = True
            break
        coef0 = np.append(w, b) if fit_intercept else w
    return dict(kappa=kfit, kappa_star=kappa, w=w, b=b, rounds=rnd, converged=converged,
                at_bound=at_bound)


# ------------------------------------------------------------------------------ cases
@lru_cache(maxsize=None)
def case_low():
    """Case A's design with counts generated at kappa = 0.02 (rng 41): (X, y).  The moment
    start is far from the optimum, so the alternation takes several rounds."""
    s, X, _ = N.case_a()
    rng = np.random.default_rng(41)
    mu = np.exp(X @ s.beta + s.intercept)
    y = rng.poisson(mu * rng.gamma(1.0 / 0.02, 0.02, X.shape[0])).astype(np.float64)
    y.setflags(write=False)
    return X, y


@lru_cache(maxsize=None)
def case_poisson():
    """Poisson counts on Case A's predictor (rng 43): no over-dispersion.  (X, y)."""
    s, X, _ = N.case_a()
    y = np.random.default_rng(43).poisson(np.exp(X @ s.beta + s.intercept)).astype(np.float64)
    y.setflags(write=False)
    return X, y


def ml_case(name):
    """(X, y, alpha) of a named ML case: 'A0', 'A2' (alpha 1e-2), 'A1' (alpha 1), 'T', 'L',
    'P' (the Poisson limit)."""
    if name in ("A0", "A2", "A1"):
        _, X, y = N.case_a()
        return X, y, {"A0": 0.0, "A2": 1e-2, "A1": 1.0}[name]
    if name == "T":
        _, X, y = N.case_t()
        return X, y, N.ALPHA_T
    if name == "L":
        X, y = case_low()
        return X, y, 1e-2
    if name == "P":
        X, y = case_poisson()
        return X, y, 1e-4
    raise KeyError(name)


@lru_cache(maxsize=None)
def ml_oracle(name, exact):
    X, y, alpha = ml_case(name)
    return fit_ml(X, y, alpha, exact)


GRID_KAPPAS = (0.1, 0.25, 0.5, 1.0, 2.0)
GRID_ALPHA = 1e-2


@lru_cache(maxsize=None)
def grid_oracle(kappa):
    """Per group fold of Case A at (GRID_ALPHA, kappa; kappa None = Poisson): the oracle's mean
    train and test log-likelihood at the oracle's coefficients.  ([train], [test])."""
    _, X, y = N.case_a()
    tr_s, te_s = [], []
    for f, (tr, te) in enumerate(N.group_folds(X.shape[0])):
        if kappa is None:
            from oracle import glm_ref
            w, b = glm_ref.fit_tweedie_newton(X[tr], y[tr], GRID_ALPHA, 1.0)
            rows = lambda r: ll_poisson_rows(y[r], X[r] @ w + b)      # noqa: E731
        else:
            w, b = N.oracle_rows(GRID_ALPHA, kappa, f)
            rows = lambda r: ll_nb2_rows(N.k32(kappa), y[r], X[r] @ w + b)   # noqa: E731
        tr_s.append(float(np.mean(rows(tr))))
        te_s.append(float(np.mean(rows(te))))
    return tr_s, te_s
