"""Seeded cases and float64 references of the negative-binomial family (NB2, log link, fixed
dispersion kappa; CPU only: numpy / scipy).  Shared by tests/test_nb2_cpu.py (the oracle against
scipy, the host surface) and tests/test_gpu_nb2.py (the fits on the MI355X).

Objective, TweedieRegressor's mean-scaled one with the NB2 loss (Var y = mu + kappa mu^2):

    mean_i l(y_i, eta_i) + alpha/2 |w|^2,   eta = X w + b (b unpenalised), mu = exp(eta),
    l(y, eta) = (y + 1/kappa) log(1 + kappa e^eta) - y eta

l is the negative log-likelihood up to terms free of eta; kappa -> 0 gives Poisson's
e^eta - y eta.  The dispersion every layer uses is kappa rounded to float32 (``k32``): the C ABI
carries it in a float, so the oracle runs at that value too.

Case A: synth.make(N=6000, m=6, L=4, family='nb2', rho=0.08, seed=3, beta_scale=0.5,
intercept=-0.5, kappa=0.5), p = 48, Gamma-Poisson counts; fitted at kappa in {0.25, 1.0, 0.3}
(0.3 is not float32-exact), alpha in {0, 1e-4, 1e-2, 1}, with and without intercept.
Case T: the seed-5 design at N = 4000 with intercept 1.5 and kappa = 8 (generating and fitted),
alpha = 1e-4: a large-mu tail, kappa mu >= 100 on some rows at the optimum, where
sigma(eta + ln kappa) saturates and the weights mu (1 + kappa y) / (1 + kappa mu)^2 collapse.
Case Z: Case A's data at kappa = 2^-16, alpha = 1e-2: the Poisson limit.
Case M: Case A with one continuous column appended, counts drawn with that column in the
predictor.
"""
from functools import lru_cache

import numpy as np
import scipy.linalg

ALPHAS_A = (0.0, 1e-4, 1e-2, 1.0)
KAPPAS_A = (0.25, 1.0, 0.3)
KAPPA_GEN = 0.5
KAPPA_T, ALPHA_T = 8.0, 1e-4
KAPPA_Z, ALPHA_Z = 2.0 ** -16, 1e-2
ALPHA_M, KAPPA_M = 1e-4, 0.25
NEWTON_TOL = 1e-13


def k32(kappa):
    """kappa as the engine uses it: rounded to float32 once."""
    return float(np.float32(kappa))


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def loss(kappa, y, eta):
    """Per-row NB2 loss (y + 1/kappa) softplus(eta + ln kappa) - y eta."""
    return (y + 1.0 / kappa) * softplus(eta + np.log(kappa)) - y * eta


def constant(kappa, y):
    """Saturated constant c(y) = y ln y - (y + 1/kappa) ln(1 + kappa y), 0 at y = 0:
    loss + c >= 0 with equality at mu = y."""
    y = np.asarray(y, dtype=np.float64)
    ys = np.where(y > 0, y, 1.0)
    return np.where(y > 0, ys * np.log(ys) - (ys + 1.0 / kappa) * np.log1p(kappa * ys), 0.0)


def deviance(kappa, y, eta):
    """Summed loss + constant (half the NB2 deviance)."""
    return float(np.sum(loss(kappa, y, eta)) + np.sum(constant(kappa, y)))


def null_loss(kappa, y):
    """Summed loss at eta = log(mean y), closed form from the count and the sum."""
    cnt, sy = float(y.size), float(np.sum(y))
    ym = sy / cnt
    return (sy + cnt / kappa) * np.log1p(kappa * ym) - sy * np.log(ym)


def d2(kappa, y, eta):
    """Fraction of NB2 deviance explained: 1 - (sum l + sum c) / (null + sum c)."""
    c = float(np.sum(constant(kappa, y)))
    return 1.0 - (float(np.sum(loss(kappa, y, eta))) + c) / (null_loss(kappa, y) + c)


def neg_mse(y, eta):
    return -float(np.mean((y - np.exp(eta)) ** 2))


def objective(kappa, X, y, alpha, w, b):
    return float(np.mean(loss(kappa, y, X @ w + b)) + 0.5 * alpha * np.dot(w, w))


def fit_nb2_newton(X, y, alpha, kappa, fit_intercept=True, coef0=None, tol=NEWTON_TOL,
                   max_iter=200):
    """Float64 damped Newton on the objective above with the exact Hessian.  Start: w = 0,
    b = log(mean y) (or ``coef0``, the augmented vector [w, b]).  Armijo backtracking with
    sklearn's constants beta = 1/2, sigma = 2^-11 and the stopping rule of
    binomial_cases.fit_binomial_newton: the step below tol (1 + |coef|_inf) or max |grad| <=
    tol / 1000.  Returns (w, b)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    kappa = float(kappa)
    n = X.shape[0]
    Xa = np.hstack([X, np.ones((n, 1))]) if fit_intercept else X
    pa = Xa.shape[1]
    pen = np.full(pa, float(alpha))
    if fit_intercept:
        pen[-1] = 0.0
    coef = np.zeros(pa)
    if coef0 is not None:
        coef[:] = coef0
    elif fit_intercept:
        coef[-1] = np.log(y.mean())
    f = y + 1.0 / kappa
    lk = np.log(kappa)

    def obj(c, eta):
        return loss(kappa, y, eta).mean() + 0.5 * np.dot(pen * c, c)

    eta = Xa @ coef
    for _ in range(max_iter):
        q = sigmoid(eta + lk)
        grad = Xa.T @ (f * q - y) / n + pen * coef
        if np.max(np.abs(grad)) <= tol * 1e-3:
            break
        e = np.exp(-np.abs(eta + lk))
        h = f * e / (1.0 + e) ** 2
        H = (Xa * h[:, None]).T @ Xa / n
        H[np.diag_indices_from(H)] += pen
        try:
            step = -scipy.linalg.cho_solve(scipy.linalg.cho_factor(H), grad)
        except np.linalg.LinAlgError:
            step = -scipy.linalg.lstsq(H, grad)[0]
        f0 = obj(coef, eta)
        gs = float(grad @ step)
        d_eta = Xa @ step
        t = 1.0
        for _ in range(40):
            f1 = obj(coef + t * step, eta + t * d_eta)
            if f1 - f0 <= 2.0 ** -11 * t * gs or abs(f1 - f0) <= 1e-16 * abs(f0):
                break
            t *= 0.5
        coef = coef + t * step
        eta = eta + t * d_eta
        if np.max(np.abs(t * step)) <= tol * (1 + np.max(np.abs(coef))):
            break
    if fit_intercept:
        return coef[:-1].copy(), float(coef[-1])
    return coef.copy(), 0.0


def gradient(kappa, X, y, alpha, w, b, fit_intercept=True):
    """max |gradient| of the objective at (w, b) (the intercept's component included)."""
    eta = X @ w + b
    r = (y + 1.0 / kappa) * sigmoid(eta + np.log(kappa)) - y
    g = X.T @ r / X.shape[0] + alpha * w
    return max(float(np.max(np.abs(g))), abs(float(r.mean())) if fit_intercept else 0.0)


# ------------------------------------------------------------------------------ cases
def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)


@lru_cache(maxsize=None)
def case_a():
    """(Synthetic, X [6000][48] float64, y counts)."""
    from sglm_hip import synth
    s = synth.make(N=6000, m=6, L=4, family="nb2", rho=0.08, seed=3, beta_scale=0.5,
                   intercept=-0.5, kappa=KAPPA_GEN)
    X = s.dense_X()
    _frozen(X, s.y)
    return s, X, s.y


@lru_cache(maxsize=None)
def case_t():
    """(Synthetic, X [4000][48] float64, y counts with a large-mu tail), kappa = 8."""
    from sglm_hip import synth
    s = synth.make(N=4000, m=6, L=4, family="nb2", rho=0.08, seed=5, beta_scale=0.5,
                   intercept=1.5, kappa=KAPPA_T)
    X = s.dense_X()
    _frozen(X, s.y)
    return s, X, s.y


@lru_cache(maxsize=None)
def case_mixed():
    """Case A with one continuous column appended (a mixed 0/1 + continuous design), counts
    drawn from the predictor with that column in it.  (X [6000][49], y)."""
    s, X, _ = case_a()
    rng = np.random.default_rng(17)
    c = rng.normal(0.0, 1.0, X.shape[0])
    Xm = np.hstack([X, c[:, None]])
    mu = np.exp(X @ s.beta + s.intercept + 0.4 * c)
    y = rng.poisson(mu * rng.gamma(1.0 / KAPPA_GEN, KAPPA_GEN, X.shape[0])).astype(np.float64)
    _frozen(Xm, y)
    return Xm, y


@lru_cache(maxsize=None)
def oracle(case, alpha, kappa, fit_intercept=True):
    """Cached oracle fit (w, b) of a named case -- 'A', 'T', 'Z' (Case A's data) or 'M' -- at
    float32-rounded kappa."""
    X, y = {"A": lambda: case_a()[1:], "T": lambda: case_t()[1:], "Z": lambda: case_a()[1:],
            "M": case_mixed}[case]()
    w, b = fit_nb2_newton(X, y, alpha, k32(kappa), fit_intercept)
    w.setflags(write=False)
    return w, b


def group_folds(n, k=3, block=100):
    """k group folds over trial blocks of ``block`` rows (trial t -> fold t mod k):
    [(train rows, test rows)]."""
    fold = (np.arange(n) // block) % k
    return [(np.flatnonzero(fold != f), np.flatnonzero(fold == f)) for f in range(k)]


@lru_cache(maxsize=None)
def oracle_rows(alpha, kappa, fold, roll=0):
    """Oracle fit on the training rows of one group fold of Case A (fold = -1: every row), with
    the response rolled by ``roll`` rows (np.roll, as the CV drivers shift it)."""
    _, X, y = case_a()
    yr = np.roll(y, roll)
    rows = np.arange(X.shape[0]) if fold < 0 else group_folds(X.shape[0])[fold][0]
    w, b = fit_nb2_newton(X[rows], yr[rows], alpha, k32(kappa))
    w.setflags(write=False)
    return w, b
