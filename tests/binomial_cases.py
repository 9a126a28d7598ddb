"""Seeded cases and float64 references of the Binomial (logit link) family (CPU only: numpy /
scipy).  Shared by tests/test_binomial_cpu.py (the oracle against the sklearn golden, the host
surface) and tests/test_gpu_binomial.py (the fits on the MI355X).

Objective, as sklearn's HalfBinomialLoss inside the TweedieRegressor objective:

    mean_i [softplus(eta_i) - y_i eta_i] + alpha/2 |w|^2,   eta = X w + b (b unpenalised)

``LogisticRegression(C = 1 / (alpha N))`` minimises N times this, so it has the same minimiser
(tests/golden/make_golden_binomial.py records it; penalty=None at alpha = 0).

Case A: synth.make(N=6000, m=6, L=4, rho=0.08, seed=3, beta_scale=0.5, intercept=-0.5), p = 48,
Bernoulli labels, alpha in {0, 1e-4, 1e-2, 1}.
Case S: the seed-5 design of the same shape at N = 4000 with the deterministic threshold labels
y = 1[X w* > 0.25] (w* the design's true coefficients), alpha = 1e-4: separable, so only the
penalty keeps the optimum finite -- there |eta| reaches 33 and the weights h fall to 6e-15
(max |w| = 10.2): vanishing weights at the smallest shape that has them.
"""
from functools import lru_cache

import numpy as np
import scipy.linalg

ALPHAS_A = (0.0, 1e-4, 1e-2, 1.0)
ALPHA_S = 1e-4
NEWTON_TOL = 1e-13


def sigmoid(eta):
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def loss(y, eta):
    """Per-row half-binomial loss softplus(eta) - y eta."""
    return np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))) - y * eta


def deviance(y, eta):
    """Summed loss (the loss constant of 0/1 labels is 0)."""
    return float(np.sum(loss(y, eta)))


def null_deviance(y):
    """Summed loss at eta = logit(mean y), closed form from the counts."""
    n, ym = y.size, float(np.mean(y))
    if not 0.0 < ym < 1.0:
        return 0.0
    return -n * (ym * np.log(ym) + (1.0 - ym) * np.log1p(-ym))


def d2(y, eta):
    """Fraction of binomial deviance explained."""
    return 1.0 - deviance(y, eta) / null_deviance(y)


def neg_mse(y, eta):
    return -float(np.mean((y - sigmoid(eta)) ** 2))


def fit_binomial_newton(X, y, alpha, fit_intercept=True, coef0=None, tol=NEWTON_TOL, max_iter=200):
    """Float64 damped Newton on the objective above.  Start: w = 0, b = logit(mean y) (or
    ``coef0``, the augmented vector [w, b]).  Armijo backtracking with sklearn's constants
    beta = 1/2, sigma = 2^-11 (as oracle/glm_ref.fit_tweedie_newton).  Stops when the step is
    below tol (1 + |coef|_inf) or max |grad| <= tol / 1000.  Returns (w, b)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
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
        ym = y.mean()
        coef[-1] = np.log(ym / (1.0 - ym))

    def objective(c, eta):
        return loss(y, eta).mean() + 0.5 * np.dot(pen * c, c)

    eta = Xa @ coef
    for _ in range(max_iter):
        mu = sigmoid(eta)
        grad = Xa.T @ (mu - y) / n + pen * coef
        if np.max(np.abs(grad)) <= tol * 1e-3:
            break
        e = np.exp(-np.abs(eta))
        h = e / (1.0 + e) ** 2
        H = (Xa * h[:, None]).T @ Xa / n
        H[np.diag_indices_from(H)] += pen
        try:
            step = -scipy.linalg.cho_solve(scipy.linalg.cho_factor(H), grad)
        except np.linalg.LinAlgError:
            step = -scipy.linalg.lstsq(H, grad)[0]
        f0 = objective(coef, eta)
        gs = float(grad @ step)
        d_eta = Xa @ step
        t = 1.0
        for _ in range(40):
            f1 = objective(coef + t * step, eta + t * d_eta)
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


# ------------------------------------------------------------------------------ cases
@lru_cache(maxsize=None)
def case_a():
    """(Synthetic, X [6000][48] float64, y in {0, 1})."""
    from sglm_hip import synth
    s = synth.make(N=6000, m=6, L=4, family="binomial", rho=0.08, seed=3, beta_scale=0.5,
                   intercept=-0.5)
    X = s.dense_X()
    X.setflags(write=False)
    s.y.setflags(write=False)
    return s, X, s.y


@lru_cache(maxsize=None)
def case_s():
    """(Synthetic, X [4000][48] float64, y = 1[X w* > 0.25])."""
    from sglm_hip import synth
    s = synth.make(N=4000, m=6, L=4, family="binomial", rho=0.08, seed=5, beta_scale=0.5,
                   intercept=-0.5)
    X = s.dense_X()
    y = (X @ s.beta > 0.25).astype(np.float64)
    X.setflags(write=False)
    y.setflags(write=False)
    return s, X, y


@lru_cache(maxsize=None)
def case_mixed():
    """Case A with one continuous column appended (a mixed 0/1 + continuous design), labels
    drawn from the predictor with that column in it.  (X [6000][49], y)."""
    s, X, _ = case_a()
    rng = np.random.default_rng(17)
    c = rng.normal(0.0, 1.0, X.shape[0])
    Xm = np.hstack([X, c[:, None]])
    eta = X @ s.beta + s.intercept + 0.7 * c
    y = (rng.random(X.shape[0]) < sigmoid(eta)).astype(np.float64)
    Xm.setflags(write=False)
    y.setflags(write=False)
    return Xm, y


@lru_cache(maxsize=None)
def oracle(case, alpha, fit_intercept=True):
    """Cached oracle fit (w, b) of a named case: 'A', 'S' or 'M' (mixed)."""
    X, y = {"A": lambda: case_a()[1:], "S": lambda: case_s()[1:], "M": case_mixed}[case]()
    w, b = fit_binomial_newton(X, y, alpha, fit_intercept)
    w.setflags(write=False)
    return w, b


def group_folds(n, k=3, block=100):
    """k group folds over trial blocks of ``block`` rows (trial t -> fold t mod k):
    [(train rows, test rows)]."""
    fold = (np.arange(n) // block) % k
    return [(np.flatnonzero(fold != f), np.flatnonzero(fold == f)) for f in range(k)]


@lru_cache(maxsize=None)
def oracle_rows(alpha, fold, roll=0):
    """Oracle fit on the training rows of one group fold of Case A (fold = -1: every row), with
    the response rolled by ``roll`` rows (np.roll, as the CV drivers shift it)."""
    _, X, y = case_a()
    yr = np.roll(y, roll)
    rows = np.arange(X.shape[0]) if fold < 0 else group_folds(X.shape[0])[fold][0]
    w, b = fit_binomial_newton(X[rows], yr[rows], alpha)
    w.setflags(write=False)
    return w, b
