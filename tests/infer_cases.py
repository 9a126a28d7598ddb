"""Cases and the numpy oracle of the inference tests (standard errors, covariance, Wald tests;
DESIGN.md §28).  No engine code: dense float64 X~ by plain indexing, J, M and A in float64, the
inverse and everything after it in np.longdouble (as tests/chol64_cases.py), then the formulas
of the issue.  The oracle takes coefficients as input, so a test that feeds it the engine's
fitted coefficients compares the inference arithmetic alone.

Designs are lagged 0/1 event designs at rate ~0.06 (as glasso_cases), full rank.  The condition
numbers of A = J + Lambda of the GPU cases, from the oracle at the generating coefficients, are
recorded in COND_A (tests/test_infer_cpu.py holds them to the oracle within a factor 2): every
case sits near 40, so an f32-rounded Gram (6e-8 relative) moves A^-1 by a few 1e-6 at most: the
1e-4 / 1e-5 bars have room, and a miss is a defect, not conditioning.
"""
from functools import lru_cache

import numpy as np
import pandas as pd

LD = np.longdouble
U53 = 2.0 ** -53
FAM_SQUARED, FAM_TWEEDIE, FAM_BINOMIAL, FAM_NB2 = 0, 1, 2, 3
KEPT, DEP, EXCL, ZERO = 0, 1, 2, 3


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------ families
def mean_weight_var(fam, power, eta):
    """(mu, v, V): the mean, the Fisher weight (dmu/deta)^2 / V and the variance function."""
    if fam == FAM_SQUARED:
        return eta, np.ones_like(eta), np.ones_like(eta)
    if fam == FAM_BINOMIAL:
        e = np.exp(-np.abs(eta))
        mu = np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
        v = e / (1 + e) ** 2
        return mu, v, v
    mu = np.exp(eta)
    if fam == FAM_NB2:
        return mu, mu / (1 + power * mu), mu + power * mu * mu
    return mu, mu ** (2 - power), mu ** power


def loss(fam, power, y, eta):
    """The per-row loss the engine minimises (half deviance up to terms free of eta)."""
    if fam == FAM_SQUARED:
        return 0.5 * (eta - y) ** 2
    if fam == FAM_BINOMIAL:
        return np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))) - y * eta
    if fam == FAM_NB2:
        z = eta + np.log(ld(power)).astype(eta.dtype)
        return (y + 1 / power) * (np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))) - y * eta
    if power == 1:
        return np.exp(eta) - y * eta
    if power == 2:
        return eta + y * np.exp(-eta)
    return np.exp((2 - power) * eta) / (2 - power) - y * np.exp((1 - power) * eta) / (1 - power)


def score_resid(fam, power, y, eta):
    """s = dloss/deta."""
    mu, v, V = mean_weight_var(fam, power, eta)
    if fam in (FAM_SQUARED, FAM_BINOMIAL):
        return mu - y
    if fam == FAM_NB2:
        return (mu - y) / (1 + power * mu)
    return (mu - y) * mu ** (1 - power)


def score_terms(fam, power, y, eta):
    """(t1, t2) with s = t1 - t2: the two terms whose difference the f32 row pass forms (the
    magnitude (|t1| + |t2|)^2 is what its error in s^2 is relative to)."""
    mu = mean_weight_var(fam, power, eta)[0]
    if fam in (FAM_SQUARED, FAM_BINOMIAL):
        return mu, y
    if fam == FAM_NB2:
        return mu / (1 + power * mu), y / (1 + power * mu)
    return mu ** (2 - power), y * mu ** (1 - power)


def observed_weight(fam, power, y, eta):
    """loss'' (the IRLS weight sglm_link_weights writes): linear in y for every family."""
    mu, v, V = mean_weight_var(fam, power, eta)
    if fam == FAM_NB2:
        return mu * (1 + power * y) / (1 + power * mu) ** 2
    if fam == FAM_TWEEDIE:
        return (2 - power) * mu ** (2 - power) - (1 - power) * y * mu ** (1 - power)
    return v


def draw(rng, fam, power, eta, phi=1.0):
    """Responses from the model at eta (Tweedie 1 < q < 2: compound Poisson-gamma)."""
    mu = mean_weight_var(fam, power, eta)[0]
    if fam == FAM_SQUARED:
        return eta + np.sqrt(phi) * rng.normal(0, 1, eta.shape)
    if fam == FAM_BINOMIAL:
        return (rng.random(eta.shape) < mu).astype(np.float64)
    if fam == FAM_NB2:
        return rng.poisson(mu * rng.gamma(1 / power, power, eta.shape)).astype(np.float64)
    if power == 1:
        return rng.poisson(mu).astype(np.float64)
    if power == 2:
        return rng.gamma(1 / phi, phi * mu)
    N = rng.poisson(mu ** (2 - power) / (phi * (2 - power)))
    a = (2 - power) / (power - 1)
    return np.where(N > 0, rng.gamma(np.maximum(N, 1) * a, phi * (power - 1) * mu ** (power - 1)),
                    0.0)


# ------------------------------------------------------------------------------ linear algebra
def ld_chol_inv(A):
    """(T, R) in np.longdouble with A = R^T R (upper) and T = R^-1; A^-1 = T T^T."""
    A = ld(A).copy()
    n = A.shape[0]
    R = np.zeros((n, n), LD)
    for j in range(n):
        R[j, j] = np.sqrt(A[j, j])
        R[j, j + 1:] = A[j, j + 1:] / R[j, j]
        A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return ld_tri_inv(R), R


def ld_tri_inv(R):
    """Inverse of an upper triangular matrix in np.longdouble (back substitution by rows)."""
    R = ld(R)
    n = R.shape[0]
    T = np.zeros((n, n), LD)
    for i in range(n - 1, -1, -1):
        rhs = -(R[i, i + 1:] @ T[i + 1:, :])
        rhs[i] += 1
        T[i, :] = rhs / R[i, i]
    return T


def ld_inv(A):
    T, _ = ld_chol_inv(A)
    return T @ T.T


def embed(Bk, K, P):
    out = np.zeros((P, P), Bk.dtype)
    out[np.ix_(K, K)] = Bk
    return out


# ------------------------------------------------------------------------------ the oracle
def csr(ids):
    """(group ids ascending, goff, gcols): the CSR of glasso.group_csr, by plain indexing."""
    ids = np.asarray(ids)
    u = np.unique(ids)
    cols = [np.flatnonzero(ids == g) for g in u]
    goff = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    return u, goff, np.concatenate(cols).astype(np.int32)


def covariance(Ainv, J, M, lam_diag, phi, cov_type):
    """C from A^-1 (longdouble): the three covariance types of the issue."""
    if cov_type == "bayes":
        return phi * Ainv
    if cov_type == "robust":
        return Ainv @ ld(M) @ Ainv
    return phi * (Ainv - Ainv @ (ld(lam_diag)[:, None] * Ainv))


def oracle(Xt, y, fam, power, lam, beta, fit_intercept=True, cov_type="model", scale=None,
           groups=None, m=None, s2=None):
    """Inference at coefficients ``beta`` (length p + 1, intercept last) on the dense X~ ``Xt``
    (n x (p + 1), ones column last): a dict with se (p + 1, NaN where not kept), cov, scale, df,
    n, cond (2-norm condition of A on the kept coordinates) and, with ``groups`` (one id per
    coefficient), ids / stat / dof.  ``s2``: the squared score residuals to use in the robust
    meat instead of the sample's."""
    n, P = Xt.shape
    p = P - 1
    m = np.ones(n) if m is None else np.asarray(m, dtype=np.float64)
    eta = Xt @ beta
    mu, v, V = mean_weight_var(fam, power, eta)
    J = Xt.T @ ((m * v)[:, None] * Xt)
    s = score_resid(fam, power, y, eta)
    M = Xt.T @ ((m * (s * s if s2 is None else s2))[:, None] * Xt)
    lam_diag = np.r_[np.full(p, float(lam)), 0.0]
    A = J + np.diag(lam_diag)
    state = np.where(np.diag(A) > 0, KEPT, ZERO)
    if not fit_intercept:
        state[p] = EXCL
    K = np.flatnonzero(state == KEPT)
    Ainv = embed(ld_inv(A[np.ix_(K, K)]), K, P)
    df = LD(K.size) - LD(lam) * np.sum(np.diag(Ainv)[:p])
    nn = LD(m.sum())
    pearson = np.sum(ld(m) * (ld(y) - ld(mu)) ** 2 / ld(V)) / (nn - df)
    unit = fam in (FAM_BINOMIAL, FAM_NB2) or (fam == FAM_TWEEDIE and power == 1)
    phi = pearson if scale == "pearson" else LD(scale) if scale is not None else \
        LD(1) if unit else pearson
    C = covariance(Ainv, J, M, lam_diag, phi, cov_type)
    var = np.diag(C).astype(np.float64)
    var[state != KEPT] = np.nan
    out = dict(se=np.sqrt(var), cov=C.astype(np.float64), scale=float(phi), df=float(df),
               n=float(nn), cond=float(np.linalg.cond(A[np.ix_(K, K)])), state=state,
               Ainv=Ainv, J=J, M=M)
    if groups is not None:
        ids, goff, gcols = csr(groups)
        stat, dof = [], []
        for g in range(len(ids)):
            c = gcols[goff[g]:goff[g + 1]]
            c = c[state[c] == KEPT]
            dof.append(c.size)
            if c.size == 0:
                stat.append(0.0)
                continue
            Tg, _ = ld_chol_inv(C[np.ix_(c, c)])
            z = Tg.T @ ld(beta[c])
            stat.append(float(z @ z))
        out.update(ids=ids, stat=np.array(stat), dof=np.array(dof))
    return out


# ------------------------------------------------------------------------------ designs
def lagged(rng, n, m, L, rate=0.06):
    """(frame of the n x (m L) lagged 0/1 design, group ids): column a L + b is event a delayed
    by b rows, named ev{a} (b = 0) / ev{a}_{b} -- sglm_ez.event_groups' naming."""
    Ev = (rng.random((n, m)) < rate).astype(np.float64)
    X = np.zeros((n, m * L))
    names = []
    for a in range(m):
        for b in range(L):
            X[b:, a * L + b] = Ev[:n - b, a]
            names.append(f"ev{a}" if b == 0 else f"ev{a}_{b}")
    return pd.DataFrame(X, columns=names), np.repeat(np.arange(m), L)


def xt(X):
    X = np.asarray(X, dtype=np.float64)
    return np.hstack([X, np.ones((X.shape[0], 1))])


# name: (family, power / kappa, estimator alpha, intercept of the generating model, phi)
GPU_N, GPU_M, GPU_L = 4000, 6, 21
GPU_FAMILIES = {
    "normal": (FAM_SQUARED, 0.0, 0.0, 1.0, 0.49),
    "ridge": (FAM_SQUARED, 0.0, 25.0, 1.0, 0.49),
    "poisson": (FAM_TWEEDIE, 1.0, 1e-3, -0.5, 1.0),
    "gamma": (FAM_TWEEDIE, 2.0, 1e-3, 0.5, 0.5),
    "tweedie15": (FAM_TWEEDIE, 1.5, 1e-3, 0.5, 0.8),
    "binomial": (FAM_BINOMIAL, 0.0, 1e-3, -1.0, 1.0),
    "nb2": (FAM_NB2, 0.5, 1e-3, 0.0, 1.0),
}
# cond_2(A) of each case at the generating coefficients (oracle; see the module docstring)
COND_A = {"normal": 39.1, "ridge": 33.8, "poisson": 41.2, "gamma": 38.1,
          "tweedie15": 39.2, "binomial": 35.1, "nb2": 38.8}


def true_beta(m, L, b0):
    """Event 0 strong, event 1 a zero kernel, the rest moderate; intercept last."""
    t = np.arange(L)
    w = np.zeros((m, L))
    w[0] = 0.6 * np.exp(-t / 6.0)
    for a in range(2, m):
        w[a] = (0.1 + 0.05 * a) * np.cos(t / 4.0 + a) * np.exp(-t / 10.0)
    return np.r_[w.reshape(-1), b0]


@lru_cache(maxsize=None)
def gpu_design():
    rng = np.random.default_rng(2801)
    return lagged(rng, GPU_N, GPU_M, GPU_L)


@lru_cache(maxsize=None)
def gpu_case(name, resp=0):
    """(frame, y, group ids, generating beta) of a GPU case; ``resp`` picks another draw of y."""
    fam, power, alpha, b0, phi = GPU_FAMILIES[name]
    X, ids = gpu_design()
    beta = true_beta(GPU_M, GPU_L, b0)
    rng = np.random.default_rng([2802, sorted(GPU_FAMILIES).index(name), resp])
    y = draw(rng, fam, power, xt(X) @ beta, phi)
    return X, y, ids, beta


def lam_of(name, n):
    """The penalty in the engine's sum scaling: alpha for Ridge / OLS, alpha n for the GLMs."""
    fam, power, alpha, b0, phi = GPU_FAMILIES[name]
    return alpha if fam == FAM_SQUARED else alpha * n


@lru_cache(maxsize=None)
def small_case(fam, power, n=400, m=2, L=3, b0=-0.3, seed=7):
    """A small design (p = 6) for the oracle's own checks."""
    rng = np.random.default_rng([seed, fam])
    X, ids = lagged(rng, n, m, L, rate=0.2)
    beta = np.r_[rng.normal(0, 0.3, m * L), b0]
    y = draw(rng, fam, power, xt(X) @ beta, 0.6)
    return xt(X), y, ids, beta


# ------------------------------------------------------------------------------ kernel bounds
def inverse_bound(U, state):
    """(reference A^-1 in longdouble, entrywise error bound) of sglm_chol64_inverse on a factor
    with the factor's conventions.  With T = U_KK^-1: a computed triangular inverse satisfies
    |T^ - T| <= c u |T||U||T| (Higham, Accuracy and Stability, 14.1) and the product
    |fl(T^ T^T) - T^ T^T| <= gamma_P |T||T^T|, so
    |Ainv^ - T T^T| <= (2 P + 4) u (W + W^T + |T||T^T|), W = (|T||U||T|)|T^T|."""
    P = U.shape[0]
    K = np.flatnonzero(state == KEPT)
    Uk = ld(np.triu(U)[np.ix_(K, K)])
    T = ld_tri_inv(Uk)
    aT, aU = np.abs(T), np.abs(Uk)
    W = (aT @ aU @ aT) @ aT.T
    bound = (2 * P + 4) * U53 * (W + W.T + aT @ aT.T)
    return embed(T @ T.T, K, P), embed(bound, K, P).astype(np.float64)


def cov_block_bounds(Ainv, M, lam, phi, p, cov_type, cols, w):
    """(C_gg, entrywise bound E on its computed value, stat, bound on the computed stat) for the
    columns ``cols`` of sglm_cov_groups, in longdouble.  Every entry of C_gg is a sum of at most
    P^2 products accumulated in float64 FMA: |C^ - C| <= (2 P + 4) u S, S the same sum over
    magnitudes.  The Cholesky factor R^ of C^ is exact for C^ + dC, |dC| <= (k + 2) u |R^T||R|,
    and stat = w^T C^-1 w moves by x^T dC x to first order (x = C^-1 w); the bound carries a factor
    2 for the higher orders and (2 k + 4) u stat for the triangular solve and the final sum."""
    P = Ainv.shape[0]
    A_, aA = ld(Ainv), np.abs(ld(Ainv))
    c = np.asarray(cols)
    if cov_type == "robust":
        C = (A_[c] @ ld(M)) @ A_[:, c]
        S = (aA[c] @ np.abs(ld(M))) @ aA[:, c]
    elif cov_type == "bayes":
        C = phi * A_[np.ix_(c, c)]
        S = np.abs(C)
    else:
        D = np.r_[np.ones(p), np.zeros(P - p)]
        C = phi * (A_[np.ix_(c, c)] - lam * (A_[c] * D) @ A_[:, c])
        S = phi * (aA[np.ix_(c, c)] + lam * (aA[c] * D) @ aA[:, c])
    E = (2 * P + 4) * U53 * S
    k = len(c)
    T, R = ld_chol_inv(C)
    x = T @ (T.T @ ld(w))
    stat = x @ ld(w)
    aR = np.abs(R)
    dC = E + (k + 2) * U53 * (aR.T @ aR)
    sb = 2 * (np.abs(x) @ dC @ np.abs(x)) + (2 * k + 4) * U53 * stat
    return C, E.astype(np.float64), float(stat), float(sb)
