"""Cases and the numpy oracle of the fitted-trace band tests (sglm_hip.inference.predict_bands,
csrc/predict.hip).  No engine code.  On the dense X~ (ones column last) and a
covariance C, in np.longdouble:

    eta = X~ beta,   v = einsum('ij,jk,ik->i', X~, C, X~),   and the same on a column group.

The kernels add the m (m + 1) / 2 terms of a row's quadratic form (m set bits: diagonal + 2
upper) in float64; the products are by 0 / 1, so only the sums round.  Whatever the order, the
computed value lies within

    (m (m + 1) / 2 + 2) 2^-53 sum_{j,k in S} |C_jk|       of v,
    (m + 2) 2^-53 sum_{j in S} |beta_j|                   of eta

(recursive summation of t terms: (t - 1) u sum |terms| to first order, and u (t + 2) / (1 - t u)
covers the higher orders for t < 2^40; the diagonal + 2 upper form has fewer terms than t).  The
link-scale intervals go through inverse links written here in plain numpy.
"""
import numpy as np

import infer_cases as C

LD = C.LD
U53 = C.U53


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------ the oracle
def traces(Xt, beta, cov, cols=None):
    """(eta, v) in longdouble on the columns ``cols`` of X~ (all when None), dense."""
    cols = np.arange(Xt.shape[1]) if cols is None else np.asarray(cols)
    Xs = ld(Xt[:, cols])
    eta = Xs @ ld(np.asarray(beta)[cols])
    v = np.einsum("ij,jk,ik->i", Xs, ld(np.asarray(cov)[np.ix_(cols, cols)]), Xs)
    return eta, v


def bounds(Xt, beta, cov, cols=None):
    """(eta bound, v bound) per row: the rounding bounds of the module docstring."""
    cols = np.arange(Xt.shape[1]) if cols is None else np.asarray(cols)
    Xs = np.asarray(Xt[:, cols], dtype=np.float64)
    m = Xs.sum(axis=1)
    sb = Xs @ np.abs(np.asarray(beta, dtype=np.float64)[cols])
    sc = np.einsum("ij,jk,ik->i", Xs, np.abs(np.asarray(cov, dtype=np.float64)[np.ix_(cols, cols)]),
                   Xs)
    return (m + 2) * U53 * sb, (m * (m + 1) / 2 + 2) * U53 * sc


def traces_rows(Xt, beta, cov, cols=None):
    """(eta, v, eta bound, v bound) by the set bits of each row: the same numbers as ``traces``
    and ``bounds`` at O(m^2) per row (the kernel tests' larger shapes)."""
    cols = np.arange(Xt.shape[1]) if cols is None else np.asarray(cols)
    Xs = np.asarray(Xt[:, cols]) != 0
    b = np.asarray(beta, dtype=np.float64)[cols]
    Cs = np.asarray(cov, dtype=np.float64)[np.ix_(cols, cols)]
    n = Xs.shape[0]
    eta, v = np.zeros(n, LD), np.zeros(n, LD)
    eb, vb = np.zeros(n), np.zeros(n)
    for i in range(n):
        S = np.flatnonzero(Xs[i])
        m = S.size
        if not m:
            continue
        blk = Cs[np.ix_(S, S)]
        eta[i] = ld(b[S]).sum()
        v[i] = ld(blk).sum()
        eb[i] = (m + 2) * U53 * np.abs(b[S]).sum()
        vb[i] = (m * (m + 1) / 2 + 2) * U53 * np.abs(blk).sum()
    return eta, v, eb, vb


def brute(Xt, beta, cov):
    """(eta, v) by the plain triple loop, longdouble."""
    n, P = Xt.shape
    eta, v = np.zeros(n, LD), np.zeros(n, LD)
    for i in range(n):
        for j in range(P):
            eta[i] += LD(Xt[i, j]) * LD(beta[j])
            for k in range(P):
                v[i] += LD(Xt[i, j]) * LD(cov[j, k]) * LD(Xt[i, k])
    return eta, v


def ratio(err, bound):
    """max |err| / bound, an error at a zero bound counting as inf (0 / 0 = 0)."""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------ links
def inv_link(fam, eta):
    """The mean at eta in float64: identity, exp, or the logistic function from exp(-|eta|)."""
    eta = np.asarray(eta, dtype=np.float64)
    if fam == C.FAM_SQUARED:
        return eta.copy()
    if fam == C.FAM_BINOMIAL:
        e = np.exp(-np.abs(eta))
        return np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
    return np.exp(eta)


def dmu_deta(fam, eta):
    eta = np.asarray(eta, dtype=np.float64)
    if fam == C.FAM_SQUARED:
        return np.ones_like(eta)
    if fam == C.FAM_BINOMIAL:
        e = np.exp(-np.abs(eta))
        return e / (1 + e) ** 2
    return np.exp(eta)


def zq(level):
    """The two-sided normal quantile by bisection on erfc (no scipy)."""
    import math
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > 1.0 - level:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def bands(fam, eta, se, level):
    """(mean, mean_se, lo, hi): the interval on the link scale through the inverse link."""
    z = zq(level)
    eta, se = np.asarray(eta, dtype=np.float64), np.asarray(se, dtype=np.float64)
    return (inv_link(fam, eta), dmu_deta(fam, eta) * se, inv_link(fam, eta - z * se),
            inv_link(fam, eta + z * se))


# ------------------------------------------------------------------------------ kernel cases
def pack_rbits(X01, ldim, P):
    """The row-major planes [P/64][ld] x 2 uint32 of a 0/1 matrix (n x <= P columns), in the
    fragment order of the header: column 64 t + al of row i at bit rho / 2 + 16 (rho % 2),
    rho = al % 32, of word al / 32 of entry [t][i]."""
    n, pc = X01.shape
    out = np.zeros((P // 64, ldim, 2), dtype=np.uint32)
    for c in range(pc):
        t, al = c >> 6, c & 63
        rho = al & 31
        pos = (rho >> 1) + 16 * (rho & 1)
        out[t, :n, al >> 5] |= (X01[:, c] != 0).astype(np.uint32) << np.uint32(pos)
    return out


def spd(rng, P, scale=1.0):
    """A random symmetric positive definite float64 matrix, bitwise symmetric."""
    G = rng.normal(0, 1, (P, 2 * P))
    A = scale * (G @ G.T / (2 * P) + 0.1 * np.eye(P))
    return (A + A.T) / 2


def kernel_design(rng, n, p, density):
    """n x p 0/1 rows at ``density`` with the edge rows: 0 all zeros, 1 all ones, 2 and 3 only
    the last real column, 4 only the first."""
    X = (rng.random((n, p)) < density).astype(np.float64)
    X[0] = 0
    X[1] = 1
    X[2:5] = 0
    X[2, p - 1] = X[3, p - 1] = 1
    X[4, 0] = 1
    return X
