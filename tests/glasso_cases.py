"""Group-lasso cases and their float64 numpy oracle (no device, no engine code).

Objective (sklearn ElasticNet's scaling, one penalty term per column group):
  1/(2n)|y - Xw - b|^2 + alpha rho sum_g sqrt(k_g)|w_g|_2 + alpha (1 - rho)/2 |w|^2,
times n on centred data: 1/2 w'Qw - q'w + sum_g lam_g|w_g| + l2/2|w|^2 with
lam_g = alpha rho n sqrt(k_g), l2 = alpha (1 - rho) n.

The oracle is block-wise majorised descent (Yang & Zou's GMD) with the majoriser
gam_g = lambda_max(Q_gg) (numpy.linalg.eigvalsh) + l2, run to max|dw| <= 1e-13 max|w|, and a
KKT function that returns the worst relative violation over the groups.
"""
import functools

import numpy as np

ORACLE_TOL = 1e-13


def csr(groups):
    """(goff, gcols) of a group-id array: groups ordered by id, columns ascending."""
    ids = np.asarray(groups).reshape(-1)
    _, inv, counts = np.unique(ids, return_inverse=True, return_counts=True)
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
            np.argsort(inv, kind="stable").astype(np.int32))


def centred(X, y, fit_intercept=True):
    """Q = Xc'Xc, q = Xc'yc and the column / response means (zeros without an intercept)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if fit_intercept:
        xm, ym = X.mean(axis=0), float(y.mean())
    else:
        xm, ym = np.zeros(X.shape[1]), 0.0
    Xc, yc = X - xm, y - ym
    return Xc.T @ Xc, Xc.T @ yc, xm, ym


def gmd(Q, q, lam_scale, l2, goff, gcols, tol=ORACLE_TOL, max_sweeps=200000):
    """Block descent on 1/2 w'Qw - q'w + lam_scale sum_g sqrt(k_g)|w_g| + l2/2|w|^2 from w = 0;
    returns (w, sweeps)."""
    p = Q.shape[0]
    G = [gcols[goff[g]:goff[g + 1]] for g in range(len(goff) - 1)]
    gam = [float(np.linalg.eigvalsh(Q[np.ix_(c, c)])[-1]) + l2 for c in G]
    w = np.zeros(p)
    Qw = np.zeros(p)
    for sweep in range(1, max_sweeps + 1):
        dmax = 0.0
        for c, g in zip(G, gam):
            if g <= 0.0:
                continue
            lam = lam_scale * np.sqrt(len(c))
            z = w[c] + (q[c] - Qw[c] - l2 * w[c]) / g
            nz = float(np.sqrt(z @ z))
            new = z * (1.0 - (lam / g) / nz) if nz > lam / g else np.zeros(len(c))
            d = new - w[c]
            if np.any(d != 0.0):
                Qw += Q[:, c] @ d
                w[c] = new
                dmax = max(dmax, float(np.max(np.abs(d))))
        wmax = float(np.max(np.abs(w)))
        if wmax == 0.0 or dmax <= tol * wmax:
            return w, sweep
    return w, max_sweeps


def kkt(Q, q, lam_scale, l2, goff, gcols, w):
    """Worst relative KKT violation over the groups: a zero group violates by
    max(0, |grad_g| - lam_g) / lam_g, a non-zero one by |grad_g - lam_g w_g/|w_g|| / lam_g,
    grad = q - Qw - l2 w."""
    w = np.asarray(w, dtype=np.float64)
    grad = q - Q @ w - l2 * w
    worst = 0.0
    for g in range(len(goff) - 1):
        c = gcols[goff[g]:goff[g + 1]]
        lam = lam_scale * np.sqrt(len(c))
        nw = float(np.sqrt(w[c] @ w[c]))
        if nw == 0.0:
            v = max(0.0, float(np.sqrt(grad[c] @ grad[c])) - lam) / lam
        else:
            r = grad[c] - lam * w[c] / nw
            v = float(np.sqrt(r @ r)) / lam
        worst = max(worst, v)
    return worst


def margins(Q, q, lam_scale, l2, goff, gcols, w):
    """(largest |grad_g| / lam_g over the zero groups (0 if none), smallest |w_g| over the
    non-zero groups / largest |w_g| (1 if none)): how well the zero pattern is determined."""
    grad = q - Q @ w - l2 * w
    zero, norms = 0.0, []
    for g in range(len(goff) - 1):
        c = gcols[goff[g]:goff[g + 1]]
        nw = float(np.sqrt(w[c] @ w[c]))
        if nw == 0.0:
            zero = max(zero, float(np.sqrt(grad[c] @ grad[c])) / (lam_scale * np.sqrt(len(c))))
        else:
            norms.append(nw)
    return zero, (min(norms) / max(norms) if norms else 1.0)


def zero_groups(w, goff, gcols):
    """Boolean per group: all its coefficients are exactly 0.0."""
    return np.array([bool(np.all(w[gcols[goff[g]:goff[g + 1]]] == 0.0))
                     for g in range(len(goff) - 1)])


def fit(X, y, alpha, rho, groups, fit_intercept=True):
    """Oracle fit of the rows given: (w, b, sweeps)."""
    Q, q, xm, ym = centred(X, y, fit_intercept)
    n = X.shape[0]
    goff, gcols = csr(groups)
    w, sw = gmd(Q, q, alpha * rho * n, alpha * (1.0 - rho) * n, goff, gcols)
    return w, (float(ym - xm @ w) if fit_intercept else 0.0), sw


# ---------------------------------------------------------------------------------------------
# designs: 0/1 event designs (an event's kernel = its block of lag columns), events at rate
# 0.06, two strong events, one weak one, the rest null

def event_design(n, sizes, seed, rate=0.06, noise=1.0, interleave=None):
    """X (n x sum(sizes), 0/1 float64), y, groups (id per column).  ``interleave`` = (a, b):
    the columns of groups a and b alternate (non-contiguous groups)."""
    rng = np.random.default_rng(seed)
    L = max(sizes)
    cols, ids, beta = [], [], []
    for e, k in enumerate(sizes):
        ev = (rng.random(n + L) < rate).astype(np.float64)
        for lag in range(k):
            cols.append(ev[L - lag:L - lag + n])
        ids += [e] * k
        amp = (1.6, -1.2, 0.25)[e] if e < 3 else 0.0
        beta += list(amp * np.exp(-np.arange(k) / max(2.0, k / 4.0)))
    X = np.stack(cols, axis=1)
    beta = np.asarray(beta)
    ids = np.asarray(ids, dtype=np.int64)
    if interleave is not None:
        a, b = interleave
        ia, ib = np.flatnonzero(ids == a), np.flatnonzero(ids == b)
        slots = np.sort(np.concatenate([ia, ib]))
        m = min(ia.size, ib.size)
        mixed = np.empty(2 * m, dtype=np.int64)
        mixed[0::2], mixed[1::2] = ia[:m], ib[:m]
        src = np.concatenate([mixed, ia[m:], ib[m:]])
        perm = np.arange(ids.size)
        perm[slots] = src
        X, beta, ids = X[:, perm], beta[perm], ids[perm]
    y = X @ beta + 0.3 + noise * rng.standard_normal(n)
    return np.ascontiguousarray(X), y, ids


# name -> (n, group sizes, seed, interleave); alphas per case in ALPHAS
CASES = {
    "6x5": (600, [5] * 6, 9, None),
    "8x12": (3000, [12] * 8, 4, None),
    "p257": (2000, [1, 3, 40, 64, 70, 79], 7, (2, 3)),
    "p640": (3000, [300, 200, 100, 30, 10], 2, None),
}
ALPHAS = (0.002, 0.01, 0.03)
RHOS = (1.0, 0.5)
ALPHA_ALL_ZERO = 0.5          # with rho = 1 every group of every case is zero


@functools.lru_cache(maxsize=None)
def case(name):
    n, sizes, seed, inter = CASES[name]
    X, y, ids = event_design(n, sizes, seed, interleave=inter)
    X.setflags(write=False)
    y.setflags(write=False)
    ids.setflags(write=False)
    return X, y, ids


@functools.lru_cache(maxsize=None)
def gram(name, fit_intercept=True):
    """(Q, q, xm, ym, n, goff, gcols) of a case's full rows (read-only)."""
    X, y, ids = case(name)
    Q, q, xm, ym = centred(X, y, fit_intercept)
    goff, gcols = csr(ids)
    for a in (Q, q, xm):
        a.setflags(write=False)
    return Q, q, xm, ym, X.shape[0], goff, gcols


@functools.lru_cache(maxsize=None)
def many_fits():
    """(Qs [2][p][p], fits, goff, gcols) on the 6x5 design: 27 fits (Q index, q, lam_scale, l2)
    sorted by Q -- Q 0 centred, Q 1 not; three responses x four penalties each, then one fit
    with every group zero (indices 12 and 25), and a last fit on Q 1."""
    X, y, ids = case("6x5")
    n = X.shape[0]
    goff, gcols = csr(ids)
    rng = np.random.default_rng(0)
    ys = [y, np.roll(y, 7) + 0.5 * X[:, 3], y + rng.standard_normal(n)]
    Qs, fits = [], []
    for qi, fi in enumerate((True, False)):
        grams = [centred(X, yy, fi) for yy in ys]
        Qs.append(grams[0][0])
        for gr in grams:
            for a, rho in ((0.002, 1.0), (0.01, 1.0), (0.03, 0.5), (0.01, 0.5)):
                fits.append((qi, gr[1], a * rho * n, a * (1 - rho) * n))
        fits.append((qi, grams[0][1], ALPHA_ALL_ZERO * n, 0.0))
    fits.append((1, grams[1][1], 0.02 * n, 0.0))
    return np.stack(Qs), fits, goff, gcols


@functools.lru_cache(maxsize=None)
def path_oracle(name="6x5", K=3):
    """(Y [n][3], {(resp, alpha, rho, k): (w, b, test neg-mse, margins)}) of the multi-response
    path test: response 0 is the case's y, the split fits of responses 1 and 2 are solved
    here (k < K)."""
    X, y, ids = case(name)
    n = X.shape[0]
    goff, gcols = csr(ids)
    rng = np.random.default_rng(8)
    Y = np.stack([y, np.roll(y, 11) + 0.7 * X[:, 7], y + 0.5 * rng.standard_normal(n)], axis=1)
    out = {}
    for resp in (1, 2):
        for rho in RHOS:
            for alpha in ALPHAS:
                for k, (tr, te) in enumerate(folds(n, K)):
                    Q, q, xm, ym = centred(X[tr], Y[tr, resp])
                    ls, l2 = alpha * rho * len(tr), alpha * (1.0 - rho) * len(tr)
                    w, _ = gmd(Q, q, ls, l2, goff, gcols)
                    b = float(ym - xm @ w)
                    out[(resp, alpha, rho, k)] = (w, b, scores(X, Y[:, resp], w, b, te)[0],
                                                  margins(Q, q, ls, l2, goff, gcols, w))
    Y.setflags(write=False)
    return Y, out


def folds(n, K=3, seed=1):
    """K (train, test) index pairs: blocks of 20 rows dealt to the folds at random."""
    rng = np.random.default_rng(seed)
    owner = np.repeat(rng.integers(0, K, size=(n + 19) // 20), 20)[:n]
    return [(np.flatnonzero(owner != k), np.flatnonzero(owner == k)) for k in range(K)]


def scores(X, y, w, b, rows):
    """(neg mse, r2, residual sum of squares, sum of squares about the mean) on ``rows``."""
    r = y[rows] - X[rows] @ w - b
    ss = float(r @ r)
    sst = float(np.sum((y[rows] - y[rows].mean()) ** 2))
    return -ss / len(rows), 1.0 - ss / sst, ss, sst


@functools.lru_cache(maxsize=None)
def grid_oracle(name, fit_intercept=True, K=3):
    """Per (alpha, rho) of ALPHAS x RHOS the oracle's CV cell of a case: split fits on
    X[train], the refit on every row, host float64 scores.  Also ``margins`` / ``kkt`` per fit."""
    X, y, ids = case(name)
    n = X.shape[0]
    goff, gcols = csr(ids)
    cv = folds(n, K)
    out = {}
    for rho in RHOS:
        for alpha in ALPHAS:
            cell = {"coefs": [], "b": [], "tr": [], "te": [], "marg": [], "kkt": []}
            ss_res = ss_tot = n_te = 0.0
            for tr, te in cv + [(np.arange(n), None)]:
                Q, q, xm, ym = centred(X[tr], y[tr], fit_intercept)
                ls, l2 = alpha * rho * len(tr), alpha * (1.0 - rho) * len(tr)
                w, _ = gmd(Q, q, ls, l2, goff, gcols)
                b = float(ym - xm @ w) if fit_intercept else 0.0
                cell["marg"].append(margins(Q, q, ls, l2, goff, gcols, w))
                cell["kkt"].append(kkt(Q, q, ls, l2, goff, gcols, w))
                if te is None:
                    cell["refit"] = (w, b)
                    continue
                cell["coefs"].append(w)
                cell["b"].append(b)
                cell["tr"].append(scores(X, y, w, b, tr))
                s_te = scores(X, y, w, b, te)
                cell["te"].append(s_te)
                ss_res += s_te[2]
                ss_tot += s_te[3]
                n_te += len(te)
            cell["cv_R2_score"] = 1.0 - ss_res / ss_tot
            cell["cv_mse_score"] = ss_res / n_te
            out[(alpha, rho)] = cell
    return cv, out


@functools.lru_cache(maxsize=None)
def solution(name, alpha, rho, fit_intercept=True, singletons=False):
    """Oracle (w, sweeps) of a case's full rows at one (alpha, rho)."""
    Q, q, xm, ym, n, goff, gcols = gram(name, fit_intercept)
    if singletons:
        goff, gcols = csr(np.arange(Q.shape[0]))
    w, sw = gmd(Q, q, alpha * rho * n, alpha * (1.0 - rho) * n, goff, gcols)
    w.setflags(write=False)
    return w, sw
