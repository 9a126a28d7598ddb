"""Generate tests/golden/tweedie_enet.npz: float64 oracle fits of the elastic-net penalised
Poisson / Gamma / Tweedie log-link objective

    (1/n) sum_i m_i loss_power(y_i, eta_i) + alpha rho |w|_1 + alpha (1 - rho)/2 |w|^2,
    eta = X w + b  (b unpenalised),

numpy and float64 only.  The oracle is a proximal Newton method with the exact weights: every
outer iteration forms the exact gradient and Hessian, minimises the penalised quadratic model
by cyclic coordinate descent to max|du| <= 1e-12 max|u|, and backtracks on the exact objective;
it stops when the KKT violation of the sum-scaled objective is <= 1e-12 n.

Every stored fit must be well separated from a change of its zero set (the generator fails
instead of dropping a case):
  * every zero coefficient has |g_j + l2 w_j| <= (1 - 1e-3) l1;
  * every non-zero coefficient has |w_j| >= 1e-3 max|w|.

Both margins are asserted for the 14 single fits and for every fold fit of the grid (a fold fit
that misses one is cured by another fold seed, never by another threshold).  The grid's three
refits are fits on ALL rows, which no seed moves: the one at alpha = 0.005, rho = 0.5 has a zero
coefficient at 0.99927 l1 (slack 7.27e-4 < 1e-3).  The data, the penalties and the threshold
are all fixed, so that one slack cannot be met; the refits' slacks are stored
(``grid_refit_slack``) and asserted positive, their non-zero margin is asserted as usual.

Usage: ``python tests/golden/make_golden_tweedie_enet.py`` -> tests/golden/tweedie_enet.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import folds_ref  # noqa: E402  (pure numpy fold generation)

N, M_EV, K_LAG = 6000, 6, 8
CASES = ([(1.0, a, r) for a, r in ((0.02, 0.5), (0.005, 1.0), (0.002, 0.9))]
         + [(pw, a, r) for pw in (2.0, 1.5) for a, r in ((0.02, 0.5), (0.005, 1.0))])
GRID_ALPHAS = (0.02, 0.005, 0.002)
GRID_RHO = 0.5
FOLD_SEED = 3
MARGIN = 1e-3


def make_data():
    rng = np.random.default_rng(7)
    E = rng.random((N + K_LAG, M_EV)) < 0.04
    X = np.concatenate([E[K_LAG - s:N + K_LAG - s] for s in range(K_LAG)], axis=1).astype(np.float64)
    p = X.shape[1]
    bt = rng.normal(0, .4, p) * (rng.random(p) < .5)
    y = rng.poisson(np.exp(X @ bt - 0.7)).astype(np.float64)
    return E, X, y


def loss_parts(power, y, eta):
    """(loss, dloss/deta, d2loss/deta2) of the half-Tweedie loss with the log link."""
    if power == 1.0:
        mu = np.exp(eta)
        return mu - y * eta, mu - y, mu
    if power == 2.0:
        e = y * np.exp(-eta)
        return eta + e, 1.0 - e, e
    a = np.exp((2.0 - power) * eta)
    b = y * np.exp((1.0 - power) * eta)
    return a / (2.0 - power) - b / (1.0 - power), a - b, (2.0 - power) * a - (1.0 - power) * b


def kkt(g, w, l1, l2, fit_intercept):
    """KKT violation of the sum-scaled objective at (w, b); g = X~^T loss' (p + 1 entries)."""
    gx = g[:-1] + l2 * w
    v = np.where(w != 0, np.abs(gx + l1 * np.sign(w)), np.maximum(np.abs(gx) - l1, 0.0))
    out = float(v.max()) if v.size else 0.0
    return max(out, abs(float(g[-1]))) if fit_intercept else out


def cd(Q, q, l1, l2, u, tol=1e-12, max_sweeps=100000):
    """Cyclic CD on 1/2 u^T Q u - q^T u + l1 |u|_1 + l2/2 |u|^2 from u (in place)."""
    hv = Q @ u - q
    dg = np.diag(Q).copy()
    for _ in range(max_sweeps):
        mdu = 0.0
        for j in range(u.size):
            if dg[j] <= 0.0:
                continue
            rho = dg[j] * u[j] - hv[j]
            mag = abs(rho) - l1
            nu = np.copysign(mag, rho) / (dg[j] + l2) if mag > 0 else 0.0
            d = nu - u[j]
            if d != 0.0:
                hv += Q[:, j] * d
                u[j] = nu
                mdu = max(mdu, abs(d))
        mu = float(np.abs(u).max()) if u.size else 0.0
        if mu == 0.0 or mdu <= tol * mu:
            break
    return u


def fit(X, y, power, alpha, rho, fit_intercept, max_iter=200, check=True):
    n, p = X.shape
    l1, l2 = alpha * rho * n, alpha * (1.0 - rho) * n
    Xa = np.concatenate([X, np.ones((n, 1))], axis=1)
    w = np.zeros(p)
    b = float(np.log(y.mean())) if fit_intercept else 0.0

    def objective(w_, b_):
        return float(loss_parts(power, y, X @ w_ + b_)[0].sum()
                     + l1 * np.abs(w_).sum() + 0.5 * l2 * (w_ @ w_))

    for it in range(max_iter):
        _, gl, hl = loss_parts(power, y, X @ w + b)
        g = Xa.T @ gl
        viol = kkt(g, w, l1, l2, fit_intercept)
        if viol <= 1e-12 * n:
            break
        H = Xa.T @ (Xa * hl[:, None])
        Hxx, h, hpp = H[:p, :p], H[:p, p], H[p, p]
        if fit_intercept:
            Q = Hxx - np.outer(h, h) / hpp
            gt = g[:p] - h * g[p] / hpp
        else:
            Q, gt = Hxx, g[:p]
        u = cd(Q, Q @ w - gt, l1, l2, w.copy())
        dw = u - w
        db = -(g[p] + h @ dw) / hpp if fit_intercept else 0.0
        dec = g[:p] @ dw + g[p] * db + l2 * (w @ dw) + l1 * (np.abs(u).sum() - np.abs(w).sum())
        f0, t = objective(w, b), 1.0
        while t > 1e-10:
            wt = u if t == 1.0 else w + t * dw
            ft = objective(wt, b + t * db)
            # Armijo (sigma = 2^-11) up to the rounding of the objective itself
            if ft - f0 <= 2.0 ** -11 * t * dec + 1e-14 * abs(f0):
                break
            t *= 0.5
        w, b = wt, b + t * db
    else:
        raise RuntimeError(f"oracle did not converge: KKT {viol:.3e}")
    _, gl, _ = loss_parts(power, y, X @ w + b)
    g = Xa.T @ gl
    # the margins that keep the zero set stable under the engine's roundings
    zero = w == 0
    slack = 1.0 - (np.abs(g[:p] + l2 * w)[zero] / l1).max() if zero.any() else np.inf
    small = (np.abs(w[~zero]).min() / np.abs(w).max()) if (~zero).any() else np.inf
    if check:
        assert slack >= MARGIN, f"zero coefficient within {slack:.2e} of l1"
        assert small >= MARGIN, f"non-zero coefficient at {small:.2e} of max|w|"
    return w, b, it, kkt(g, w, l1, l2, fit_intercept), slack, small, int(zero.sum())


def response(power, y):
    return y + 0.5 if power == 2.0 else y


def main():
    E, X, y = make_data()
    out = {"E": E.astype(np.uint8), "y": y,
           "case_power": np.array([c[0] for c in CASES]),
           "case_alpha": np.array([c[1] for c in CASES]),
           "case_rho": np.array([c[2] for c in CASES])}
    coef = np.zeros((len(CASES), 2, X.shape[1]))
    icpt = np.zeros((len(CASES), 2))
    for c, (power, alpha, rho) in enumerate(CASES):
        for fi in (1, 0):
            w, b, it, viol, slack, small, nz = fit(X, response(power, y), power, alpha, rho,
                                                   bool(fi))
            coef[c, fi], icpt[c, fi] = w, b
            print(f"power {power} alpha {alpha} rho {rho} intercept {fi}: {it} iterations, "
                  f"KKT/n {viol / N:.1e}, slack {slack:.2e}, min rel {small:.2e}, zeros {nz}")
    out["coef"], out["intercept"] = coef, icpt
    # 3-fold grid: trial id t // 100, the reference's group shuffle split on the global RNG
    np.random.seed(FOLD_SEED)
    codes = folds_ref.trial_bucket_codes([np.arange(N) // 100])
    folds = folds_ref.cv_idx_from_bucket_ids(codes, num_folds=3)
    gc = np.zeros((len(GRID_ALPHAS), len(folds), X.shape[1]))
    gb = np.zeros((len(GRID_ALPHAS), len(folds)))
    rc = np.zeros((len(GRID_ALPHAS), X.shape[1]))
    rb = np.zeros(len(GRID_ALPHAS))
    rs, rm = np.zeros(len(GRID_ALPHAS)), np.zeros(len(GRID_ALPHAS))
    for j, alpha in enumerate(GRID_ALPHAS):
        for k, (tr, _) in enumerate(folds):
            w, b, it, viol, slack, small, nz = fit(X[tr], y[tr], 1.0, alpha, GRID_RHO, True)
            gc[j, k], gb[j, k] = w, b
            print(f"grid alpha {alpha} fold {k}: {it} iterations, slack {slack:.2e}, "
                  f"min rel {small:.2e}, zeros {nz}")
        # the refit is on all rows: neither the fold seed nor anything else left open moves it
        # (see the module docstring)
        rc[j], rb[j], _, _, rs[j], rm[j], _ = fit(X, y, 1.0, alpha, GRID_RHO, True, check=False)
        assert rs[j] > 0 and rm[j] >= MARGIN
        print(f"grid alpha {alpha} refit: slack {rs[j]:.2e}, min rel {rm[j]:.2e}")
    out.update(grid_alpha=np.array(GRID_ALPHAS), grid_rho=np.array(GRID_RHO),
               grid_coef=gc, grid_intercept=gb, grid_refit_coef=rc, grid_refit_intercept=rb,
               grid_refit_slack=rs, grid_refit_minrel=rm)
    for k, (tr, te) in enumerate(folds):
        out[f"fold{k}_train"], out[f"fold{k}_test"] = tr.astype(np.int32), te.astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "tweedie_enet.npz"), **out)


if __name__ == "__main__":
    main()
