"""Elastic-net penalised Poisson / Gamma / Tweedie (log link) fits on the MI355X: the proximal
Newton solve (sglm_hip/pn.py, csrc/pn.hip) against the float64 oracle fixture
tests/golden/tweedie_enet.npz (make_golden_tweedie_enet.py), its closed-form edge, the paths that
must not change, warm starts, the CV grid, the three kernels against numpy float64, and the
cases that are refused.

The single-fit test prints each fit's float64 KKT violation / (alpha rho n), a diagnostic with no
threshold: worst 3.9e-6 over the 28 fits (worst coefficient error 3.2e-7 max|w|), DESIGN.md §21."""
import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

K_LAG = 8


def _design(Ev):
    N = Ev.shape[0] - K_LAG
    return np.concatenate([Ev[K_LAG - s:N + K_LAG - s] for s in range(K_LAG)],
                          axis=1).astype(np.float64)


@pytest.fixture(scope="module")
def fx(golden, engine):
    G = golden("tweedie_enet.npz")
    Ev = G["E"].astype(bool)
    X = np.ascontiguousarray(_design(Ev))
    from sglm_hip.lagframe import LagFrame
    df = pd.DataFrame(Ev.astype(np.float64), columns=[f"e{a}" for a in range(Ev.shape[1])])
    lf = LagFrame.from_shifts(df, [], list(range(K_LAG)))[K_LAG:]
    assert lf.shape == X.shape and lf.design().lag is not None
    return {"G": G, "X": X, "y": G["y"], "lf": lf}


def _grad(power, X, y, w, b):
    eta = X @ w + b
    if power == 1.0:
        r = np.exp(eta) - y
    elif power == 2.0:
        r = 1.0 - y * np.exp(-eta)
    else:
        r = np.exp((2.0 - power) * eta) - y * np.exp((1.0 - power) * eta)
    return np.concatenate([X.T @ r, [r.sum()]])


def _kkt(power, X, y, w, b, alpha, rho, fi):
    n, p = X.shape
    l1, l2 = alpha * rho * n, alpha * (1 - rho) * n
    g = _grad(power, X, y, w, b)
    gs = g[:p] + l2 * w
    v = np.where(w != 0, np.abs(gs + l1 * np.sign(w)), np.maximum(np.abs(gs) - l1, 0.0)).max()
    return max(v, abs(g[p])) if fi else v


def _hold(coef, icpt, w0, b0, what):
    """The project's Poisson tolerance (README): 1e-4 max|w| on coefficients and intercept;
    the zero set identical, zeros exactly 0.0."""
    bound = 1e-4 * np.abs(w0).max()
    err = max(np.abs(coef - w0).max(), abs(icpt - b0))
    assert err <= bound, f"{what}: error {err:.3e} > {bound:.3e}"
    assert np.array_equal(coef == 0.0, w0 == 0.0), f"{what}: zero set differs"


@pytest.mark.parametrize("fi", [1, 0])
@pytest.mark.parametrize("case", range(7))
def test_single_fits_match_the_oracle(fx, engine, monkeypatch, case, fi):
    from sglm_hip.estimators import TweedieRegressor
    G, X = fx["G"], fx["X"]
    power, alpha, rho = (float(G[k][case]) for k in ("case_power", "case_alpha", "case_rho"))
    y = fx["y"] + 0.5 if power == 2.0 else fx["y"]
    w0, b0 = G["coef"][case, fi], float(G["intercept"][case, fi])
    # the lag design takes its Hessians from the event-structured Gram whatever its cost model
    # says at this size
    ran = []
    lagw = engine._lag_gram_w
    monkeypatch.setattr(engine, "_lagw_pays", lambda *a: True)
    monkeypatch.setattr(engine, "_lag_gram_w", lambda *a, **k: ran.append(1) or lagw(*a, **k))
    # the estimator keeps no convergence flag: read it off the solver's result
    from sglm_hip import pn
    outs, solve = [], pn.prox_newton
    monkeypatch.setattr(pn, "prox_newton", lambda *a, **k: outs.append(solve(*a, **k)) or outs[-1])
    for name, Xd in (("dense", X), ("lag", fx["lf"])):
        ran.clear()
        m = TweedieRegressor(power=power, alpha=alpha, l1_ratio=rho, fit_intercept=bool(fi))
        m.fit(Xd, y)
        what = f"power {power} alpha {alpha} rho {rho} intercept {fi} {name}"
        _hold(m.coef_, m.intercept_, w0, b0, what)
        assert outs[-1][0][0].converged, what
        assert m.n_iter_ >= 1
        assert (name == "lag") == bool(ran), f"{what}: structured Gram calls {len(ran)}"
        viol = _kkt(power, X, y, m.coef_, m.intercept_, alpha, rho, fi)
        print(f"{what}: {m.n_iter_} iterations, KKT / (alpha rho n) = "
              f"{viol / (alpha * rho * X.shape[0]):.3e}, "
              f"err / max|w| = {np.abs(m.coef_ - w0).max() / np.abs(w0).max():.3e}")


def test_closed_form_edge_all_zero(fx):
    from sglm_hip.estimators import PoissonRegressor
    X, y = fx["X"], fx["y"]
    n, rho = X.shape[0], 0.5
    alpha = 1.01 * np.abs(X.T @ (y - y.mean())).max() / (n * rho)
    m = PoissonRegressor(alpha=alpha, l1_ratio=rho).fit(X, y)
    assert np.array_equal(m.coef_, np.zeros(X.shape[1]))
    assert abs(m.intercept_ - np.log(y.mean())) <= 1e-12
    assert m.n_iter_ == 1


def test_no_op_paths_are_bitwise(fx):
    from sglm_hip.estimators import ElasticNet, TweedieRegressor
    X, y = fx["X"], fx["y"]
    for power in (1.0, 2.0):
        yy = y + 0.5 if power == 2.0 else y
        a = TweedieRegressor(power=power, alpha=0.01).fit(X, yy)
        b = TweedieRegressor(power=power, alpha=0.01, l1_ratio=0).fit(X, yy)
        assert np.array_equal(a.coef_, b.coef_) and a.intercept_ == b.intercept_
        assert a.n_iter_ == b.n_iter_
    a = ElasticNet(alpha=0.01, l1_ratio=0.5).fit(X, y)
    b = TweedieRegressor(power=0, alpha=0.01, l1_ratio=0.5).fit(X, y)
    assert np.array_equal(a.coef_, b.coef_) and a.intercept_ == b.intercept_
    assert (a.coef_ != 0).any()


def test_warm_start_from_the_solution_takes_one_iteration(fx, engine):
    from sglm_hip.estimators import PoissonRegressor
    X, y = fx["X"], fx["y"]
    m = PoissonRegressor(alpha=0.005, l1_ratio=0.5, warm_start=True).fit(X, y)
    w, b = m.coef_.copy(), m.intercept_
    assert m.n_iter_ > 1
    m.fit(X, y)
    assert m.n_iter_ == 1
    scale = max(np.abs(w).max(), engine.STOP_SCALE_FLOOR)
    assert np.abs(m.coef_ - w).max() <= engine.STOP_TOL * scale
    assert abs(m.intercept_ - b) <= engine.STOP_TOL
    assert np.array_equal(m.coef_ == 0, w == 0)


def test_cv_grid_matches_the_oracle(fx):
    import sglm_cv
    G, X, y = fx["G"], fx["X"], fx["y"]
    cv_idx = [(G[f"fold{k}_train"].astype(np.int64), G[f"fold{k}_test"].astype(np.int64))
              for k in range(3)]
    alphas = [float(a) for a in G["grid_alpha"]]
    kw = [{"model_name": "Poisson", "alpha": a, "l1_ratio": .5} for a in alphas]
    out = sglm_cv.cv_glm_mult_params(X, y, cv_idx, "Poisson", kw)
    want_mean = []
    for j, r in enumerate(out["full_cv_results"]):
        assert r["glm_kwargs"]["alpha"] == alphas[j]
        tr_s, te_s = np.zeros(3), np.zeros(3)
        for k, (tr, te) in enumerate(cv_idx):
            w0, b0 = G["grid_coef"][j, k], float(G["grid_intercept"][j, k])
            _hold(r["cv_coefs"][:, k], r["cv_intercepts"][k], w0, b0, f"alpha {alphas[j]} fold {k}")
            tr_s[k] = -np.mean((y[tr] - np.exp(X[tr] @ w0 + b0)) ** 2)
            te_s[k] = -np.mean((y[te] - np.exp(X[te] @ w0 + b0)) ** 2)
        _hold(r["model"].coef_, r["model"].intercept_, G["grid_refit_coef"][j],
              float(G["grid_refit_intercept"][j]), f"alpha {alphas[j]} refit")
        for got, want in ((r["cv_scores_train"], tr_s), (r["cv_scores_test"], te_s),
                          (r["cv_mean_score"], te_s.mean())):
            rel = np.abs(np.asarray(got) - want).max() / np.abs(want).max()
            print(f"alpha {alphas[j]}: score rel err {rel:.3e}")
            assert rel <= 1e-6
        want_mean.append(te_s.mean())
    best = int(np.argmax(want_mean))
    assert out["best_params"]["alpha"] == alphas[best]
    assert abs(out["best_score"] - want_mean[best]) <= 1e-6 * abs(want_mean[best])


# ---- the kernels against numpy float64 ------------------------------------------------------

def _np_cd(Q, q, l1, l2, u, tol=1e-12):
    u = u.copy()
    hv = Q @ u - q
    dg = np.diag(Q)
    for _ in range(100000):
        mdu = 0.0
        for j in range(u.size):
            if dg[j] <= 0.0:
                nu = 0.0
            else:
                rho = dg[j] * u[j] - hv[j]
                mag = abs(rho) - l1
                nu = np.copysign(mag, rho) / (dg[j] + l2) if mag > 0 else 0.0
            d = nu - u[j]
            if d != 0.0:
                hv += Q[:, j] * d
                u[j] = nu
                mdu = max(mdu, abs(d))
        mu = np.abs(u).max()
        if mu == 0.0 or mdu <= tol * mu:
            return u
    raise AssertionError("numpy CD did not converge")


@pytest.mark.parametrize("fi", [1, 0])
@pytest.mark.parametrize("p", [1, 48, 70, 300])
def test_kernels_against_numpy(engine, p, fi):
    import torch
    from sglm_hip import _lib
    E = engine
    rng = np.random.default_rng(100 + p)
    n, P = 500, E.pad_to(p + 1, E.COL_PAD)
    # zero-mean entries: Q has no dominant direction with or without the intercept, so cyclic
    # descent reaches 1e-12 in tens of sweeps
    Xa = np.concatenate([(rng.random((n, p)) < 0.3) * rng.normal(0.0, 1.0, (n, p)),
                         np.ones((n, 1))], axis=1)
    zc = 3 if p > 1 else None
    if zc is not None:
        Xa[:, zc] = 0.0                                       # an all-zero column
    Wt = rng.random(n) + 0.5
    H32 = (Xa.T @ (Xa * Wt[:, None])).astype(np.float32)
    # two slots; only slot 1 is listed.  Below the diagonal the engine's Grams hold nothing the
    # kernels may read: NaN there
    Hd = np.full((2, P, P), np.nan, dtype=np.float32)
    Hd[1][np.triu_indices(P)] = 0.0
    Hd[1, :p + 1, :p + 1][np.triu_indices(p + 1)] = H32[np.triu_indices(p + 1)]
    H = H32.astype(np.float64)
    H = np.triu(H) + np.triu(H, 1).T
    g = np.zeros((2, P))
    g[1, :p + 1] = rng.normal(0, 5.0, p + 1)
    beta = np.zeros((2, P))
    beta[1, :p] = rng.normal(0, 0.3, p) * (rng.random(p) < 0.6)
    beta[1, p] = -0.4 if fi else 0.0
    w = beta[1, :p].copy()
    Hxx, h, hpp = H[:p, :p], H[:p, p], H[p, p]
    if fi:
        Q0 = Hxx - np.outer(h, h) / hpp
        gt = g[1, :p] - h * g[1, p] / hpp
    else:
        Q0, gt = Hxx.copy(), g[1, :p].copy()
    q0 = Q0 @ w - gt
    dev = "cuda"
    st = E._stream()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    H_d, g_d, beta_d = t(Hd), t(g), t(beta)
    slots, icpt = t(np.array([1], np.int32)), t(np.array([fi], np.uint8))
    Q_d = torch.full((1, p, p), np.nan, dtype=torch.float64, device=dev)
    q_d = torch.full((1, p), np.nan, dtype=torch.float64, device=dev)
    _lib.call("sglm_pn_model", E._p(H_d), P, p, E._p(slots), E._p(icpt), 1, E._p(g_d),
              E._p(beta_d), E._p(Q_d), E._p(q_d), st)
    Q, q = Q_d.cpu().numpy()[0], q_d.cpu().numpy()[0]
    assert np.abs(Q - Q0).max() <= 1e-12 * np.abs(Q0).max()
    assert np.array_equal(Q, Q.T)
    assert np.abs(q - q0).max() <= 1e-12 * max(np.abs(q0).max(), np.abs(Q0).max())

    # ---- the warm coordinate descent on the kernel's own model
    l1 = 0.35 * np.abs(gt).max()
    l2 = 0.05 * np.abs(np.diag(Q)).max()
    tol = 1e-12
    l1_d, l2_d = t(np.array([l1])), t(np.array([l2]))

    def warm(start):
        w_d = t(start[None, :].copy())
        sw = torch.full((2,), -1, dtype=torch.int32, device=dev)
        nz = torch.full((1,), -1, dtype=torch.int32, device=dev)
        _lib.call("sglm_enet_cd_warm", E._p(Q_d), p, 1, E._p(q_d), E._p(l1_d), E._p(l2_d), 10000,
                  tol, E._p(w_d), E._p(sw), E._p(nz), st)
        return w_d.cpu().numpy()[0], sw.cpu().numpy(), int(nz.cpu().numpy()[0])

    u0 = _np_cd(Q, q, l1, l2, w)
    scale = max(np.abs(u0).max(), 1e-300)
    start = w.copy()
    if zc is not None:
        start[zc] = 0.7                   # a warm value on the dead column must be cleared
    u, sw, nz = warm(start)
    assert np.abs(u - u0).max() <= 1e-9 * scale
    assert np.array_equal(u == 0.0, u0 == 0.0) and nz == int((u0 != 0).sum())
    if zc is not None:
        assert u[zc] == 0.0
    assert sw[0] >= 1 and sw[0] + sw[1] < 10000
    if p >= 48:
        assert (u0 == 0).any() and (u0 != 0).any() and sw[1] >= 1
    # from the solution: one full sweep, bitwise unchanged
    u2, sw2, nz2 = warm(u)
    assert np.array_equal(u2, u) and tuple(sw2) == (1, 0) and nz2 == nz
    # from a cold start: the answer of the shared-Gram kernel
    uc, _, _ = warm(np.zeros(p))
    ws = torch.zeros((1, p), dtype=torch.float64, device=dev)
    sws = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.call("sglm_enet_cd_shared", E._p(Q_d), p, E._p(t(np.array([0], np.int32))), 1,
              E._p(q_d), E._p(l1_d), E._p(l2_d), 10000, tol, E._p(ws), E._p(sws), st)
    assert np.abs(uc - ws.cpu().numpy()[0]).max() <= 1e-9 * scale

    # ---- direction, decrease, penalties, KKT
    ts = np.array([0.0, 1.0, 0.5, 0.25, 0.125, 0.0625, 2.0 ** -10])
    T = ts.size
    u_d = t(u[None, :])
    delta = torch.full((2, P), 7.0, dtype=torch.float32, device=dev)
    rec = torch.zeros((1, 4 + 2 * T), dtype=torch.float64, device=dev)
    _lib.call("sglm_pn_step", E._p(H_d), P, p, E._p(slots), E._p(icpt), 1, E._p(g_d),
              E._p(beta_d), E._p(u_d), E._p(l1_d), E._p(l2_d), E._p(t(ts)), T, E._p(delta),
              E._p(rec), st)
    r, dl = rec.cpu().numpy()[0], delta.cpu().numpy()
    dw = u - w
    db = -(g[1, p] + h @ dw) / hpp if fi else 0.0
    dec = g[1, :p] @ dw + (g[1, p] * db if fi else 0.0) + l2 * (w @ dw) \
        + l1 * (np.abs(u).sum() - np.abs(w).sum())
    gs = g[1, :p] + l2 * w
    viol = np.where(w != 0, np.abs(gs + l1 * np.sign(w)), np.maximum(np.abs(gs) - l1, 0.0)).max()
    if fi:
        viol = max(viol, abs(g[1, p]))
    trial = [u if tt == 1.0 else w + tt * dw for tt in ts]
    want = np.concatenate([[db, dec, viol, np.abs(dw).max()],
                           [l1 * np.abs(x).sum() + 0.5 * l2 * (x @ x) for x in trial],
                           [np.abs(x).max() for x in trial]])
    # sums of signed terms: relative to the size of their terms
    size = np.abs(want).copy()
    size[0] = max(size[0], (abs(g[1, p]) + np.abs(h * dw).sum()) / hpp) if fi else 1.0
    size[1] = (np.abs(g[1, :p] * dw).sum() + abs(g[1, p] * db) + l2 * np.abs(w * dw).sum()
               + l1 * (np.abs(u).sum() + np.abs(w).sum()))
    assert np.all(np.abs(r - want) <= 1e-12 * np.maximum(size, 1e-300)), (r, want)
    assert np.array_equal(dl[0], np.full(P, 7.0, np.float32))           # unlisted slot untouched
    assert np.array_equal(dl[1, :p], dw.astype(np.float32))
    assert dl[1, p] == np.float32(r[0]) and not dl[1, p + 1:].any()

    # ---- the step taken
    for tt in (1.0, 0.25, 0.0):
        b_d = t(beta)
        _lib.call("sglm_pn_update", P, p, E._p(slots), 1, E._p(t(np.array([tt]))), E._p(u_d),
                  E._p(rec), 4 + 2 * T, E._p(b_d), st)
        got = b_d.cpu().numpy()
        assert np.array_equal(got[0], beta[0])
        assert np.array_equal(got[1, :p], u if tt == 1.0 else w + tt * dw)
        assert got[1, p] == beta[1, p] + tt * r[0]


def test_unsupported_cases_raise(fx):
    import sglm
    from sglm_hip import grid
    from sglm_hip.comm import SimComm
    from sglm_hip.estimators import NotYetImplementedError, PoissonRegressor
    X, y = fx["X"], fx["y"]
    cv = [(np.arange(4000), np.arange(4000, 6000))]
    groups = [{"cv_idx": cv, "objectives": [PoissonRegressor(alpha=.01, l1_ratio=.5).objective()],
               "rolls": [0]}]
    with pytest.raises(NotYetImplementedError, match="log-link"):
        grid.run_multi(X, y, groups, drop_sets=[[], [1]])
    with pytest.raises(NotYetImplementedError, match="row-sharded"):
        grid.run_multi(X, y, groups, simulate=SimComm.recorder())
    # a mixed (0/1 plus continuous columns) or a non-binary design: refused, never a wrong answer
    rng = np.random.default_rng(0)
    Xm = X[:2000].copy()
    Xm[:, 5] = rng.normal(0, 1, 2000)
    with pytest.raises(NotYetImplementedError, match="0/1 design"):
        sglm.GLM("Poisson", alpha=.01, l1_ratio=.5).fit(Xm, y[:2000])
    with pytest.raises(NotYetImplementedError, match="0/1 design"):
        sglm.GLM("Poisson", alpha=.01, l1_ratio=.5).fit(rng.normal(0, 1, (2000, 20)), y[:2000])
