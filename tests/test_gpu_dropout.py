"""Leave-one-event-out drop-set grids on the MI355X (engine._gram_ls_drop, csrc/chol64_drop.hip).

The oracle throughout is oracle.glm_ref.fit_ols / fit_ridge on the COLUMN-DELETED host float64
matrix restricted to the fold's rows (X[idx]: repeats count); scores are recomputed on the
host in float64 from the oracle's coefficients.  Bars: coefficients and intercepts 1e-5
relative (the README parity bar for Gaussian), scores and pooled R^2 1e-6 (as
tests/test_gpu_api.py holds them); the kernel identity against numpy.linalg.solve on the
submatrix within 1e-10 relative (float64; measured 9e-16 in numpy).  No HIP route is compared
only with another HIP route.
"""
import numpy as np
import pandas as pd
import pytest

from oracle import glm_ref

pytestmark = pytest.mark.gpu
TOL_COEF, TOL_SCORE = 1e-5, 1e-6
M_EV, L_LAG = 4, 5


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


# ------------------------------------------------------------------------------ kernel level
def _drop_kernel_case(P, sets, seed):
    """prep + solve_add on a numpy-factored SPD matrix vs numpy.linalg.solve on the submatrix."""
    import torch
    from sglm_hip import _lib
    rng = np.random.default_rng(seed)
    M = rng.normal(0, 1, (P, P))
    A = M @ M.T / P + np.diag(rng.uniform(0.5, 2.0, P))
    U = np.linalg.cholesky(A).T.copy()
    c = rng.normal(0, 1, (2, P))
    ng = len(sets)
    kmax = max(len(s) for s in sets)
    assert kmax <= _lib.query("sglm_chol64_drop_kmax") and _lib.query("sglm_chol64_drop_kmax") >= 64
    tab = np.zeros((ng, kmax), np.int32)
    for i, s in enumerate(sets):
        tab[i, :len(s)] = s
    dev = "cuda"
    U_d = torch.from_numpy(U[None]).to(dev)
    state = torch.zeros((1, P), dtype=torch.uint8, device=dev)
    counts = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    sets_d = torch.from_numpy(tab).to(dev)
    lens_d = torch.tensor([len(s) for s in sets], dtype=torch.int32, device=dev)
    pf = torch.zeros(ng, dtype=torch.int32, device=dev)
    pg = torch.arange(ng, dtype=torch.int32, device=dev)
    work = torch.empty(_lib.query("sglm_chol64_drop_work_bytes", P, ng, kmax), dtype=torch.uint8,
                       device=dev)
    status = torch.full((ng,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("sglm_chol64_drop_prep", U_d.data_ptr(), P, state.data_ptr(), counts.data_ptr(),
              pf.data_ptr(), pg.data_ptr(), ng, sets_d.data_ptr(), lens_d.data_ptr(), kmax,
              work.data_ptr(), status.data_ptr(), st)
    # fit q = 2 g + r: drop set g, right-hand side r
    nq = 2 * ng
    fits = torch.arange(nq, dtype=torch.int32, device=dev)
    fsrc = torch.zeros(nq, dtype=torch.int32, device=dev)
    gsrc = torch.tensor([q % 2 for q in range(nq)], dtype=torch.int32, device=dev)
    psrc = torch.tensor([q // 2 for q in range(nq)], dtype=torch.int32, device=dev)
    c_d = torch.from_numpy(c).to(dev)
    outs = []
    for _ in range(2):
        x = torch.zeros((nq, P), dtype=torch.float64, device=dev)
        _lib.call("sglm_chol64_drop_solve_add", U_d.data_ptr(), P, state.data_ptr(),
                  fits.data_ptr(), fsrc.data_ptr(), gsrc.data_ptr(), psrc.data_ptr(), nq,
                  c_d.data_ptr(), x.data_ptr(), pg.data_ptr(), ng, sets_d.data_ptr(),
                  lens_d.data_ptr(), kmax, work.data_ptr(), status.data_ptr(), st)
        outs.append(x.cpu().numpy())
    assert np.array_equal(status.cpu().numpy(), np.zeros(ng, np.int32))
    assert np.array_equal(outs[0], outs[1])                     # bitwise repeatable
    for q in range(nq):
        S = np.asarray(sets[q // 2])
        keep = np.setdiff1d(np.arange(P), S)
        ref = np.linalg.solve(A[np.ix_(keep, keep)], c[q % 2][keep])
        err = rel(outs[0][q][keep], ref)
        print(f"P={P} set={sets[q // 2][:3]}..({len(S)}) rhs={q % 2}: rel err {err:.2e}")
        assert err < 1e-10
        assert np.all(outs[0][q][S] == 0.0)


def test_drop_kernels_p128(engine):
    _drop_kernel_case(128, [[17], [0, 1, 2, 3, 4], list(range(60, 69)),
                            [3, 4, 5, 70, 71, 72, 73], list(range(120, 127))], seed=1)


def test_drop_kernels_p256_width41(engine):
    _drop_kernel_case(256, [list(range(100, 141))], seed=2)


# ------------------------------------------------------------------------------ grid level
def _design(n, seed, rank_deficient=False):
    """n x (4 events x 5 lags) 0/1 event design, event-major columns, and a response."""
    rng = np.random.default_rng(seed)
    E = rng.random((n, M_EV)) < 0.06
    if rank_deficient:
        E[:, 1] &= ~E[:, 0]
        E[:, 3] = E[:, 0] | E[:, 1]             # = event 0 + event 1 (disjoint)
    X = np.zeros((n, M_EV * L_LAG))
    for e in range(M_EV):
        for s in range(L_LAG):
            X[s:, e * L_LAG + s] = E[:n - s, e]
    beta = rng.normal(0, 1, M_EV * L_LAG)
    y = X @ beta + 0.7 + rng.normal(0, 0.5, n)
    return X, y


def _folds(n, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    cv = []
    for k in range(3):
        te = np.sort(perm[k::3])
        tr = np.setdiff1d(np.arange(n), te)
        cv.append((tr, te))
    tr0, te0 = cv[0]
    cv[0] = (np.concatenate([tr0, tr0[:57], tr0[5:9]]), te0)      # repeated train rows
    return cv


def _event_cols(*events):
    return sorted(c for e in events for c in range(e * L_LAG, (e + 1) * L_LAG))


DROPS = [[]] + [_event_cols(e) for e in range(M_EV)] + [_event_cols(1, 3)]
_ORACLE = {}


def _oracle(tag, X, y, cv, drop, alpha, fi):
    """Coefficients / scores of one (drop set, alpha, intercept) cell from the column-deleted
    host matrix: per split and for the refit (computed once per session, shared)."""
    key = (tag, tuple(drop), alpha, fi)
    if key in _ORACLE:
        return _ORACLE[key]
    Xd = np.delete(X, drop, axis=1)

    def fit(idx):
        if alpha == 0:
            return glm_ref.fit_ols(Xd[idx], y[idx], fit_intercept=fi)
        return glm_ref.fit_ridge(Xd[idx], y[idx], alpha, fit_intercept=fi)

    out = {"coefs": [], "b": [], "tr": [], "te": []}
    ss_res = ss_tot = 0.0
    for tr, te in cv:
        coef, b = fit(tr)
        out["coefs"].append(coef)
        out["b"].append(b)
        out["tr"].append(-np.mean((y[tr] - Xd[tr] @ coef - b) ** 2))
        r = y[te] - Xd[te] @ coef - b
        out["te"].append(-np.mean(r ** 2))
        ss_res += np.sum(r ** 2)
        ss_tot += np.sum((y[te] - y[te].mean()) ** 2)
    out["R2"] = 1 - ss_res / ss_tot
    out["refit"] = fit(np.arange(len(y)))
    _ORACLE[key] = out
    return out


def _check_grid(tag, X, y, cv, res, alphas, fi):
    p = X.shape[1]
    assert len(res) == len(DROPS)
    for drop, rs in zip(DROPS, res):
        keep = np.setdiff1d(np.arange(p), drop)
        assert len(rs) == len(alphas)
        for alpha, r in zip(alphas, rs):
            o = _oracle(tag, X, y, cv, drop, alpha, fi)
            assert r["cv_coefs"].shape == (p, len(cv)) and r["refit_coef"].shape == (p,)
            assert np.all(r["cv_coefs"][drop] == 0.0) and np.all(r["refit_coef"][drop] == 0.0)
            for k in range(len(cv)):
                e = rel(r["cv_coefs"][keep, k], o["coefs"][k])
                assert e < TOL_COEF, (tag, drop, alpha, fi, k, e)
                assert abs(r["cv_intercepts"][k] - o["b"][k]) < TOL_COEF * max(1, abs(o["b"][k]))
            assert rel(r["refit_coef"][keep], o["refit"][0]) < TOL_COEF, (tag, drop, alpha, fi)
            assert abs(r["refit_intercept"] - o["refit"][1]) < TOL_COEF * max(1, abs(o["refit"][1]))
            assert rel(r["cv_scores_train"], o["tr"]) < TOL_SCORE
            assert rel(r["cv_scores_test"], o["te"]) < TOL_SCORE
            assert abs(r["cv_R2_score"] - o["R2"]) < TOL_SCORE
            assert set(r) == {"cv_coefs", "cv_intercepts", "cv_scores_train", "cv_scores_test",
                              "cv_mean_score_train", "cv_mean_score", "cv_std_score",
                              "cv_R2_score", "cv_mse_score", "refit_coef", "refit_intercept",
                              "n_iter", "converged"}


def _objectives(alphas, fi):
    from sglm_hip.estimators import LinearRegression, Ridge
    return [(LinearRegression(fit_intercept=fi) if a == 0 else
             Ridge(alpha=a, fit_intercept=fi)).objective() for a in alphas]


@pytest.mark.parametrize("route", ["auto", "exclude"])
@pytest.mark.parametrize("fi", [True, False])
def test_grid_drop_sets_well_conditioned(engine, monkeypatch, route, fi):
    from sglm_hip import grid
    monkeypatch.setenv("SGLM_DROP_ROUTE", route)
    n = 3001
    X, y = _design(n, seed=5)
    cv = _folds(n, seed=6)
    alphas = [0, 2.5]
    stats = engine.IrlsStats()
    res = grid.run(X, y, cv, _objectives(alphas, fi), [0, 0], stats=stats, drop_sets=DROPS)
    _check_grid("well", X, y, cv, res, alphas, fi)
    nfit = (len(DROPS) - 1) * len(alphas) * (len(cv) + 1)
    if route == "auto":
        assert stats.drop_reduced == nfit and stats.drop_excluded == 0
    else:
        assert stats.drop_reduced == 0 and stats.drop_excluded == nfit


@pytest.mark.parametrize("route", ["auto", "exclude"])
def test_grid_drop_sets_in_small_chunks(engine, monkeypatch, route):
    """The byte budgets cut to a few slots: one Gram slot, three eta rows and one factor (with
    its W blocks) at a time give the same fits."""
    from sglm_hip import grid
    monkeypatch.setenv("SGLM_DROP_ROUTE", route)
    n = 3001
    X, y = _design(n, seed=5)
    cv = _folds(n, seed=6)
    d = engine.Design.from_host(X)
    monkeypatch.setattr(engine, "GRAM_LS_DROP_BYTES", 12.5 * d.ld)      # 3 eta rows, 1 Gram slot
    monkeypatch.setattr(engine, "GRAM_LS_FACTOR_BYTES", 1.0)
    alphas = [0, 2.5]
    stats = engine.IrlsStats()
    res = grid.run(d, y, cv, _objectives(alphas, True), [0, 0], stats=stats, drop_sets=DROPS)
    _check_grid("well", X, y, cv, res, alphas, True)
    assert stats.drop_reduced + stats.drop_excluded == (len(DROPS) - 1) * 2 * (len(cv) + 1)


@pytest.mark.parametrize("route", ["auto", "exclude"])
def test_grid_drop_sets_rank_deficient(engine, monkeypatch, route):
    """Event 1 disjoint from event 0, event 3 = event 0 + event 1: the full design has rank 16
    of 21; dropping event 0, 1 or 3 leaves full rank, dropping event 2 rank 11 of 16.  alpha = 0
    must give lstsq's minimum-norm answer on the deleted matrix for every drop (the exclusion
    route: the full model's factor has dependent coordinates), alpha = 2.5 fit_ridge's."""
    from sglm_hip import grid
    monkeypatch.setenv("SGLM_DROP_ROUTE", route)
    n = 3001
    X, y = _design(n, seed=7, rank_deficient=True)
    Xa = np.hstack([X, np.ones((n, 1))])
    assert np.linalg.matrix_rank(Xa) == 16
    assert np.linalg.matrix_rank(np.delete(Xa, _event_cols(2), axis=1)) == 11
    cv = _folds(n, seed=8)
    alphas = [0, 2.5]
    stats = engine.IrlsStats()
    res = grid.run(X, y, cv, _objectives(alphas, True), [0, 0], stats=stats, drop_sets=DROPS)
    _check_grid("rankdef", X, y, cv, res, alphas, True)
    per_alpha = (len(DROPS) - 1) * (len(cv) + 1)
    if route == "auto":
        assert stats.drop_excluded == per_alpha and stats.drop_reduced == per_alpha
    else:
        assert stats.drop_excluded == 2 * per_alpha


def test_grid_drop_sets_mixed_design(engine):
    """Two continuous columns beside the 0/1 event lags, one of them inside a drop set."""
    from sglm_hip import grid
    n = 1203
    X, y = _design(n, seed=9)
    rng = np.random.default_rng(10)
    X = np.hstack([X, rng.random((n, 2)) ** 2])
    p = X.shape[1]
    y = y + 0.8 * X[:, p - 2] - 0.4 * X[:, p - 1]
    cv = _folds(n, seed=11)
    drops = [[], [p - 1] + _event_cols(2), [0, 7, p - 2]]
    d = engine.Design.from_host(X)
    assert d.k == 2
    stats = engine.IrlsStats()
    res = grid.run(d, y, cv, _objectives([0, 1.5], True), [0, 0], stats=stats, drop_sets=drops)
    assert stats.drop_reduced == 2 * 2 * 4
    for drop, rs in zip(drops, res):
        keep = np.setdiff1d(np.arange(p), drop)
        Xd = X[:, keep]
        for alpha, r in zip([0, 1.5], rs):
            for k, (tr, te) in enumerate(cv + [(np.arange(n), None)]):
                ref = (glm_ref.fit_ols(Xd[tr], y[tr]) if alpha == 0 else
                       glm_ref.fit_ridge(Xd[tr], y[tr], alpha))
                got = (r["cv_coefs"][:, k], r["cv_intercepts"][k]) if te is not None else \
                    (r["refit_coef"], r["refit_intercept"])
                assert rel(got[0][keep], ref[0]) < TOL_COEF, (drop, alpha, k)
                assert abs(got[1] - ref[1]) < TOL_COEF * max(1, abs(ref[1]))
                assert np.all(got[0][drop] == 0.0)
                if te is not None:
                    sc = -np.mean((y[te] - Xd[te] @ ref[0] - ref[1]) ** 2)
                    assert abs(r["cv_scores_test"][k] - sc) < TOL_SCORE * abs(sc)


def test_drop_variants_stay_on_their_rows_rank(engine):
    """A rank's share of a sharded grid (simulate=(rank, world): the raw per-fit results) holds
    every drop variant of each of its fit-table rows, and the ranks' rows partition the table."""
    from sglm_hip import grid
    n = 900
    X, y = _design(n, seed=18)
    cv = _folds(n, seed=19)
    objs = _objectives([0, 2.5], True)
    drops = DROPS[:3]
    shares = [grid.run(X, y, cv, objs, [0, 0], drop_sets=drops, simulate=(r, 2)) for r in range(2)]
    rows = [sorted({i for i, _ in s}) for s in shares]
    assert rows[0] and rows[1] and not set(rows[0]) & set(rows[1])
    assert sorted(rows[0] + rows[1]) == list(range(len(objs) * (len(cv) + 1)))
    for s, rw in zip(shares, rows):
        assert sorted(s) == [(i, v) for i in rw for v in range(len(drops))]
    # a variant solved in a share is the fit of the column-deleted matrix
    i, v = next(k for k in shares[1] if k[1] == 2)
    j, k = divmod(i, len(cv) + 1)
    idx = cv[k][0] if k < len(cv) else np.arange(n)
    Xd = np.delete(X, drops[2], axis=1)
    ref = glm_ref.fit_ols(Xd[idx], y[idx]) if j == 0 else glm_ref.fit_ridge(Xd[idx], y[idx], 2.5)
    keep = np.setdiff1d(np.arange(X.shape[1]), drops[2])
    assert rel(shares[1][(i, v)][0][keep], ref[0]) < TOL_COEF


# ------------------------------------------------------------------------------ drop-in
def _frames(n, seed):
    """A base frame of 3 event columns, its lagged DataFrame and LagFrame (shifts 0, 1, 2)."""
    import sglm_ez
    from sglm_hip.lagframe import LagFrame
    rng = np.random.default_rng(seed)
    base = pd.DataFrame({c: (rng.random(n) < 0.07).astype(np.float64) for c in ("ev_a", "ev_b", "lick")})
    lag = sglm_ez.timeshift_cols(base, ["ev_a", "ev_b", "lick"], neg_order=0, pos_order=2)
    assert isinstance(lag, LagFrame)
    rows = np.arange(2, n)                                  # the drivers' NaN-row drop
    lag = lag.iloc[rows]
    df = lag.to_pandas().reset_index(drop=True)
    lag = sglm_ez.timeshift_cols(base, ["ev_a", "ev_b", "lick"], neg_order=0, pos_order=2).iloc[rows]
    Xh = df.to_numpy(dtype=np.float64)
    y = Xh @ rng.normal(0, 1, Xh.shape[1]) + 0.3 + rng.normal(0, 0.4, len(df))
    return df, lag, pd.Series(y)


@pytest.mark.parametrize("kind", ["dataframe", "lagframe"])
def test_leave_one_out_cv_fit_vs_simple_cv_fit_loop(engine, kind):
    import sglm_ez
    n = 1500
    df, lag, y = _frames(n, seed=12)
    m = len(df)
    X = df if kind == "dataframe" else lag
    assert list(X.columns) == list(df.columns)
    hold = np.arange(m - 300, m)
    setup = np.arange(m - 300)
    cv = _folds(len(setup), seed=13)
    kws = lambda: [{"alpha": 0, "l1_ratio": 0}, {"alpha": 3.0, "l1_ratio": 0}]     # noqa: E731
    left = [[], ["ev_a"], ["lick"], ["ev_a", "ev_b"]]
    out = sglm_ez.leave_one_out_cv_fit(X, y, cv, kws(), left, X_holdout=hold)
    assert list(out) == [(), ("ev_a",), ("lick",), ("ev_a", "ev_b")]
    Xh, yh = df.to_numpy(dtype=np.float64), y.to_numpy()
    for lo in left:
        cols = [c for c in df.columns if not any(c == b or c.startswith(b + "_") for b in lo)]
        got = out[tuple(lo)]
        assert len(got) == 7
        Xs = df.iloc[setup][cols].reset_index(drop=True)
        ys = y.iloc[setup].reset_index(drop=True)
        ref = sglm_ez.simple_cv_fit(Xs, ys, cv, kws())
        assert got[2] == ref[2]                                  # best params
        assert abs(got[0] - ref[0]) < TOL_SCORE * max(1, abs(ref[0]))
        assert got[3].model.n_features_in_ == len(cols) == got[3].coef_.shape[0]
        assert rel(got[3].coef_, ref[3].coef_) < TOL_COEF
        for a, b in zip(got[4]["full_cv_results"], ref[4]["full_cv_results"]):
            assert a["cv_coefs"].shape == b["cv_coefs"].shape == (len(cols), len(cv))
            assert rel(a["cv_coefs"], b["cv_coefs"]) < TOL_COEF
            assert rel(a["cv_scores_test"], b["cv_scores_test"]) < TOL_SCORE
        # both against the oracle, and the holdout scores of the best refit
        j = [k["alpha"] for k in kws()].index(got[2]["alpha"])
        Xd = df[cols].to_numpy(dtype=np.float64)
        for alpha, a, b in zip([0, 3.0], got[4]["full_cv_results"], ref[4]["full_cv_results"]):
            o = glm_ref.fit_ols(Xd[setup], yh[setup]) if alpha == 0 else \
                glm_ref.fit_ridge(Xd[setup], yh[setup], alpha)
            assert rel(a["model"].coef_, o[0]) < TOL_COEF and rel(b["model"].coef_, o[0]) < TOL_COEF
            assert abs(a["model"].intercept_ - o[1]) < TOL_COEF * max(1, abs(o[1]))
            r = yh[hold] - Xd[hold] @ o[0] - o[1]
            r2 = 1 - np.sum(r ** 2) / np.sum((yh[hold] - yh[hold].mean()) ** 2)
            assert abs(a["holdout_score"] - r2) < TOL_SCORE
            assert abs(a["holdout_neg_mse_score"] + np.mean(r ** 2)) < TOL_SCORE * np.mean(r ** 2)
            if alpha == [0, 3.0][j]:
                assert got[5] == a["holdout_score"] and got[6] == a["holdout_neg_mse_score"]
    assert Xh.shape[1] == 9
    if kind == "dataframe":
        # holdout data given as frames: the same holdout scores as the row-index form
        out2 = sglm_ez.leave_one_out_cv_fit(
            df.iloc[setup].reset_index(drop=True), y.iloc[setup].reset_index(drop=True), cv,
            kws(), [[], ["lick"]], X_holdout=df.iloc[hold], y_holdout=y.iloc[hold])
        for lo in ((), ("lick",)):
            cols = [c for c in df.columns if not any(c == b or c.startswith(b + "_") for b in lo)]
            Xd = df[cols].to_numpy(dtype=np.float64)
            alpha = out2[lo][2]["alpha"]
            o = glm_ref.fit_ols(Xd[setup], yh[setup]) if alpha == 0 else \
                glm_ref.fit_ridge(Xd[setup], yh[setup], alpha)
            r = yh[hold] - Xd[hold] @ o[0] - o[1]
            r2 = 1 - np.sum(r ** 2) / np.sum((yh[hold] - yh[hold].mean()) ** 2)
            assert abs(out2[lo][5] - r2) < TOL_SCORE
            assert abs(out2[lo][6] + np.mean(r ** 2)) < TOL_SCORE * np.mean(r ** 2)
            assert out2[lo][2] == out[lo][2] and rel(out2[lo][3].coef_, o[0]) < TOL_COEF


# ------------------------------------------------------------------------------ error paths
def test_drop_sets_refused_off_the_gram_path(engine):
    from sglm_hip import grid
    from sglm_hip.estimators import NotYetImplementedError, PoissonRegressor
    n = 600
    X, y = _design(n, seed=14)
    cv = _folds(n, seed=15)
    with pytest.raises(NotYetImplementedError, match="log-link"):
        grid.run(X, np.abs(y), cv, [PoissonRegressor(alpha=1.0).objective()], [0],
                 drop_sets=[[], [0, 1]])
    # the engine's own check (requests built by hand)
    d = engine.Design.from_host(X)
    prob = engine.Problem.from_index_lists(d, np.abs(y), [0], [(None, False)])
    req = engine.FitReq(engine.FAM_TWEEDIE_LOG, 1.0, 1.0, 0, 0, drop=0)
    with pytest.raises(NotYetImplementedError, match="log-link"):
        engine.irls(prob, [req], drop_sets=[[0, 1]])
    with pytest.raises(ValueError):
        engine.irls(prob, [engine.FitReq(engine.FAM_SQUARED, 0.0, 1.0, 0, 0, drop=0)])


def test_drop_sets_none_is_todays_output(engine):
    from sglm_hip import grid
    n = 900
    X, y = _design(n, seed=16)
    cv = _folds(n, seed=17)
    objs = _objectives([0, 2.5], True)
    a = grid.run(X, y, cv, objs, [0, 0])
    b = grid.run(X, y, cv, objs, [0, 0], drop_sets=None)
    assert len(a) == len(b) == 2
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    # the full model of a drop-set run is the same fit
    c = grid.run(X, y, cv, objs, [0, 0], drop_sets=[[], [3]])
    for ra, rc in zip(a, c[0]):
        assert rel(rc["cv_coefs"], ra["cv_coefs"]) < 1e-12
