"""Binomial (logit link) fits on the MI355X through the public surface -- GLM('Binomial'),
BinomialRegressor, sglm_cv.cv_glm_mult_params, grid.run -- against the float64 Newton oracle of
tests/binomial_cases.py and the sklearn golden (tests/golden/binomial.npz).

Parity bar (the README's for Poisson): max |w - w_ref| <= 1e-4 max |w_ref|, likewise the
intercept (relative to max(1, |b_ref|)); scores within 1e-6."""
import os

import numpy as np
import pytest

import binomial_cases as bc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binomial.npz")
BAR = 1e-4


def coef_err(w, b, w_ref, b_ref):
    """(coefficient error / bar scale, intercept error / bar scale)."""
    return (np.max(np.abs(np.asarray(w) - w_ref)) / np.max(np.abs(w_ref)),
            abs(float(b) - b_ref) / max(1.0, abs(b_ref)))


def check(tag, w, b, w_ref, b_ref):
    ew, eb = coef_err(w, b, w_ref, b_ref)
    print(f"{tag}: coef err {ew:.2e}, intercept err {eb:.2e} (bar {BAR:g})")
    assert ew <= BAR and eb <= BAR, tag


@pytest.mark.parametrize("j", range(len(bc.ALPHAS_A)))
def test_case_a_matches_oracle_and_golden(engine, j):
    import sglm
    alpha = bc.ALPHAS_A[j]
    _, X, y = bc.case_a()
    g = np.load(GOLDEN)
    w_ref, b_ref = bc.oracle("A", alpha)
    scores = {}
    for method in ("mse", "r2"):
        glm = sglm.GLM("Binomial", alpha=alpha, score_method=method)
        glm.fit(X, y)
        check(f"A alpha={alpha:g} vs oracle", glm.coef_, glm.intercept_, w_ref, b_ref)
        scores[method] = glm.score(X, y)
    check(f"A alpha={alpha:g} vs golden", glm.coef_, glm.intercept_, g[f"A{j}_coef"],
          float(g[f"A{j}_intercept"]))
    eta = X @ w_ref + b_ref
    print(f"D2 {scores['r2']:.8f} (oracle {bc.d2(y, eta):.8f}), neg mse {scores['mse']:.8f} "
          f"(oracle {bc.neg_mse(y, eta):.8f})")
    assert abs(scores["r2"] - bc.d2(y, eta)) <= 1e-6
    assert abs(scores["mse"] - bc.neg_mse(y, eta)) <= 1e-6
    res, mres = glm.get_residuals(X, y)
    assert np.max(np.abs(res - (y - bc.sigmoid(eta)))) <= 1e-5
    assert np.array_equal(mres, y - y.mean())


def test_case_s_vanishing_weights(engine):
    from sglm_hip.estimators import BinomialRegressor
    _, X, y = bc.case_s()
    g = np.load(GOLDEN)
    w_ref, b_ref = bc.oracle("S", bc.ALPHA_S)
    m = BinomialRegressor(alpha=bc.ALPHA_S).fit(X, y)
    check("S vs oracle", m.coef_, m.intercept_, w_ref, b_ref)
    check("S vs golden", m.coef_, m.intercept_, g["S_coef"], float(g["S_intercept"]))
    assert m.n_iter_ < 100
    # `converged` as the grid reports it
    from sglm_hip import grid
    r = grid.run(X, y, [(np.arange(0, 4000, 2), np.arange(1, 4000, 2))], [m.objective()], [0])[0]
    assert r["converged"]
    check("S refit in the grid", r["refit_coef"], r["refit_intercept"], w_ref, b_ref)


def test_options_and_predictions(engine):
    from sglm_hip.estimators import BinomialRegressor
    _, X, y = bc.case_a()
    alpha = 1e-2
    w0, _ = bc.oracle("A", alpha, False)
    m = BinomialRegressor(alpha=alpha, fit_intercept=False).fit(X, y)
    assert m.intercept_ == 0.0
    check("fit_intercept=False", m.coef_, 0.0, w0, 0.0)
    # warm start from the oracle's solution: it is returned, in at most 2 iterations
    w_ref, b_ref = bc.oracle("A", alpha)
    ws = BinomialRegressor(alpha=alpha, warm_start=True)
    ws.coef_, ws.intercept_ = w_ref.copy(), b_ref
    ws.fit(X, y)
    check("warm start", ws.coef_, ws.intercept_, w_ref, b_ref)
    assert ws.n_iter_ <= 2
    # labels as bool / int give the same fit
    mb = BinomialRegressor(alpha=alpha).fit(X, y.astype(bool))
    assert np.array_equal(mb.coef_, BinomialRegressor(alpha=alpha).fit(X, y.astype(np.int64)).coef_)
    check("bool labels", mb.coef_, mb.intercept_, w_ref, b_ref)
    mu, eta = mb.predict(X), mb.decision_function(X)
    assert np.all((mu > 0) & (mu < 1))
    assert np.array_equal(mu, bc.sigmoid(eta))
    assert np.max(np.abs(eta - (X @ mb.coef_ + mb.intercept_))) <= 1e-5
    assert abs(mb.score(X, y) - bc.d2(y, X @ w_ref + b_ref)) <= 1e-6


def test_mixed_design(engine):
    """One continuous column next to the 48 event columns (the mixed 0/1 + continuous path)."""
    import sglm
    X, y = bc.case_mixed()
    w_ref, b_ref = bc.oracle("M", 1e-4)
    glm = sglm.GLM("Binomial", alpha=1e-4)
    glm.fit(X, y)
    check("mixed design", glm.coef_, glm.intercept_, w_ref, b_ref)


def fold_scores(alpha, fold, roll, method):
    """Oracle (train, test) score of one fold of Case A."""
    _, X, y = bc.case_a()
    yr = np.roll(y, roll)
    w, b = bc.oracle_rows(alpha, fold, roll)
    f = bc.neg_mse if method == "mse" else bc.d2
    tr, te = bc.group_folds(X.shape[0])[fold]
    return f(yr[tr], X[tr] @ w + b), f(yr[te], X[te] @ w + b)


@pytest.mark.parametrize("method", ["mse", "r2"])
def test_cv_grid(engine, method):
    """3 group folds x 4 alphas and their refits through sglm_cv.cv_glm_mult_params."""
    import sglm_cv
    _, X, y = bc.case_a()
    cv_idx = bc.group_folds(X.shape[0])
    kws = [{"model_name": "Binomial", "alpha": a} for a in bc.ALPHAS_A]
    out = sglm_cv.cv_glm_mult_params(X, y, cv_idx, "Binomial", kws, score_method=method)
    assert len(out["full_cv_results"]) == len(bc.ALPHAS_A)
    for a, r in zip(bc.ALPHAS_A, out["full_cv_results"]):
        for k in range(3):
            w, b = bc.oracle_rows(a, k)
            check(f"alpha={a:g} fold {k}", r["cv_coefs"][:, k], r["cv_intercepts"][k], w, b)
            tr, te = fold_scores(a, k, 0, method)
            assert abs(r["cv_scores_train"][k] - tr) <= 1e-6, (a, k)
            assert abs(r["cv_scores_test"][k] - te) <= 1e-6, (a, k)
        w, b = bc.oracle_rows(a, -1)
        check(f"alpha={a:g} refit", r["model"].coef_, r["model"].intercept_, w, b)
    assert out["best_model"].model_name == "Binomial"


def lag_grid(engine_mod, grid, simulate=None, slab=None, stats=None):
    """grid.run on Case A's lagged event design (device-expanded): 3 folds x (2 alphas on y, one
    on y rolled by 7 rows) and their refits."""
    s, X, y = bc.case_a()
    d = engine_mod.Design.from_events(s.E, s.shifts, s.L - 1, s.N, slab=slab)
    from sglm_hip.estimators import BinomialRegressor
    objs = [BinomialRegressor(alpha=a).objective() for a in (1e-4, 1e-2, 1e-2)]
    return grid.run(d, y, bc.group_folds(s.N), objs, LAG_ROLLS, score_method="r2",
                    simulate=simulate, stats=stats)


LAG_ALPHAS = (1e-4, 1e-2, 1e-2)
LAG_ROLLS = [0, 0, 7]


def test_grid_run_with_rolled_response(engine):
    from sglm_hip import engine as E, grid
    st = E.IrlsStats()
    out = lag_grid(E, grid, stats=st)
    # the refits start at one constant weight mean(y) (1 - mean(y)) on every row: their first
    # Gram comes from the event cross-correlations, as Poisson's does
    print(f"lag Grams {st.lag_grams}, Grams {st.gram_fits}, aliased {st.aliased}, "
          f"reused {st.reused}")
    assert st.lag_grams >= 1
    for a, roll, r in zip(LAG_ALPHAS, LAG_ROLLS, out):
        assert r["converged"]
        for k in range(3):
            w, b = bc.oracle_rows(a, k, roll)
            check(f"alpha={a:g} roll {roll} fold {k}", r["cv_coefs"][:, k], r["cv_intercepts"][k],
                  w, b)
            tr, te = fold_scores(a, k, roll, "r2")
            assert abs(r["cv_scores_train"][k] - tr) <= 1e-6
            assert abs(r["cv_scores_test"][k] - te) <= 1e-6
        w, b = bc.oracle_rows(a, -1)                  # the refit is on the un-rolled response
        check(f"alpha={a:g} roll {roll} refit", r["refit_coef"], r["refit_intercept"], w, b)


def test_row_sharded_two_ranks(engine):
    """A simulated two-rank row-sharded run of that grid (comm.SimComm: each rank's slab fed the
    global sums of the recorded unsharded run) against the unsharded grid, at the tolerance
    tests/test_gpu_sharded.py holds Poisson to: 1e-5 relative on the coefficients."""
    from sglm_hip import engine as E, grid
    from sglm_hip.comm import SimComm, row_slab
    s = bc.case_a()[0]
    full = lag_grid(E, grid, simulate=(0, 1))
    rec = SimComm.recorder()
    a = lag_grid(E, grid, simulate=rec)
    assert len(rec.tape) > 0 and sorted(a) == sorted(full)
    for rank in range(2):
        rp = rec.replay(rank, 2)
        b = lag_grid(E, grid, simulate=rp, slab=row_slab(s.N, rank, 2))
        assert sorted(b) == sorted(full)
        for i in full:
            scale = max(np.max(np.abs(full[i][0])), 1e-30)
            assert np.max(np.abs(b[i][0] - full[i][0])) / scale < 1e-5, (rank, i)
            assert abs(b[i][1] - full[i][1]) <= 1e-5 * max(1.0, abs(full[i][1])), (rank, i)
            assert b[i][3] and full[i][3]


def test_refusals(engine):
    import sglm_cv
    from sglm_hip import grid
    from sglm_hip.estimators import BinomialRegressor, NotYetImplementedError
    _, X, y = bc.case_a()
    n = X.shape[0]
    # a fold whose training labels are all 0
    zeros, ones = np.flatnonzero(y == 0), np.flatnonzero(y == 1)
    cv_idx = [(zeros[:2000], ones[:500]), (np.arange(0, n, 2), np.arange(1, n, 2))]
    with pytest.raises(ValueError, match="all 0 or all 1"):
        sglm_cv.cv_glm_mult_params(X, y, cv_idx, "Binomial",
                                   [{"model_name": "Binomial", "alpha": 1e-2}])
    with pytest.raises(ValueError, match="all 0 or all 1"):
        BinomialRegressor(alpha=1e-2).fit(X[ones], y[ones])
    obj = BinomialRegressor(alpha=1e-2).objective()
    with pytest.raises(NotYetImplementedError):
        grid.run(X, y, bc.group_folds(n), [obj], [0], drop_sets=[[], [0, 1]])
