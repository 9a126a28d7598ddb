"""Group lasso through the public interface on the MI355X, against the numpy block-descent
oracle of glasso_cases on X[idx] (repeats count): estimator, GLM dispatch, fit_set, CV grids,
the multi-response path, mixed solve groups and the refusals.

Bars: coefficients and intercepts 1e-5 relative (the README parity bar for Gaussian) with
identical zero groups; scores and pooled scores 1e-6 against host float64 scores recomputed
from the ORACLE's coefficients (the bars of tests/test_gpu_dropout.py)."""
import numpy as np
import pandas as pd
import pytest

import glasso_cases as C

pytestmark = pytest.mark.gpu
TOL_COEF, TOL_SCORE = 1e-5, 1e-6


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / (s if s else 1.0)


def same_fit(tag, w, b, w_ref, b_ref, ids):
    goff, gcols = C.csr(ids)
    e = rel(w, w_ref)
    assert e < TOL_COEF, (tag, e)
    assert abs(b - b_ref) < TOL_COEF * max(1.0, abs(b_ref)), (tag, b, b_ref)
    zk, zr = C.zero_groups(np.asarray(w), goff, gcols), C.zero_groups(w_ref, goff, gcols)
    assert np.array_equal(zk, zr), (tag, zk, zr)
    return e


def objectives(ids, fit_intercept=True):
    from sglm_hip.estimators import GroupLasso
    return [GroupLasso(a, groups=ids, l1_ratio=rho, fit_intercept=fit_intercept).objective()
            for rho in C.RHOS for a in C.ALPHAS]


KEYS = [(a, rho) for rho in C.RHOS for a in C.ALPHAS]


@pytest.mark.parametrize("fit_intercept", [True, False])
def test_estimator_glm_and_fit_set_against_the_oracle(engine, fit_intercept):
    import sglm
    from sglm_hip.estimators import GroupLasso
    X, y, ids = C.case("6x5")
    n, p = X.shape
    rng = np.random.default_rng(4)
    idx = np.sort(rng.integers(0, n, size=n))            # a train list with repeated rows
    assert np.unique(idx).size < idx.size
    Xt, yt = np.ascontiguousarray(X[idx]), y[idx]
    worst = 0.0
    for alpha, rho in ((0.01, 1.0), (0.03, 0.5), (0.002, 0.5)):
        w_ref, b_ref, _ = C.fit(Xt, yt, alpha, rho, ids, fit_intercept)
        m = GroupLasso(alpha, groups=ids, l1_ratio=rho, fit_intercept=fit_intercept).fit(Xt, yt)
        worst = max(worst, same_fit(("GroupLasso", alpha, rho), m.coef_, m.intercept_, w_ref,
                                    b_ref, ids))
        assert m.n_iter_ >= 1 and m.n_features_in_ == p
        pred = m.predict(X)
        ref_pred = X @ w_ref + b_ref
        assert rel(pred, ref_pred) < 1e-4                # the f32 linear predictor
        r2 = 1 - np.sum((y - ref_pred) ** 2) / np.sum((y - y.mean()) ** 2)
        assert abs(m.score(X, y) - r2) < 1e-4
        glm = sglm.GLM("Normal", alpha=alpha, l1_ratio=rho, groups=ids,
                       fit_intercept=fit_intercept)
        glm.fit(Xt, yt)
        assert np.array_equal(glm.coef_, m.coef_) and glm.intercept_ == m.intercept_
        # fit_set on the rows of the list
        te = np.setdiff1d(np.arange(n), idx)
        cv_coefs, cv_b = np.zeros((p, 1)), np.zeros(1)
        s_tr, s_te = np.zeros(1), np.zeros(1)
        glm2 = sglm.GLM("Gaussian", alpha=alpha, l1_ratio=rho, groups=ids,
                        fit_intercept=fit_intercept)
        glm2.fit_set(Xt, yt, np.ascontiguousarray(X[te]), y[te], cv_coefs, cv_b, s_tr, s_te, 0,
                     resids=[], mean_resids=[])
        same_fit(("fit_set", alpha, rho), cv_coefs[:, 0], cv_b[0], w_ref, b_ref, ids)
        mse_te = -np.mean((y[te] - X[te] @ w_ref - b_ref) ** 2)
        assert abs(s_te[0] - mse_te) < 1e-4 * abs(mse_te)
    print(f"estimator (fit_intercept={fit_intercept}): worst distance {worst:.2e}")
    # alpha == 0 is LinearRegression
    from oracle import glm_ref
    m0 = GroupLasso(0.0, groups=ids, fit_intercept=fit_intercept).fit(Xt, yt)
    w0, b0 = glm_ref.fit_ols(Xt, yt, fit_intercept)
    assert rel(m0.coef_, w0) < TOL_COEF


@pytest.fixture(scope="module")
def grid_runs(engine):
    """grid.run of ALPHAS x RHOS over 3 folds, per (case, fit_intercept, score method)."""
    from sglm_hip import grid
    out = {}

    def get(name, fi, method):
        key = (name, fi, method)
        if key not in out:
            X, y, ids = C.case(name)
            cv, _ = C.grid_oracle(name, fi)
            out[key] = grid.run(np.array(X), np.array(y), cv, objectives(ids, fi),
                                [0] * len(KEYS), score_method=method)
        return out[key]
    return get


@pytest.mark.parametrize("name,fit_intercept,method", [("6x5", True, "mse"), ("6x5", False, "r2"),
                                                       ("8x12", True, "r2")])
def test_grid_against_the_oracle_per_cell(grid_runs, name, fit_intercept, method):
    X, y, ids = C.case(name)
    cv, ora = C.grid_oracle(name, fit_intercept)
    res = grid_runs(name, fit_intercept, method)
    assert len(res) == len(KEYS)
    worst = 0.0
    col = 0 if method == "mse" else 1
    for key, r in zip(KEYS, res):
        o = ora[key]
        assert r["converged"], key
        for k in range(len(cv)):
            worst = max(worst, same_fit((name, key, k), r["cv_coefs"][:, k], r["cv_intercepts"][k],
                                        o["coefs"][k], o["b"][k], ids))
        worst = max(worst, same_fit((name, key, "refit"), r["refit_coef"], r["refit_intercept"],
                                    o["refit"][0], o["refit"][1], ids))
        tr = np.array([s[col] for s in o["tr"]])
        te = np.array([s[col] for s in o["te"]])
        assert rel(r["cv_scores_train"], tr) < TOL_SCORE, (key, r["cv_scores_train"], tr)
        assert rel(r["cv_scores_test"], te) < TOL_SCORE, (key, r["cv_scores_test"], te)
        assert abs(r["cv_mean_score"] - te.mean()) < TOL_SCORE * max(1.0, abs(te.mean()))
        assert abs(r["cv_R2_score"] - o["cv_R2_score"]) < TOL_SCORE
        assert abs(r["cv_mse_score"] - o["cv_mse_score"]) < TOL_SCORE * o["cv_mse_score"]
        assert set(r) == {"cv_coefs", "cv_intercepts", "cv_scores_train", "cv_scores_test",
                          "cv_mean_score_train", "cv_mean_score", "cv_std_score", "cv_R2_score",
                          "cv_mse_score", "refit_coef", "refit_intercept", "n_iter", "converged"}
    print(f"grid {name} fit_intercept={fit_intercept}: worst distance {worst:.2e}")


def _kwarg_list(ids):
    return [{"alpha": a, "l1_ratio": rho, "groups": ids} for rho in C.RHOS for a in C.ALPHAS]


@pytest.mark.parametrize("method", ["mse", "r2"])
def test_cv_drivers_select_what_the_oracle_selects(engine, method):
    import sglm_cv
    import sglm_ez
    name = "6x5"
    X, y, ids = C.case(name)
    cv, ora = C.grid_oracle(name, True)
    if method == "mse":
        sc = [np.mean([s[0] for s in ora[k]["te"]]) for k in KEYS]
    else:
        sc = [ora[k]["cv_R2_score"] for k in KEYS]
    best = int(np.argmax(sc))
    assert np.sort(sc)[-1] - np.sort(sc)[-2] > 1e-4      # the choice is well determined
    out = sglm_cv.cv_glm_mult_params(np.array(X), np.array(y), cv, "Normal", _kwarg_list(ids),
                                     score_method=method)
    assert out["best_params"]["alpha"] == KEYS[best][0]
    assert out["best_params"]["l1_ratio"] == KEYS[best][1]
    assert abs(out["best_score"] - sc[best]) < TOL_SCORE * max(1.0, abs(sc[best]))
    same_fit("best model", out["best_model"].coef_, out["best_model"].intercept_,
             ora[KEYS[best]]["refit"][0], ora[KEYS[best]]["refit"][1], ids)
    df = pd.DataFrame(np.array(X), columns=[f"c{j}" for j in range(X.shape[1])])
    ez = sglm_ez.simple_cv_fit(df, pd.Series(np.array(y)), cv, _kwarg_list(ids),
                               model_type="Normal", score_method=method)
    assert ez[2]["alpha"] == KEYS[best][0] and ez[2]["l1_ratio"] == KEYS[best][1]
    assert abs(ez[0] - sc[best]) < TOL_SCORE * max(1.0, abs(sc[best]))


def test_multi_response_path(engine, grid_runs):
    """cv_enet_path(groups=...) with 3 responses: response 0 is the grid's y (same cells as
    grid.run and the oracle); the others are checked against the oracle."""
    from sglm_hip import enet
    name = "6x5"
    X, y, ids = C.case(name)
    cv, ora = C.grid_oracle(name, True)
    Y, path = C.path_oracle(name)
    Y = np.array(Y)
    alphas = list(C.ALPHAS)
    for rho in C.RHOS:
        st = {}
        out = enet.cv_enet_path(np.array(X), Y, cv, alphas, l1_ratio=rho, score_method="mse",
                                stats=st, groups=ids)
        assert st["fits"] == 3 * len(alphas) * (len(cv) + 1)
        gr = grid_runs(name, True, "mse")
        for j, a in enumerate(alphas):
            o, g, r = ora[(a, rho)], gr[KEYS.index((a, rho))], out[0][j]
            assert r["converged"]
            for k in range(len(cv)):
                same_fit(("path", a, rho, k), r["cv_coefs"][:, k], r["cv_intercepts"][k],
                         o["coefs"][k], o["b"][k], ids)
            same_fit(("path refit", a, rho), r["refit_coef"], r["refit_intercept"], *o["refit"],
                     ids)
            assert rel(r["cv_coefs"], g["cv_coefs"]) < 1e-9 and \
                rel(r["refit_coef"], g["refit_coef"]) < 1e-9
            te = np.array([s[0] for s in o["te"]])
            assert rel(r["cv_scores_test"], te) < TOL_SCORE
            assert rel(r["cv_scores_test"], g["cv_scores_test"]) < TOL_SCORE
            assert abs(r["cv_R2_score"] - o["cv_R2_score"]) < TOL_SCORE
            assert abs(r["cv_mse_score"] - o["cv_mse_score"]) < TOL_SCORE * o["cv_mse_score"]
            for resp in (1, 2):                          # the other responses: oracle per fit
                rr = out[resp][j]
                for k in range(len(cv)):
                    w_ref, b_ref, sc, _ = path[(resp, a, rho, k)]
                    same_fit(("path", resp, a, rho, k), rr["cv_coefs"][:, k],
                             rr["cv_intercepts"][k], w_ref, b_ref, ids)
                    assert abs(rr["cv_scores_test"][k] - sc) < TOL_SCORE * abs(sc)
    with pytest.raises(ValueError):
        enet.cv_enet_path(np.array(X), Y, cv, alphas, groups=ids[:-1])


def test_mixed_solve_groups(engine, grid_runs):
    """'gcd', 'cd' and Ridge objectives (and a second grouping) in one call: each cell as the
    separate calls return it."""
    from sglm_hip import grid
    from sglm_hip.estimators import ElasticNet, GroupLasso, Ridge
    name = "6x5"
    X, y, ids = C.case(name)
    cv, ora = C.grid_oracle(name, True)
    pairs = np.arange(X.shape[1]) // 2                   # another grouping: column pairs
    objs = [GroupLasso(0.01, groups=ids).objective(), ElasticNet(0.01, l1_ratio=0.5).objective(),
            Ridge(2.0).objective(), GroupLasso(0.03, groups=ids, l1_ratio=0.5).objective(),
            GroupLasso(0.01, groups=pairs).objective()]
    Xa, ya = np.array(X), np.array(y)
    mixed = grid.run(Xa, ya, cv, objs, [0] * len(objs))
    alone = [grid.run(Xa, ya, cv, [o], [0])[0] for o in objs]
    for j, (a, b) in enumerate(zip(mixed, alone)):
        for k in ("cv_coefs", "cv_intercepts", "refit_coef", "refit_intercept", "cv_scores_train",
                  "cv_scores_test", "cv_R2_score", "cv_mse_score", "n_iter"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (j, k)
    gr = grid_runs(name, True, "mse")
    assert np.array_equal(mixed[0]["cv_coefs"], gr[KEYS.index((0.01, 1.0))]["cv_coefs"])
    same_fit("mixed gcd", mixed[3]["refit_coef"], mixed[3]["refit_intercept"],
             *ora[(0.03, 0.5)]["refit"], ids)
    w_ref, b_ref, _ = C.fit(X, y, 0.01, 1.0, pairs)
    assert rel(mixed[4]["refit_coef"], w_ref) < TOL_COEF
    assert np.array_equal(C.zero_groups(mixed[4]["refit_coef"], *C.csr(pairs)),
                          C.zero_groups(w_ref, *C.csr(pairs)))


def test_refusals(engine):
    import sglm
    from sglm_hip import grid
    from sglm_hip.comm import SimComm
    from sglm_hip.estimators import GroupLasso, NotYetImplementedError
    X, y, ids = C.case("6x5")
    cv = C.folds(X.shape[0])
    obj = GroupLasso(0.01, groups=ids).objective()
    Xa, ya = np.array(X), np.array(y)
    with pytest.raises(NotYetImplementedError, match="GroupLasso"):
        grid.run(Xa, ya, cv, [obj], [0], drop_sets=[[], [0, 1]])
    with pytest.raises(NotYetImplementedError, match="row-sharded"):
        grid.run_multi(Xa, ya, [{"cv_idx": cv, "objectives": [obj], "rolls": [0]}],
                       simulate=SimComm.recorder())
    for name in ("Poisson", "Binomial"):
        with pytest.raises(NotYetImplementedError):
            sglm.GLM(name, alpha=0.01, groups=ids)
    with pytest.raises(ValueError):
        GroupLasso(0.01, groups=ids[:-1]).fit(Xa, ya)
    with pytest.raises(ValueError):                      # a grouping of another length in a grid
        grid.run(Xa, ya, cv, [GroupLasso(0.01, groups=ids[:-1]).objective()], [0])


def test_event_groups_of_a_lagged_frame(engine):
    """sglm_ez.event_groups while the frame is lazy and after it is a plain DataFrame."""
    import sglm_ez
    from sglm_hip.lagframe import LagFrame
    rng = np.random.default_rng(2)
    n = 400
    df = pd.DataFrame({"a": (rng.random(n) < 0.1).astype(float),
                       "ab": (rng.random(n) < 0.1).astype(float),
                       "t": np.arange(n, dtype=float)})
    lf = sglm_ez.timeshift_cols(df, ["a", "ab"], neg_order=-1, pos_order=2)
    assert isinstance(lf, LagFrame) and lf.is_lazy
    g_lazy = sglm_ez.event_groups(lf)
    cols = [str(c) for c in lf.columns]
    plain = pd.DataFrame(np.zeros((1, len(cols))), columns=cols)
    g_plain = sglm_ez.event_groups(plain)
    assert np.array_equal(g_lazy, g_plain)
    by = {c: g for c, g in zip(cols, g_lazy)}
    assert by["a"] == by["a_1"] == by["a_-1"] == by["a_2"]
    assert by["ab"] == by["ab_1"] == by["ab_-1"] and by["a"] != by["ab"] != by["t"]
    assert len(set(g_lazy)) == 3
    for name in ("a", "ab", "t"):
        assert np.flatnonzero(g_lazy == by[name]).tolist() == sglm_ez.left_out_columns(lf, [name])
