"""Negative-binomial (NB2, log link, fixed kappa) fits on the MI355X through the public surface --
GLM('NegativeBinomial' | 'NB2'), NegativeBinomialRegressor, sglm_cv.cv_glm_mult_params,
sglm_ez.simple_cv_fit, grid.run -- against the float64 Newton oracle of tests/nb2_cases.py.

Parity bar (the README's for Poisson): max |w - w_ref| <= 1e-4 max |w_ref|, likewise the
intercept (relative to max(1, |b_ref|)); scores within 1e-6."""
import numpy as np
import pytest

import nb2_cases as nc

pytestmark = pytest.mark.gpu

BAR = 1e-4
CV_ALPHAS = nc.ALPHAS_A
CV_KAPPAS = (0.25, 0.3)


def coef_err(w, b, w_ref, b_ref):
    """(coefficient error / bar scale, intercept error / bar scale)."""
    return (np.max(np.abs(np.asarray(w) - w_ref)) / np.max(np.abs(w_ref)),
            abs(float(b) - b_ref) / max(1.0, abs(b_ref)))


def check(tag, w, b, w_ref, b_ref):
    ew, eb = coef_err(w, b, w_ref, b_ref)
    print(f"{tag}: coef err {ew:.2e}, intercept err {eb:.2e} (bar {BAR:g})")
    assert ew <= BAR and eb <= BAR, tag


@pytest.fixture
def solves(engine, monkeypatch):
    """The FitResults of every engine.irls call (the estimators keep no convergence flag)."""
    seen = []
    irls = engine.irls

    def spy(*a, **k):
        out = irls(*a, **k)
        seen.extend(out[0])
        return out
    monkeypatch.setattr(engine, "irls", spy)
    return seen


@pytest.mark.parametrize("alpha", nc.ALPHAS_A)
@pytest.mark.parametrize("kappa", nc.KAPPAS_A)
def test_case_a_matches_oracle(engine, solves, kappa, alpha):
    """Case A with and without intercept: coefficients at the bar, converged, n_iter >= 1;
    predict is exp(eta) and score the D^2 of nb2_cases at the float32-rounded kappa."""
    import sglm
    _, X, y = nc.case_a()
    k = nc.k32(kappa)
    for fi in (True, False):
        w_ref, b_ref = nc.oracle("A", alpha, kappa, fi)
        scores = {}
        for method in ("mse", "r2"):
            glm = sglm.GLM("NegativeBinomial", alpha=alpha, kappa=kappa, fit_intercept=fi,
                           score_method=method)
            glm.fit(X, y)
            check(f"A kappa={kappa:g} alpha={alpha:g} intercept={fi}", glm.coef_, glm.intercept_,
                  w_ref, b_ref)
            assert solves[-1].converged and solves[-1].n_iter >= 1
            scores[method] = glm.score(X, y)
        if not fi:
            assert glm.intercept_ == 0.0
        eta = X @ w_ref + b_ref
        print(f"D2 {scores['r2']:.8f} (oracle {nc.d2(k, y, eta):.8f}), neg mse "
              f"{scores['mse']:.8f} (oracle {nc.neg_mse(y, eta):.8f})")
        assert abs(scores["r2"] - nc.d2(k, y, eta)) <= 1e-6
        assert abs(scores["mse"] - nc.neg_mse(y, eta)) <= 1e-6
    mu = glm.predict(X)
    eta_d = X @ glm.coef_ + glm.intercept_
    assert np.all(mu > 0) and np.max(np.abs(np.log(mu) - eta_d)) <= 1e-5


def test_case_t_saturated_tail(engine, solves):
    from sglm_hip.estimators import NegativeBinomialRegressor
    _, X, y = nc.case_t()
    w_ref, b_ref = nc.oracle("T", nc.ALPHA_T, nc.KAPPA_T)
    assert np.max(nc.KAPPA_T * np.exp(X @ w_ref + b_ref)) >= 100
    m = NegativeBinomialRegressor(kappa=nc.KAPPA_T, alpha=nc.ALPHA_T).fit(X, y)
    check("T vs oracle", m.coef_, m.intercept_, w_ref, b_ref)
    assert solves[-1].converged and 1 <= m.n_iter_ < 100
    assert abs(m.score(X, y) - nc.d2(nc.KAPPA_T, y, X @ w_ref + b_ref)) <= 1e-6


def test_case_z_poisson_limit(engine, solves):
    import sglm
    _, X, y = nc.case_a()
    w_ref, b_ref = nc.oracle("Z", nc.ALPHA_Z, nc.KAPPA_Z)
    glm = sglm.GLM("NB2", alpha=nc.ALPHA_Z, kappa=nc.KAPPA_Z)
    glm.fit(X, y)
    check("Z vs oracle", glm.coef_, glm.intercept_, w_ref, b_ref)
    assert solves[-1].converged and solves[-1].n_iter >= 1
    po = sglm.GLM("Poisson", alpha=nc.ALPHA_Z)
    po.fit(X, y)
    assert np.max(np.abs(glm.coef_ - po.coef_)) <= 1e-3 * np.max(np.abs(po.coef_))


def test_mixed_design_and_warm_start(engine, solves):
    """One continuous column next to the 48 event columns (the mixed 0/1 + continuous path); a
    warm-started refit from the solution stops in one iteration at the same coefficients."""
    import sglm
    from sglm_hip.estimators import NegativeBinomialRegressor
    X, y = nc.case_mixed()
    w_ref, b_ref = nc.oracle("M", nc.ALPHA_M, nc.KAPPA_M)
    glm = sglm.GLM("NegativeBinomial", alpha=nc.ALPHA_M, kappa=nc.KAPPA_M)
    glm.fit(X, y)
    check("mixed design", glm.coef_, glm.intercept_, w_ref, b_ref)
    assert solves[-1].converged and solves[-1].n_iter >= 1
    _, Xa, ya = nc.case_a()
    m = NegativeBinomialRegressor(kappa=1.0, alpha=1e-2, warm_start=True).fit(Xa, ya)
    w1, b1, it1 = m.coef_.copy(), m.intercept_, m.n_iter_
    m.fit(Xa, ya)
    print(f"warm start: {it1} iterations cold, {m.n_iter_} from the solution")
    assert it1 > 1 and m.n_iter_ <= 1 and solves[-1].converged
    check("warm refit", m.coef_, m.intercept_, w1, b1)
    check("warm refit vs oracle", m.coef_, m.intercept_, *nc.oracle("A", 1e-2, 1.0))


def fold_scores(alpha, kappa, fold, roll, method):
    """Oracle (train, test) score of one fold of Case A."""
    _, X, y = nc.case_a()
    yr = np.roll(y, roll)
    w, b = nc.oracle_rows(alpha, kappa, fold, roll)
    k = nc.k32(kappa)
    f = (lambda yy, e: nc.neg_mse(yy, e)) if method == "mse" else (lambda yy, e: nc.d2(k, yy, e))
    tr, te = nc.group_folds(X.shape[0])[fold]
    return f(yr[tr], X[tr] @ w + b), f(yr[te], X[te] @ w + b)


def score_close(got, ref):
    print(f"score {got:.9f} (oracle {ref:.9f}, difference {abs(got - ref):.2e})")
    return abs(got - ref) <= 1e-6


@pytest.mark.parametrize("method", ["mse", "r2"])
def test_cv_grid_mult_params(engine, monkeypatch, method):
    """3 group folds x 4 alphas x 2 kappas and their refits through sglm_cv.cv_glm_mult_params:
    every fit at the bar, scores within 1e-6, one solve group per kappa."""
    import sglm_cv
    groups = []
    irls_scored = engine.irls_scored
    monkeypatch.setattr(engine, "irls_scored",
                        lambda prob, reqs, *a, **k: groups.append(
                            {(r.family, float(r.power)) for r in reqs})
                        or irls_scored(prob, reqs, *a, **k))
    _, X, y = nc.case_a()
    cv_idx = nc.group_folds(X.shape[0])
    params = [(kp, a) for kp in CV_KAPPAS for a in CV_ALPHAS]
    kws = [{"model_name": "NegativeBinomial", "alpha": a, "kappa": kp} for kp, a in params]
    out = sglm_cv.cv_glm_mult_params(X, y, cv_idx, "NegativeBinomial", kws, score_method=method)
    assert len(out["full_cv_results"]) == len(params)
    for (kp, a), r in zip(params, out["full_cv_results"]):
        for k in range(3):
            w, b = nc.oracle_rows(a, kp, k)
            check(f"kappa={kp:g} alpha={a:g} fold {k}", r["cv_coefs"][:, k],
                  r["cv_intercepts"][k], w, b)
            tr, te = fold_scores(a, kp, k, 0, method)
            assert score_close(r["cv_scores_train"][k], tr), (kp, a, k)
            assert score_close(r["cv_scores_test"][k], te), (kp, a, k)
        w, b = nc.oracle_rows(a, kp, -1)
        check(f"kappa={kp:g} alpha={a:g} refit", r["model"].coef_, r["model"].intercept_, w, b)
    assert out["best_model"].model_name == "NegativeBinomial"
    # the two kappas are solved in separate groups, each of one (family, kappa)
    assert all(len(g) == 1 for g in groups)
    assert {next(iter(g)) for g in groups} == {(3, nc.k32(kp)) for kp in CV_KAPPAS}


def test_simple_cv_fit(engine):
    """sglm_ez.simple_cv_fit over the same grid: the fold fits and the best model's refit."""
    import pandas as pd
    import sglm_ez
    _, X, y = nc.case_a()
    cols = [f"x{j}" for j in range(X.shape[1])]
    df = pd.DataFrame(X, columns=cols)
    df["y"] = y
    cv_idx = nc.group_folds(X.shape[0])
    kws = [{"model_name": "NB2", "alpha": a, "kappa": kp} for kp in CV_KAPPAS for a in CV_ALPHAS]
    params = [(d["kappa"], d["alpha"]) for d in kws]
    best_score, best_score_std, best_params, best_model, cv_results = sglm_ez.simple_cv_fit(
        df[cols], df["y"], cv_idx, [dict(d) for d in kws], model_type="NB2", score_method="r2")
    assert len(cv_results["full_cv_results"]) == len(params)
    for (kp, a), r in zip(params, cv_results["full_cv_results"]):
        for k in range(3):
            w, b = nc.oracle_rows(a, kp, k)
            check(f"ez kappa={kp:g} alpha={a:g} fold {k}", r["cv_coefs"][:, k],
                  r["cv_intercepts"][k], w, b)
            assert score_close(r["cv_scores_test"][k], fold_scores(a, kp, k, 0, "r2")[1])
    w, b = nc.oracle_rows(best_params["alpha"], best_params["kappa"], -1)
    check("ez best model", best_model.coef_, best_model.intercept_, w, b)


LAG_PARAMS = ((1e-4, 0.25), (1e-2, 0.25), (1e-2, 0.3))
LAG_ROLLS = [0, 0, 7]


def lag_grid(engine_mod, grid, simulate=None, slab=None, stats=None):
    """grid.run on Case A's lagged event design (device-expanded): 3 folds x (alpha, kappa) in
    LAG_PARAMS, the last on y rolled by 7 rows, and their refits."""
    s, X, y = nc.case_a()
    d = engine_mod.Design.from_events(s.E, s.shifts, s.L - 1, s.N, slab=slab)
    from sglm_hip.estimators import NegativeBinomialRegressor
    objs = [NegativeBinomialRegressor(alpha=a, kappa=kp).objective() for a, kp in LAG_PARAMS]
    return grid.run(d, y, nc.group_folds(s.N), objs, LAG_ROLLS, score_method="r2",
                    simulate=simulate, stats=stats)


def test_lag_design_grid_with_rolled_response(engine, monkeypatch):
    """The lag design with the event-structured Gram forced on (as
    tests/test_gpu_tweedie_enet.py forces it): _lag_gram_w forms the Hessians, the first-Gram
    shortcut from the event correlations stays off (the NB2 weight carries y at the start)."""
    from sglm_hip import grid
    ran = []
    lagw = engine._lag_gram_w
    monkeypatch.setattr(engine, "_lagw_pays", lambda *a: True)
    monkeypatch.setattr(engine, "_lag_gram_w", lambda *a, **k: ran.append(1) or lagw(*a, **k))
    st = engine.IrlsStats()
    out = lag_grid(engine, grid, stats=st)
    print(f"lag-structured Grams {len(ran)} calls, first-Gram shortcut {st.lag_grams}, "
          f"Grams {st.gram_fits}")
    assert len(ran) >= 1 and st.lag_grams == 0
    for (a, kp), roll, r in zip(LAG_PARAMS, LAG_ROLLS, out):
        assert r["converged"]
        for k in range(3):
            w, b = nc.oracle_rows(a, kp, k, roll)
            check(f"lag kappa={kp:g} alpha={a:g} roll {roll} fold {k}", r["cv_coefs"][:, k],
                  r["cv_intercepts"][k], w, b)
            tr, te = fold_scores(a, kp, k, roll, "r2")
            assert score_close(r["cv_scores_train"][k], tr)
            assert score_close(r["cv_scores_test"][k], te)
        w, b = nc.oracle_rows(a, kp, -1)              # the refit is on the un-rolled response
        check(f"lag kappa={kp:g} alpha={a:g} roll {roll} refit", r["refit_coef"],
              r["refit_intercept"], w, b)


def test_row_sharded_two_ranks(engine):
    """A simulated two-rank row-sharded run of that grid (comm.SimComm: each rank's slab fed the
    global sums of the recorded unsharded run) against the unsharded grid, at the tolerance
    tests/test_gpu_binomial.py holds Binomial to: 1e-5 relative on the coefficients."""
    from sglm_hip import grid
    from sglm_hip.comm import SimComm, row_slab
    s = nc.case_a()[0]
    full = lag_grid(engine, grid, simulate=(0, 1))
    rec = SimComm.recorder()
    a = lag_grid(engine, grid, simulate=rec)
    assert len(rec.tape) > 0 and sorted(a) == sorted(full)
    for rank in range(2):
        rp = rec.replay(rank, 2)
        b = lag_grid(engine, grid, simulate=rp, slab=row_slab(s.N, rank, 2))
        assert sorted(b) == sorted(full)
        for i in full:
            scale = max(np.max(np.abs(full[i][0])), 1e-30)
            assert np.max(np.abs(b[i][0] - full[i][0])) / scale < 1e-5, (rank, i)
            assert abs(b[i][1] - full[i][1]) <= 1e-5 * max(1.0, abs(full[i][1])), (rank, i)
            assert b[i][3] and full[i][3]
            for key in ("train", "test"):            # the D^2 scores (constants summed over slabs)
                if key in full[i][4]:
                    assert abs(b[i][4][key] - full[i][4][key]) <= 1e-6, (rank, i, key)


def test_refusals(engine):
    import sglm_cv
    from sglm_hip import grid
    from sglm_hip.estimators import NegativeBinomialRegressor, NotYetImplementedError
    _, X, y = nc.case_a()
    n = X.shape[0]
    # a fold whose training responses are all 0: Poisson's ValueError
    zeros = np.flatnonzero(y == 0)
    cv_idx = [(zeros[:1500], np.arange(1, n, 2)), (np.arange(0, n, 2), np.arange(1, n, 2))]
    with pytest.raises(ValueError, match="out of the valid range"):
        sglm_cv.cv_glm_mult_params(X, y, cv_idx, "NB2",
                                   [{"model_name": "NB2", "alpha": 1e-2, "kappa": 0.5}])
    with pytest.raises(ValueError, match="out of the valid range"):
        NegativeBinomialRegressor(alpha=1e-2).fit(X[zeros], y[zeros])
    obj = NegativeBinomialRegressor(alpha=1e-2, kappa=0.5).objective()
    with pytest.raises(NotYetImplementedError):
        grid.run(X, y, nc.group_folds(n), [obj], [0], drop_sets=[[], [0, 1]])
    with pytest.raises(NotYetImplementedError):
        NegativeBinomialRegressor(alpha=1e-2, l1_ratio=0.5).fit(X, y)
