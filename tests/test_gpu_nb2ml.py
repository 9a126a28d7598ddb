"""NB2 dispersion by maximum likelihood and the log-likelihood score on the MI355X through the
public surface -- nb2.kappa_profile, NegativeBinomialRegressor(kappa='ml'), GLM('NB2',
kappa='ml'), score_method='ll' in sglm_cv.cv_glm_mult_params / sglm_ez.simple_cv_fit / grid.run --
against the CPU oracle of tests/nb2ml_cases.py.

Bars: ln kappa of a profile within 1e-5 of the oracle's (the project's Gaussian coefficient bar);
ln kappa_ of an ML fit within 5e-6 of the exact alternation (10 x the oracle-side gap between the
product's stop rule and the exact one, tests/test_nb2ml_cpu.py); coefficients within 1e-4 max|w| of
the float64 Newton fit at exactly kappa_ (the bar of tests/test_gpu_nb2.py); 'll' scores within
1e-6 relative of the oracle's mean logpmf."""
import math
import warnings

import numpy as np
import pytest

import nb2_cases as nc
import nb2ml_cases as mc

pytestmark = pytest.mark.gpu

BAR = 1e-4


def check(tag, w, b, w_ref, b_ref):
    ew = np.max(np.abs(np.asarray(w) - w_ref)) / np.max(np.abs(w_ref))
    eb = abs(float(b) - b_ref) / max(1.0, abs(b_ref))
    print(f"{tag}: coef err {ew:.2e}, intercept err {eb:.2e} (bar {BAR:g})")
    assert ew <= BAR and eb <= BAR, tag


def test_kappa_profile_batched(engine):
    """Case A, the oracle's coefficients at alpha 1e-2, kappa 0.25: the refit on every row and
    the three group folds' training sets in one call."""
    from sglm_hip import nb2
    _, X, y = nc.case_a()
    folds = nc.group_folds(X.shape[0])
    rows = [None] + [tr for tr, _ in folds]
    fits = [nc.oracle_rows(1e-2, 0.25, f) for f in (-1, 0, 1, 2)]
    ref = []
    for r, (w, b) in zip(rows, fits):
        rr = np.arange(X.shape[0]) if r is None else r
        k, at_bound = mc.kappa_profile(y[rr], X[rr] @ w + b)
        assert not at_bound
        ref.append(k)
    assert np.allclose(ref, [0.5380, 0.5193, 0.4855, 0.5742], atol=5e-5)
    kappa, at_bound = nb2.kappa_profile(X, y, np.stack([w for w, _ in fits]),
                                        [b for _, b in fits], rows=rows)
    err = np.abs(np.log(kappa) - np.log(ref))
    print(f"kappa_profile {kappa}, oracle {ref}, worst |d ln kappa| = {err.max():.3g} (bar 1e-5)")
    assert not at_bound.any() and err.max() <= 1e-5
    # one fit, every row: the 1-D forms of the arguments
    k1, ab1 = nb2.kappa_profile(X, y, fits[0][0], fits[0][1])
    assert k1.shape == (1,) and k1[0] == kappa[0] and not ab1[0]


def _ml_checks(tag, m, X, y, alpha, exact):
    err = abs(math.log(m.kappa_) - math.log(exact["kappa"]))
    print(f"{tag}: kappa_ {m.kappa_:.9g} (exact {exact['kappa']:.9g}, |d ln kappa| {err:.3g}, "
          f"bar 5e-6), {m.kappa_n_rounds_} rounds, {m.n_iter_} IRLS iterations")
    assert err <= 5e-6
    assert m.kappa_ == float(np.float32(m.kappa_))
    assert m.kappa_n_rounds_ >= 2 and m.kappa_converged_ and not m.kappa_at_bound_
    assert m.n_iter_ >= 2                      # the total over the rounds
    w, b = nc.fit_nb2_newton(X, y, alpha, m.kappa_)
    check(tag, m.coef_, m.intercept_, w, b)
    return w, b


@pytest.mark.parametrize("name", ["A0", "A2", "T", "L"])
def test_ml_fit_dense(engine, name):
    import sglm
    X, y, alpha = mc.ml_case(name)
    exact = mc.ml_oracle(name, True)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="NegativeBinomialRegressor")
        glm = sglm.GLM("NB2", alpha=alpha, kappa="ml", score_method="ll")
        glm.fit(X, y)
    m = glm.model
    assert m.get_params()["kappa"] == "ml"
    w, b = _ml_checks(name, m, X, y, alpha, exact)
    eta = X @ w + b
    # everything that needs a dispersion uses kappa_
    assert abs(m.score(X, y) - nc.d2(m.kappa_, y, eta)) <= 1e-6
    ref = float(np.mean(mc.ll_nb2_rows(m.kappa_, y, eta)))
    got = glm.score(X, y)
    print(f"{name}: mean log-likelihood {got:.9f} (oracle {ref:.9f})")
    assert abs(got - ref) <= 1e-6 * abs(ref)
    assert np.max(np.abs(np.log(glm.predict(X)) - (X @ m.coef_ + m.intercept_))) <= 1e-5


def test_ml_fit_through_a_lagframe(engine, monkeypatch):
    """Case A (alpha 1e-2) from its event frame: the lagged frame stays resident and the
    event-structured Gram forms the Hessians."""
    import pandas as pd
    import sglm_ez
    from sglm_hip.estimators import NegativeBinomialRegressor
    from sglm_hip.lagframe import LagFrame
    s, X, y = nc.case_a()
    ran = []
    lagw = engine._lag_gram_w
    monkeypatch.setattr(engine, "_lagw_pays", lambda *a: True)
    monkeypatch.setattr(engine, "_lag_gram_w", lambda *a, **k: ran.append(1) or lagw(*a, **k))
    Nr, nev = s.E.shape
    ev = [f"e{a}" for a in range(nev)]
    df = pd.DataFrame(s.E.astype(np.float64), columns=ev)
    lf = sglm_ez.timeshift_cols(df, ev, neg_order=-s.L, pos_order=s.L - 1)
    xcols = sglm_ez.add_timeshifts_to_col_list(ev, ev, neg_order=-s.L, pos_order=s.L - 1)
    lf = lf[lf[xcols].isna().sum(axis=1) == 0][xcols]
    assert isinstance(lf, LagFrame) and lf.shape == X.shape
    Xl = np.asarray(lf.to_pandas(), dtype=np.float64)
    m = NegativeBinomialRegressor(alpha=1e-2, kappa="ml").fit(lf, y)
    assert len(ran) >= 1
    _ml_checks("lag frame A2", m, Xl, y, 1e-2, mc.ml_oracle("A2", True))


def test_poisson_limit(engine):
    """Poisson counts on Case A's predictor: the likelihood has no interior maximum in kappa."""
    from sglm_hip.estimators import NegativeBinomialRegressor
    X, y, alpha = mc.ml_case("P")
    assert mc.ml_oracle("P", False)["at_bound"]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = NegativeBinomialRegressor(alpha=alpha, kappa="ml").fit(X, y)
    mine = [w for w in rec if issubclass(w.category, UserWarning)
            and "NegativeBinomialRegressor" in str(w.message)]
    assert len(mine) == 1 and "Poisson limit" in str(mine[0].message)
    assert m.kappa_at_bound_ and m.kappa_converged_ and m.kappa_ == 2.0 ** -20
    w, b = nc.fit_nb2_newton(X, y, alpha, 2.0 ** -20)
    check("Poisson limit", m.coef_, m.intercept_, w, b)


def _rel_close(tag, got, ref):
    print(f"{tag}: {got:.9f} (oracle {ref:.9f}, relative {abs(got - ref) / abs(ref):.2e})")
    return abs(got - ref) <= 1e-6 * abs(ref)


def test_ll_grid_chooses_kappa(engine):
    """cv_glm_mult_params on Case A's group folds: NB2 at alpha 1e-2 x kappa in GRID_KAPPAS with
    score_method='ll'; then the Poisson grid on the same counts scores below the best NB2."""
    import sglm_cv
    _, X, y = nc.case_a()
    cv_idx = nc.group_folds(X.shape[0])
    kws = [{"model_name": "NB2", "alpha": mc.GRID_ALPHA, "kappa": k} for k in mc.GRID_KAPPAS]
    out = sglm_cv.cv_glm_mult_params(X, y, cv_idx, "NB2", kws, score_method="ll")
    for k, r in zip(mc.GRID_KAPPAS, out["full_cv_results"]):
        tr, te = mc.grid_oracle(k)
        for f in range(3):
            assert _rel_close(f"kappa {k:g} fold {f} train", r["cv_scores_train"][f], tr[f])
            assert _rel_close(f"kappa {k:g} fold {f} test", r["cv_scores_test"][f], te[f])
    means = {k: float(np.mean(mc.grid_oracle(k)[1])) for k in mc.GRID_KAPPAS}
    assert out["best_params"]["kappa"] == max(means, key=means.get) == 0.5
    assert abs(out["best_score"] - means[0.5]) <= 1e-6 * abs(means[0.5])
    po = sglm_cv.cv_glm_mult_params(X, y, cv_idx, "Poisson",
                                    [{"model_name": "Poisson", "alpha": mc.GRID_ALPHA}],
                                    score_method="ll")
    tr, te = mc.grid_oracle(None)
    r = po["full_cv_results"][0]
    for f in range(3):
        assert _rel_close(f"Poisson fold {f} train", r["cv_scores_train"][f], tr[f])
        assert _rel_close(f"Poisson fold {f} test", r["cv_scores_test"][f], te[f])
    assert po["best_score"] < out["best_score"]
    assert float(np.mean(te)) < means[0.5]


def test_ll_through_simple_cv_fit(engine):
    import pandas as pd
    import sglm_ez
    _, X, y = nc.case_a()
    cols = [f"x{j}" for j in range(X.shape[1])]
    df = pd.DataFrame(X, columns=cols)
    df["y"] = y
    kws = [{"model_name": "NB2", "alpha": mc.GRID_ALPHA, "kappa": k} for k in mc.GRID_KAPPAS]
    best_score, _, best_params, best_model, res = sglm_ez.simple_cv_fit(
        df[cols], df["y"], nc.group_folds(X.shape[0]), kws, model_type="NB2", score_method="ll")
    assert best_params["kappa"] == 0.5
    ref = float(np.mean(mc.grid_oracle(0.5)[1]))
    assert abs(best_score - ref) <= 1e-6 * abs(ref)
    w, b = nc.oracle_rows(mc.GRID_ALPHA, 0.5, -1)
    check("ll best model", best_model.coef_, best_model.intercept_, w, b)


def test_binomial_ll_is_minus_the_mean_loss(engine):
    import binomial_cases as bc
    import sglm_cv
    _, X, y = bc.case_a()
    cv_idx = bc.group_folds(X.shape[0])
    out = sglm_cv.cv_glm_mult_params(X, y, cv_idx, "Binomial",
                                     [{"model_name": "Binomial", "alpha": 1e-2}],
                                     score_method="ll")
    r = out["full_cv_results"][0]
    for f, (tr, te) in enumerate(cv_idx):
        w, b = bc.oracle_rows(1e-2, f)
        assert _rel_close(f"Binomial fold {f} train", r["cv_scores_train"][f],
                          -float(np.mean(bc.loss(y[tr], X[tr] @ w + b))))
        assert _rel_close(f"Binomial fold {f} test", r["cv_scores_test"][f],
                          -float(np.mean(bc.loss(y[te], X[te] @ w + b))))


def test_refusals(engine):
    import sglm
    import sglm_cv
    from sglm_hip import grid
    from sglm_hip.estimators import (NegativeBinomialRegressor, NotYetImplementedError, Ridge,
                                     TweedieRegressor)
    _, X, y = nc.case_a()
    cv_idx = nc.group_folds(X.shape[0])
    ml = NegativeBinomialRegressor(alpha=1e-2, kappa="ml")
    with pytest.raises(NotYetImplementedError, match="score_method='ll'"):
        grid.run(X, y, cv_idx, [ml.objective()], [0])
    with pytest.raises(NotYetImplementedError, match="score_method='ll'"):
        sglm_cv.cv_glm_mult_params(X, y, cv_idx, "NB2",
                                   [{"model_name": "NB2", "alpha": 1e-2, "kappa": "ml"}])
    for est, name in ((Ridge(alpha=1.0), "Normal"), (TweedieRegressor(power=2.0), "Gamma")):
        with pytest.raises(NotYetImplementedError, match=name):
            grid.run(X, y + 1, cv_idx, [est.objective()], [0], score_method="ll")
    for name in ("Normal", "Gamma"):
        with pytest.raises(NotYetImplementedError, match=name):
            sglm_cv.cv_glm_mult_params(X, y + 1, cv_idx, name,
                                       [{"model_name": name, "alpha": 1e-2}], score_method="ll")
    obj = NegativeBinomialRegressor(alpha=1e-2, kappa=0.5).objective()
    half = y.copy()
    half[17] = 2.5
    with pytest.raises(ValueError, match="integer counts"):
        grid.run(X, half, cv_idx, [obj], [0], score_method="ll")
    with pytest.raises(ValueError, match="integer counts"):
        ml.fit(X, half)
    grid.run(X, half, cv_idx, [obj], [0], score_method="mse")     # as before: accepted
    huge = y.copy()
    huge[17] = 2.0 ** 20
    with pytest.raises(NotYetImplementedError, match="2\\^20"):
        grid.run(X, huge, cv_idx, [obj], [0], score_method="ll")
    with pytest.raises(NotYetImplementedError, match="2\\^20"):
        ml.fit(X, huge)
    with pytest.raises(ValueError, match="integer counts"):
        sglm.GLM("Poisson", alpha=1e-2, score_method="ll").score(X, half)


def test_ll_row_sharded_two_ranks(engine):
    """A simulated two-rank row-sharded 'll' grid on Case A's lag design (comm.SimComm, as
    tests/test_gpu_nb2.py runs it): the maximum, the histograms and the flags of count_tails are
    reduced over the slabs, so each rank's scores equal the unsharded grid's to 1e-6."""
    from sglm_hip import grid
    from sglm_hip.comm import SimComm, row_slab
    from sglm_hip.estimators import NegativeBinomialRegressor
    s, X, y = nc.case_a()
    objs = [NegativeBinomialRegressor(alpha=1e-2, kappa=k).objective() for k in (0.25, 0.5)]

    def run(simulate, slab=None):
        d = engine.Design.from_events(s.E, s.shifts, s.L - 1, s.N, slab=slab)
        return grid.run(d, y, nc.group_folds(s.N), objs, [0, 0], score_method="ll",
                        simulate=simulate)
    full = run((0, 1))
    rec = SimComm.recorder()
    assert sorted(run(rec)) == sorted(full) and len(rec.tape) > 0
    for rank in range(2):
        b = run(rec.replay(rank, 2), slab=row_slab(s.N, rank, 2))
        for i in full:
            for key in ("train", "test"):
                if key in full[i][4]:
                    assert abs(b[i][4][key] - full[i][4][key]) <= 1e-6 * abs(full[i][4][key]), (
                        rank, i, key)
    # and the unsharded scores are the oracle's
    for j, k in enumerate((0.25, 0.5)):
        tr, te = mc.grid_oracle(k)
        for f in range(3):
            assert _rel_close(f"lag kappa {k:g} fold {f} test", full[j * 4 + f][4]["test"], te[f])
