"""Host-side parts of the elastic-net penalised Poisson / Gamma / Tweedie fits (no device): the
public surface (l1_ratio on TweedieRegressor / PoissonRegressor / GLM), the objective kinds and
their penalty scaling, the new entry points in the built library, and the committed float64
oracle fixture (tests/golden/tweedie_enet.npz): its fits meet the KKT conditions of the
objective, recomputed here independently, and keep the margins that make their zero sets
robust."""
import numpy as np
import pytest

MARGIN = 1e-3


def test_objective_kinds_and_penalty_scaling():
    import sglm
    from sglm_hip import engine as E
    from sglm_hip.estimators import ElasticNet, PoissonRegressor, TweedieRegressor
    o = PoissonRegressor(alpha=0.1, l1_ratio=0.5).objective()
    assert (o.kind, o.family, o.power, o.l1_ratio) == ("pn", E.FAM_TWEEDIE_LOG, 1.0, 0.5)
    n = 1234.0
    assert o.l1(n) == 0.1 * 0.5 * n and o.l2(n) == 0.1 * (1 - 0.5) * n
    o = TweedieRegressor(power=1.5, alpha=0.3, l1_ratio=1.0, fit_intercept=False).objective()
    assert (o.kind, o.power, o.fit_intercept) == ("pn", 1.5, False)
    assert o.l1(10.0) == 0.3 * 10.0 and o.l2(10.0) == 0.0
    # l1_ratio == 0 or alpha == 0: the IRLS objective, exactly as without the argument
    for kw in ({"alpha": 0.1}, {"alpha": 0.0, "l1_ratio": 0.7}, {"alpha": 0.1, "l1_ratio": 0}):
        o = TweedieRegressor(power=2.0, **kw).objective()
        ref = TweedieRegressor(power=2.0, alpha=kw["alpha"]).objective()
        assert o.kind == "irls" and o == ref
    # the drop-in GLM passes the kwarg through for every log-link family
    for name, kw in (("Poisson", {}), ("Gamma", {}), ("Tweedie", {"power": 1.5})):
        g = sglm.GLM(name, alpha=.1, l1_ratio=.5, **kw)
        assert g.model.objective().kind == "pn"
        assert g.model.get_params()["l1_ratio"] == .5
    assert sglm.GLM("Poisson", alpha=.1).model.objective().kind == "irls"
    with pytest.raises(TypeError):
        sglm.GLM("Poisson", reg_lambda=0)
    # power 0 with the identity link is the coordinate-descent objective ElasticNet builds
    o = TweedieRegressor(power=0, alpha=0.2, l1_ratio=0.4, fit_intercept=False).objective()
    assert o == ElasticNet(alpha=0.2, l1_ratio=0.4, fit_intercept=False).objective()
    assert o.kind == "cd" and o.family == E.FAM_SQUARED


def test_l1_ratio_range_and_params():
    from sglm_hip.estimators import PoissonRegressor, TweedieRegressor
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="l1_ratio"):
            TweedieRegressor(power=1, alpha=1.0, l1_ratio=bad).objective()
        with pytest.raises(ValueError, match="l1_ratio"):
            PoissonRegressor(alpha=1.0, l1_ratio=bad).objective()
    m = PoissonRegressor()
    assert m.get_params()["l1_ratio"] == 0.0
    assert m.set_params(l1_ratio=0.25).l1_ratio == 0.25
    assert TweedieRegressor().get_params()["l1_ratio"] == 0.0


def test_fitreq_keeps_its_positional_form_and_gains_l1():
    from sglm_hip import engine
    r = engine.FitReq(engine.FAM_TWEEDIE_LOG, 1.0, 2.0, 0, 0, True, 50, None, None)
    assert r.l1 == 0.0 and r.drop == -1
    assert engine.FitReq(engine.FAM_TWEEDIE_LOG, 1.0, 2.0, 0, 0, l1=3.0).l1 == 3.0
    s = engine.IrlsStats()
    assert s.pn_fit_iters == 0 and s.cd_full_sweeps == 0 and s.cd_active_sweeps == 0


def test_library_exports_the_proximal_newton_entry_points():
    from sglm_hip import _lib
    lib = _lib.load()
    for name in ("sglm_pn_model", "sglm_enet_cd_warm", "sglm_pn_step", "sglm_pn_update"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_unsupported_grids_raise_without_a_device():
    from sglm_hip import grid
    from sglm_hip.comm import SimComm
    from sglm_hip.estimators import NotYetImplementedError, PoissonRegressor
    X = np.zeros((30, 5))
    y = np.zeros(30)
    groups = [{"cv_idx": [(np.arange(20), np.arange(20, 30))],
               "objectives": [PoissonRegressor(alpha=1.0, l1_ratio=0.5).objective()],
               "rolls": [0]}]
    with pytest.raises(NotYetImplementedError, match="log-link"):
        grid.run_multi(X, y, groups, drop_sets=[[], [1]])
    with pytest.raises(NotYetImplementedError, match="row-sharded"):
        grid.run_multi(X, y, groups, simulate=SimComm.recorder())


# ---- the oracle fixture ---------------------------------------------------------------------

def _design(E, K=8):
    N = E.shape[0] - K
    return np.concatenate([E[K - s:N + K - s] for s in range(K)], axis=1).astype(np.float64)


def _grad(power, X, y, w, b):
    """X~^T loss'(y, X w + b) of the half-Tweedie loss with the log link (p + 1 entries)."""
    eta = X @ w + b
    if power == 1.0:
        r = np.exp(eta) - y
    elif power == 2.0:
        r = 1.0 - y * np.exp(-eta)
    else:
        r = np.exp((2.0 - power) * eta) - y * np.exp((1.0 - power) * eta)
    return np.concatenate([X.T @ r, [r.sum()]])


def _check(power, X, y, w, b, alpha, rho, fit_intercept, slack_bound=MARGIN):
    n, p = X.shape
    l1, l2 = alpha * rho * n, alpha * (1.0 - rho) * n
    g = _grad(power, X, y, w, b)
    gs = g[:p] + l2 * w
    nz = w != 0
    viol = np.abs(gs[nz] + l1 * np.sign(w[nz])).max(initial=0.0)
    viol = max(viol, np.maximum(np.abs(gs[~nz]) - l1, 0.0).max(initial=0.0))
    if fit_intercept:
        viol = max(viol, abs(g[p]))
    else:
        assert b == 0.0
    assert viol <= 1e-10 * n, f"KKT violation {viol:.3e}"
    if (~nz).any():
        assert np.abs(gs[~nz]).max() <= (1.0 - slack_bound) * l1
    if nz.any():
        assert np.abs(w[nz]).min() >= MARGIN * np.abs(w).max()


def test_oracle_single_fits_meet_kkt_and_margins(golden):
    G = golden("tweedie_enet.npz")
    X, y = _design(G["E"].astype(bool)), G["y"]
    assert X.shape == (6000, 48) and len(G["case_power"]) == 7
    for c, (power, alpha, rho) in enumerate(zip(G["case_power"], G["case_alpha"],
                                                G["case_rho"])):
        yy = y + 0.5 if power == 2.0 else y
        for fi in (1, 0):
            _check(float(power), X, yy, G["coef"][c, fi], float(G["intercept"][c, fi]),
                   float(alpha), float(rho), bool(fi))
    zeros = (G["coef"] == 0).sum(axis=2)
    assert zeros[:, 1].min() >= 17 and zeros[:, 1].max() <= 38        # with intercept
    assert zeros[:, 0].min() >= 2 and zeros[:, 0].max() <= 37         # without


def test_oracle_grid_fits_meet_kkt_and_margins(golden):
    """The fold fits keep both margins.  The refits are fits on all rows, which no fold seed
    moves; the one at alpha = 0.005 has a zero coefficient at 0.99927 l1 (slack 7.27e-4), so the
    refits' zero-coefficient slack is only required to be positive (their stored value is
    checked against the recomputed one), their non-zero margin as everywhere."""
    G = golden("tweedie_enet.npz")
    X, y = _design(G["E"].astype(bool)), G["y"]
    rho = float(G["grid_rho"])
    for j, alpha in enumerate(G["grid_alpha"]):
        for k in range(3):
            tr = G[f"fold{k}_train"]
            _check(1.0, X[tr], y[tr], G["grid_coef"][j, k], float(G["grid_intercept"][j, k]),
                   float(alpha), rho, True)
        w, b = G["grid_refit_coef"][j], float(G["grid_refit_intercept"][j])
        _check(1.0, X, y, w, b, float(alpha), rho, True, slack_bound=0.0)
        n = X.shape[0]
        gs = _grad(1.0, X, y, w, b)[:-1] + alpha * (1 - rho) * n * w
        slack = 1.0 - np.abs(gs[w == 0]).max() / (alpha * rho * n)
        assert slack > 0 and abs(slack - G["grid_refit_slack"][j]) <= 1e-9
    assert G["grid_refit_slack"].min() == pytest.approx(7.27e-4, abs=1e-6)


def test_fold_lists_are_the_reference_split(golden):
    """The stored folds are sglm_ez.cv_idx_by_trial_id(num_folds=3) on trial id t // 100 with
    np.random.seed(3) -- what the grid test hands to cv_glm_mult_params."""
    import pandas as pd
    import sglm_ez
    G = golden("tweedie_enet.npz")
    np.random.seed(3)
    cv = sglm_ez.cv_idx_by_trial_id(pd.DataFrame({"nTrial": np.arange(6000) // 100}),
                                    trial_id_columns=["nTrial"], num_folds=3)
    assert len(cv) == 3
    for k, (tr, te) in enumerate(cv):
        assert np.array_equal(tr, G[f"fold{k}_train"]) and np.array_equal(te, G[f"fold{k}_test"])
