"""Host-side parts of the leave-one-event-out drop-set grid (no device): name -> column-set
resolution, reshaping full-length results to the reduced frame, argument validation of
grid.run_multi(..., drop_sets=...), and the new entry points in the built library."""
import numpy as np
import pandas as pd
import pytest


def _lagged_frame():
    import sglm_ez
    base = ["ev_a", "ev_b", "lick"]
    cols = sglm_ez.add_timeshifts_to_col_list(base + ["nTrial"], base, neg_order=-2, pos_order=1)
    return pd.DataFrame(np.zeros((4, len(cols))), columns=cols), cols


def test_left_out_columns_follow_the_shift_naming():
    import sglm_ez
    df, cols = _lagged_frame()
    assert cols == ["ev_a", "ev_b", "lick", "nTrial", "ev_a_-2", "ev_b_-2", "lick_-2",
                    "ev_a_-1", "ev_b_-1", "lick_-1", "ev_a_1", "ev_b_1", "lick_1"]
    assert sglm_ez.left_out_columns(df, []) == []
    assert sglm_ez.left_out_columns(df, ["ev_a"]) == [0, 4, 7, 10]
    assert sglm_ez.left_out_columns(df, ["lick", "ev_a"]) == [0, 2, 4, 6, 7, 9, 10, 12]
    assert sglm_ez.left_out_columns(df, ["nTrial"]) == [3]
    # a name is a whole base name: 'ev' is no column, nor is a shifted name's prefix
    for bad in ("ev", "ev_", "lick_", "missing"):
        with pytest.raises(KeyError):
            sglm_ez.left_out_columns(df, [bad])
    # the reduced frame keeps the frame's column order
    drop = sglm_ez.left_out_columns(df, ["ev_b"])
    kept = [c for i, c in enumerate(cols) if i not in drop]
    assert kept == [c for c in cols if not c.startswith("ev_b")]


def test_reduce_cv_result_shapes_and_order():
    import sglm_ez
    p, K = 7, 3
    rng = np.random.default_rng(0)
    drop = [1, 4, 5]
    keep = [0, 2, 3, 6]
    cvc = rng.normal(size=(p, K))
    cvc[drop] = 0.0
    refit = rng.normal(size=p)
    refit[drop] = 0.0
    r = {"cv_coefs": cvc, "cv_intercepts": np.arange(K, dtype=float),
         "cv_scores_train": -np.ones(K), "cv_scores_test": -2 * np.ones(K),
         "cv_mean_score_train": -1.0, "cv_mean_score": -2.0, "cv_std_score": 0.0,
         "cv_R2_score": 0.5, "cv_mse_score": 2.0, "refit_coef": refit, "refit_intercept": 0.25,
         "n_iter": [3, 3, 3, 3], "converged": True, "refit_holdout_r2": 0.4,
         "refit_holdout_neg_mse": -1.5}
    d = sglm_ez.reduce_cv_result(r, drop, {"alpha": 0}, "Normal")
    assert d["cv_coefs"].shape == (len(keep), K) and np.array_equal(d["cv_coefs"], cvc[keep])
    assert np.array_equal(d["model"].coef_, refit[keep]) and d["model"].intercept_ == 0.25
    assert d["model"].model.n_features_in_ == len(keep)
    assert d["holdout_score"] == 0.4 and d["holdout_neg_mse_score"] == -1.5
    assert d["glm_kwargs"] == {"alpha": 0} and d["cv_R2_score"] == 0.5
    full = sglm_ez.reduce_cv_result(r, [], {"alpha": 0}, "Normal")
    assert np.array_equal(full["cv_coefs"], cvc) and full["model"].model.n_features_in_ == p


def test_drop_sets_argument_validation_needs_no_device():
    from sglm_hip import grid
    from sglm_hip.estimators import (ElasticNet, LinearRegression, NotYetImplementedError,
                                     PoissonRegressor)
    X = np.zeros((30, 5))
    y = np.zeros(30)
    cv = [(np.arange(20), np.arange(20, 30))]
    ols = LinearRegression().objective()

    def run(ds, objs=(ols,)):
        return grid.run_multi(X, y, [{"cv_idx": cv, "objectives": list(objs),
                                      "rolls": [0] * len(objs)}], drop_sets=ds)

    for bad, exc in ((3, TypeError), ("ab", TypeError), ([1, 2], TypeError), ([["a"]], TypeError),
                     ([[0.5]], TypeError), ([[5]], ValueError), ([[-1]], ValueError),
                     ([[1, 1]], ValueError), ([[0, 1, 2, 3, 4]], ValueError), ([], ValueError)):
        with pytest.raises(exc):
            run(bad)
    with pytest.raises(NotYetImplementedError, match="log-link"):
        run([[], [1]], [PoissonRegressor(alpha=1.0).objective()])
    with pytest.raises(NotYetImplementedError, match="coordinate-descent"):
        run([[], [1]], [ElasticNet(alpha=0.1, l1_ratio=0.5).objective()])
    assert grid.check_drop_sets([[], (3, 1), np.array([2])], 5) == [[], [1, 3], [2]]


def test_library_exports_the_drop_entry_points():
    from sglm_hip import _lib
    lib = _lib.load()
    for name in ("sglm_chol64_drop_kmax", "sglm_chol64_drop_work_bytes", "sglm_chol64_drop_prep",
                 "sglm_chol64_drop_solve_add"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    kmax = _lib.query("sglm_chol64_drop_kmax")
    assert kmax >= 64
    # W [P][kmax] and the 64 x 64 factor of T per pair, float64
    assert _lib.query("sglm_chol64_drop_work_bytes", 768, 3, 41) == 3 * (768 * 41 + 64 * 64) * 8
    assert _lib.query("sglm_chol64_drop_work_bytes", 768, 0, 41) == 0


def test_fitreq_and_stats_carry_the_drop_fields():
    from sglm_hip import engine
    r = engine.FitReq(engine.FAM_SQUARED, 0.0, 1.0, 0, 0)
    assert r.drop == -1
    s = engine.IrlsStats()
    assert s.drop_reduced == 0 and s.drop_excluded == 0
