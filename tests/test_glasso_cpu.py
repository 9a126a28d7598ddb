"""Group lasso without a device: the numpy oracle against its own optimality conditions and
against the elastic-net oracle, the margin condition that makes the zero patterns of the GPU
tests well determined, the estimator / GLM dispatch and validation, the C ABI names and
``sglm_ez.event_groups``."""
import numpy as np
import pandas as pd
import pytest

import glasso_cases as C

GRID_CASES = ("6x5", "8x12")
ALL = [(name, a, rho) for name in C.CASES for rho in C.RHOS for a in C.ALPHAS]


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_meets_its_kkt_conditions(name):
    Q, q, xm, ym, n, goff, gcols = C.gram(name)
    for rho in C.RHOS:
        for a in C.ALPHAS + (C.ALPHA_ALL_ZERO,):
            w, sw = C.solution(name, a, rho)
            v = C.kkt(Q, q, a * rho * n, a * (1 - rho) * n, goff, gcols, w)
            assert sw < 200000 and v <= 1e-10, (name, a, rho, sw, v)
    for gname in GRID_CASES:
        for fi in (True, False):
            for cell in C.grid_oracle(gname, fi)[1].values():
                assert max(cell["kkt"]) <= 1e-10, (gname, fi, cell["kkt"])


def test_oracle_patterns_cover_the_regimes():
    """Mixed zero / non-zero groups, all groups in, and all groups out occur in the cases."""
    for name in ("6x5", "8x12"):
        Q, q, xm, ym, n, goff, gcols = C.gram(name)
        z = {a: C.zero_groups(C.solution(name, a, 1.0)[0], goff, gcols) for a in C.ALPHAS}
        assert not z[0.002].any()
        assert z[0.01].any() and not z[0.01].all()
        w, sw = C.solution(name, C.ALPHA_ALL_ZERO, 1.0)
        assert sw == 1 and np.all(w == 0.0)


@pytest.mark.parametrize("name", ["6x5", "8x12"])
def test_singleton_groups_are_the_elastic_net(name):
    from oracle import glm_ref
    X, y, ids = C.case(name)
    for rho in C.RHOS:
        for a in C.ALPHAS:
            w, b, _ = C.fit(X, y, a, rho, np.arange(X.shape[1]))
            w_ref, b_ref = glm_ref.fit_enet_cd(X, y, a, rho, tol=1e-14)
            scale = max(np.max(np.abs(w_ref)), 1e-300)
            assert np.max(np.abs(w - w_ref)) <= 1e-10 * scale, (name, a, rho)
            assert abs(b - b_ref) <= 1e-10 * max(1.0, abs(b_ref))
            assert np.array_equal(w == 0.0, w_ref == 0.0)


def test_margin_condition_of_every_case():
    """Zero groups sit inside the threshold by 1e-3 and non-zero groups are not vanishing: the
    zero pattern of every fit the GPU tests compare is determined far above rounding."""
    for name, a, rho in ALL:
        Q, q, xm, ym, n, goff, gcols = C.gram(name)
        w, _ = C.solution(name, a, rho)
        zero, small = C.margins(Q, q, a * rho * n, a * (1 - rho) * n, goff, gcols, w)
        assert zero <= 1 - 1e-3 and small >= 1e-3, (name, a, rho, zero, small)
    for gname in GRID_CASES:
        for fi in (True, False):
            for key, cell in C.grid_oracle(gname, fi)[1].items():
                for zero, small in cell["marg"]:
                    assert zero <= 1 - 1e-3 and small >= 1e-3, (gname, fi, key, zero, small)
    for key, (_, _, _, (zero, small)) in C.path_oracle()[1].items():
        assert zero <= 1 - 1e-3 and small >= 1e-3, (key, zero, small)
    Qs, fits, goff, gcols = C.many_fits()
    for f, (qi, q, ls, l2) in enumerate(fits):
        w, _ = C.gmd(Qs[qi], q, ls, l2, goff, gcols)
        assert C.kkt(Qs[qi], q, ls, l2, goff, gcols, w) <= 1e-10
        zero, small = C.margins(Qs[qi], q, ls, l2, goff, gcols, w)
        assert zero <= 1 - 1e-3 and small >= 1e-3, (f, zero, small)


def test_estimator_objective_and_validation():
    from sglm_hip import engine as E
    from sglm_hip import estimators as est
    g = [0, 0, 7, 7, 3]
    m = est.GroupLasso(0.1, groups=g, l1_ratio=0.5, fit_intercept=False, max_iter=50)
    o = m.objective()
    assert (o.kind, o.family, o.alpha, o.l1_ratio, o.fit_intercept, o.max_iter) == \
        ("gcd", E.FAM_SQUARED, 0.1, 0.5, False, 50)
    assert o.groups == (0, 0, 7, 7, 3) and hash(o.groups) is not None
    assert est.GroupLasso(groups=g).get_params() == {
        "alpha": 1.0, "groups": g, "l1_ratio": 1.0, "fit_intercept": True, "max_iter": 1000,
        "tol": 1e-4, "warm_start": False}
    assert m.set_params(alpha=0.3).alpha == 0.3
    with pytest.raises(ValueError):
        m.set_params(nope=1)
    with pytest.raises(TypeError):
        est.GroupLasso(0.1)                                   # groups is required
    o0 = est.GroupLasso(0.0, groups=g).objective()            # alpha == 0: LinearRegression
    assert o0 == est.LinearRegression().objective() and o0.kind == "irls"
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            est.GroupLasso(0.1, groups=g, l1_ratio=bad).objective()
    with pytest.raises(ValueError):
        est.GroupLasso(-1.0, groups=g).objective()
    with pytest.raises(ValueError):                           # length checked before any device
        est.GroupLasso(0.1, groups=g).fit(np.ones((8, 4)), np.ones(8))
    # the existing objectives carry no groups
    assert est.ElasticNet(0.1).objective().groups is None
    assert est.ElasticNet(0.1).objective().kind == "cd"


def test_glm_dispatch_with_groups():
    import sglm
    from sglm_hip import estimators as est
    g = np.array([0, 0, 1, 1])
    for name in ("Normal", "Gaussian"):
        glm = sglm.GLM(name, alpha=0.1, l1_ratio=0.5, groups=g)
        assert glm.Base is est.GroupLasso and glm.model.objective().kind == "gcd"
        assert sglm.GLM(name, alpha=0.1, l1_ratio=1, groups=g).Base is est.GroupLasso
        assert sglm.GLM(name, alpha=0.1, groups=g).Base is est.GroupLasso
        lin = sglm.GLM(name, alpha=0, l1_ratio=0.5, groups=g)
        assert lin.Base is est.LinearRegression and "groups" not in lin.kwargs
        rdg = sglm.GLM(name, alpha=0.1, l1_ratio=0, groups=g)
        assert rdg.Base is est.Ridge and "groups" not in rdg.kwargs
    for name, kw in (("Poisson", {}), ("Binomial", {}), ("Gamma", {}), ("Tweedie", {"power": 1.5})):
        with pytest.raises(est.NotYetImplementedError):
            sglm.GLM(name, alpha=0.1, groups=g, **kw)
    # without groups nothing changes
    assert sglm.GLM("Normal", alpha=0.1, l1_ratio=0.5).Base is est.ElasticNet
    assert sglm.GLM("Normal", alpha=0.1, l1_ratio=1).Base is est.Lasso
    assert sglm.GLM("Normal", alpha=0.1, l1_ratio=0.5, groups=None).Base is est.ElasticNet
    assert sglm.GLM("Poisson", alpha=0.1).Base is est.TweedieRegressor


def test_grid_refuses_drop_sets_on_group_objectives():
    from sglm_hip import estimators as est
    from sglm_hip import grid
    obj = est.GroupLasso(0.1, groups=[0, 0, 1, 1]).objective()
    with pytest.raises(est.NotYetImplementedError, match="GroupLasso"):
        grid.check_drop_sets([[], [0]], 4, [{"objectives": [obj]}])
    assert grid.check_drop_sets([[]], 4, [{"objectives": [obj]}]) == [[]]


def test_group_csr():
    from sglm_hip import glasso
    goff, gcols = glasso.group_csr([5, 2, 5, 9, 2, 5], 6)
    assert goff.tolist() == [0, 2, 5, 6] and gcols.tolist() == [1, 4, 0, 2, 5, 3]
    assert goff.dtype == np.int32 and gcols.dtype == np.int32
    ref = C.csr([5, 2, 5, 9, 2, 5])
    assert np.array_equal(goff, ref[0]) and np.array_equal(gcols, ref[1])
    with pytest.raises(ValueError):
        glasso.group_csr([0, 1], 3)
    with pytest.raises(TypeError):
        glasso.group_csr([0.5, 1.0], 2)


def test_exports():
    from sglm_hip import _lib
    lib = _lib.load()
    for name in ("sglm_group_bound", "sglm_group_cd_shared", "sglm_group_cd_fits_per_wg"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.sglm_group_cd_fits_per_wg(30) >= 2
    assert lib.sglm_group_cd_fits_per_wg(4096) >= 1


def test_event_groups_by_name_pattern():
    import sglm_ez
    cols = ["a", "a_1", "a_-1", "ab", "ab_2", "t", "z_3"]
    df = pd.DataFrame(np.zeros((2, len(cols))), columns=cols)
    g = sglm_ez.event_groups(df)
    assert g.tolist() == [0, 0, 0, 1, 1, 2, 3]            # 'a' does not capture 'ab'; z_3 alone
    for name in ("a", "ab"):                              # left_out_columns' rule
        cols_of = sglm_ez.left_out_columns(df, [name])
        assert len(set(g[cols_of])) == 1
        assert np.flatnonzero(g == g[cols_of[0]]).tolist() == cols_of
