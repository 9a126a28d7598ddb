"""Inference without a device: the numpy oracle of tests/infer_cases.py against closed forms,
finite differences and Monte-Carlo means; every refusal that needs no device; the C ABI names."""
import os
import re
import types

import numpy as np
import pytest
import scipy.stats

import infer_cases as C
from conftest import ROOT


# ------------------------------------------------------------------------------ oracle self-checks
def test_ols_and_ridge_closed_forms():
    Xt, y, ids, beta = C.small_case(C.FAM_SQUARED, 0.0)
    n, P = Xt.shape
    G = Xt.T @ Xt
    bh = np.linalg.solve(G, Xt.T @ y)
    o = C.oracle(Xt, y, C.FAM_SQUARED, 0.0, 0.0, bh)
    s2 = np.sum((y - Xt @ bh) ** 2) / (n - P)
    assert abs(o["df"] - P) < 1e-9 and abs(o["scale"] - s2) <= 1e-12 * s2
    assert np.max(np.abs(o["cov"] - s2 * np.linalg.inv(G))) <= 1e-11 * np.max(np.abs(o["cov"]))
    lam = 7.5
    D = np.diag(np.r_[np.ones(P - 1), 0.0])
    Ai = np.linalg.inv(G + lam * D)
    br = Ai @ Xt.T @ y
    o = C.oracle(Xt, y, C.FAM_SQUARED, 0.0, lam, br)
    df = np.trace(Ai @ G)
    s2 = np.sum((y - Xt @ br) ** 2) / (n - df)
    assert abs(o["df"] - df) <= 1e-10 * df and abs(o["scale"] - s2) <= 1e-10 * s2
    assert np.max(np.abs(o["cov"] - s2 * Ai @ G @ Ai)) <= 1e-10 * np.max(np.abs(o["cov"]))
    ob = C.oracle(Xt, y, C.FAM_SQUARED, 0.0, lam, br, cov_type="bayes")
    assert np.max(np.abs(ob["cov"] - s2 * Ai)) <= 1e-10 * np.max(np.abs(ob["cov"]))
    assert np.all(np.diag(ob["cov"])[:-1] > np.diag(o["cov"])[:-1])     # A^-1 > A^-1 J A^-1


@pytest.mark.parametrize("fam,power", [(C.FAM_TWEEDIE, 1.0), (C.FAM_BINOMIAL, 0.0)])
def test_canonical_links_information_is_the_hessian(fam, power):
    """J equals a central-difference Hessian of the summed loss (evaluated in longdouble)."""
    Xt, y, ids, beta = C.small_case(fam, power)
    P = Xt.shape[1]
    J = C.oracle(Xt, y, fam, power, 0.0, beta)["J"]
    Xl, yl, h = C.ld(Xt), C.ld(y), C.LD(1e-4)

    def f(b):
        return np.sum(C.loss(fam, power, yl, Xl @ b))
    H = np.zeros((P, P))
    for i in range(P):
        for j in range(i, P):
            ei, ej = np.zeros(P, C.LD), np.zeros(P, C.LD)
            ei[i], ej[j] = h, h
            b = C.ld(beta)
            H[i, j] = H[j, i] = float((f(b + ei + ej) - f(b + ei - ej) - f(b - ei + ej)
                                       + f(b - ei - ej)) / (4 * h * h))
    assert np.max(np.abs(H - J)) <= 1e-6 * np.max(np.abs(J))


@pytest.mark.parametrize("fam,power", [(C.FAM_NB2, 0.5), (C.FAM_TWEEDIE, 2.0)])
def test_expected_information_is_the_mean_observed_hessian(fam, power):
    """Non-canonical links: J is the mean over responses drawn from the model of the observed
    Hessian X~^T diag(loss'') X~ within five Monte-Carlo standard errors entrywise -- and one
    draw's observed Hessian is far outside that."""
    Xt, y, ids, beta = C.small_case(fam, power)
    eta = Xt @ beta
    J = C.oracle(Xt, y, fam, power, 0.0, beta)["J"]
    rng = np.random.default_rng(91)
    R = 400
    Hs = np.zeros((R,) + J.shape)
    for r in range(R):
        yr = C.draw(rng, fam, power, eta, 0.6)
        Hs[r] = Xt.T @ (C.observed_weight(fam, power, yr, eta)[:, None] * Xt)
    mean, se = Hs.mean(axis=0), Hs.std(axis=0, ddof=1) / np.sqrt(R)
    assert np.all(se > 0)
    assert np.max(np.abs(mean - J) / se) <= 5.0
    assert np.max(np.abs(Hs[0] - J) / se) > 20.0


@pytest.mark.parametrize("fam,power,phi", [(C.FAM_TWEEDIE, 1.0, 1.0), (C.FAM_NB2, 0.5, 1.0),
                                           (C.FAM_TWEEDIE, 2.0, 0.6), (C.FAM_BINOMIAL, 0.0, 1.0)])
def test_robust_is_model_at_the_expected_scores(fam, power, phi):
    """E s^2 = phi v, so the sandwich with s^2 replaced by its expectation is phi A^-1 J A^-1."""
    Xt, y, ids, beta = C.small_case(fam, power)
    v = C.mean_weight_var(fam, power, Xt @ beta)[1]
    lam = 3.0
    rob = C.oracle(Xt, y, fam, power, lam, beta, cov_type="robust", s2=phi * v)
    mod = C.oracle(Xt, y, fam, power, lam, beta, cov_type="model", scale=phi)
    assert np.max(np.abs(rob["cov"] - mod["cov"])) <= 1e-12 * np.max(np.abs(mod["cov"]))
    emp = C.oracle(Xt, y, fam, power, lam, beta, cov_type="robust")
    assert np.max(np.abs(emp["cov"] - mod["cov"])) > 1e-3 * np.max(np.abs(mod["cov"]))


def test_wald_pvalues_match_chi2():
    import scipy.special
    Xt, y, ids, beta = C.small_case(C.FAM_TWEEDIE, 1.0)
    o = C.oracle(Xt, y, C.FAM_TWEEDIE, 1.0, 0.0, beta, groups=ids)
    assert o["dof"].tolist() == [3, 3]
    pv = scipy.special.gammaincc(o["dof"] / 2.0, o["stat"] / 2.0)
    assert np.allclose(pv, scipy.stats.chi2.sf(o["stat"], o["dof"]), rtol=1e-12, atol=0)
    z = beta[:-1] / o["se"][:-1]
    assert np.allclose(scipy.special.erfc(np.abs(z) / np.sqrt(2)), 2 * scipy.stats.norm.sf(np.abs(z)),
                       rtol=1e-12, atol=0)
    # a group of one column: the Wald statistic is z^2
    o1 = C.oracle(Xt, y, C.FAM_TWEEDIE, 1.0, 0.0, beta, groups=np.arange(6))
    assert np.allclose(o1["stat"], z ** 2, rtol=1e-12)


def test_zero_column_leaves_its_group():
    Xt, y, ids, beta = C.small_case(C.FAM_TWEEDIE, 1.0)
    Xz = Xt.copy()
    Xz[:, 1] = 0.0
    o = C.oracle(Xz, y, C.FAM_TWEEDIE, 1.0, 0.0, beta, groups=ids)
    assert o["dof"].tolist() == [2, 3] and np.isnan(o["se"][1]) and o["state"][1] == C.ZERO
    assert abs(o["df"] - 6) < 1e-9


@pytest.mark.parametrize("name", list(C.GPU_FAMILIES))
def test_recorded_condition_numbers(name):
    X, y, ids, beta = C.gpu_case(name)
    fam, power = C.GPU_FAMILIES[name][:2]
    o = C.oracle(C.xt(X), y, fam, power, C.lam_of(name, len(y)), beta)
    assert 0.5 <= o["cond"] / C.COND_A[name] <= 2.0 and o["cond"] < 1e4


def test_bounds_of_the_kernel_oracles_are_small():
    """The float64 bounds the GPU kernel tests hold the kernels to are tight ones: relative to
    the reference they stay below 1e-10 on the cases the tests use."""
    import chol64_cases as cc
    rng = np.random.default_rng(5)
    U, state, _ = cc.host_factor(rng, 128, excl=(0,), zero=(64,))
    ref, bound = C.inverse_bound(U, state)
    K = np.flatnonzero(state == 0)
    assert np.max(bound[np.ix_(K, K)]) <= 1e-10 * np.max(np.abs(ref))
    assert np.all(ref[0] == 0) and np.all(ref[:, 64] == 0)


# ------------------------------------------------------------------------------ refusals
def _fitted(est, p=5):
    est._set_fitted(np.arange(p, dtype=np.float64) / 7, 0.25, 3)
    return est


def test_refusals_without_a_device():
    from sglm_hip import estimators as est
    from sglm_hip import inference as inf
    X, y = np.zeros((8, 5)), np.zeros(8)
    for model, word in ((est.ElasticNet(0.1), "'cd'"), (est.Lasso(0.1), "'cd'"),
                        (est.GroupLasso(0.1, groups=[0, 0, 1, 1, 2]), "'gcd'"),
                        (est.PoissonRegressor(alpha=0.1, l1_ratio=0.5), "'pn'")):
        with pytest.raises(est.NotYetImplementedError, match=word):
            _fitted(model).inference(X, y)
        with pytest.raises(est.NotYetImplementedError, match=word):
            inf.infer(X, y, [_fitted(est.Ridge(1.0)), model])
    with pytest.raises(est.NotYetImplementedError, match="4095"):
        _fitted(est.Ridge(1.0), p=5000).inference(np.zeros((8, 5000)), y)
    for model in (est.Ridge(1.0), est.PoissonRegressor(), est.BinomialRegressor(),
                  est.NegativeBinomialRegressor(kappa="ml")):
        with pytest.raises(AttributeError, match="not fitted"):
            model.inference(X, y)
    with pytest.raises(ValueError, match="cov_type"):
        _fitted(est.Ridge(1.0)).inference(X, y, cov_type="hc3")
    for bad in ("ml", -1.0, 0.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            _fitted(est.Ridge(1.0)).inference(X, y, scale=bad)
    # the GLM wrapper reaches the same checks
    import sglm
    glm = sglm.GLM("Normal", alpha=0.1, l1_ratio=0.5)
    glm._set_fitted(np.zeros(5), 0.0)
    with pytest.raises(est.NotYetImplementedError, match="'cd'"):
        glm.inference(X, y)
    with pytest.raises(AttributeError, match="not fitted"):
        sglm.GLM("Poisson", alpha=0.1).inference(X, y)


def test_design_refusals():
    from sglm_hip import estimators as est
    from sglm_hip import inference as inf
    ok = dict(slab=None, cont=None, xbits=object(), P=256, p=100)
    inf.check_design(types.SimpleNamespace(**ok))
    for change, word in ((dict(slab=(0, 10, 20)), "row-sharded"), (dict(cont=object()), "mixed"),
                         (dict(xbits=None), "non-binary"), (dict(P=4352, p=4200), "4095")):
        with pytest.raises(est.NotYetImplementedError, match=word):
            inf.check_design(types.SimpleNamespace(**{**ok, **change}))


def test_group_lists_and_surface():
    from sglm_hip import inference as inf
    ids, goff, gcols, sizes = inf.group_lists([5, 2, 5, 9, 2, 5], 6)
    ref = C.csr([5, 2, 5, 9, 2, 5])
    assert ids.tolist() == [2, 5, 9] and sizes.tolist() == [2, 3, 1]
    assert np.array_equal(goff, ref[1]) and np.array_equal(gcols, ref[2])
    import sglm
    import sglm_ez
    from sglm_hip import estimators as est
    assert callable(sglm_ez.event_wald) and callable(sglm_ez.kernel_bands)
    assert callable(sglm.GLM.inference) and callable(est._EngineRegressor.inference)
    fields = [f.name for f in inf.Inference.__dataclass_fields__.values()]
    assert fields == ["coef", "intercept", "se", "intercept_se", "z", "pvalues", "scale", "df", "n",
                      "group_ids", "group_dof", "group_stat", "group_pvalue", "cov"]


def test_exports():
    from sglm_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sglm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sglm_infer_rows", "sglm_infer_rows_work_bytes", "sglm_chol64_inverse",
                 "sglm_chol64_inverse_work_bytes", "sglm_cov_groups", "sglm_cov_groups_kmax"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    kmax = lib.sglm_cov_groups_kmax()
    assert kmax >= 64 and kmax >= 41
    assert lib.sglm_chol64_inverse_work_bytes(192, 3) == 3 * 192 * 192 * 8
    assert lib.sglm_infer_rows_work_bytes(2, 2048) > 0
