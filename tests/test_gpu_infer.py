"""Inference end to end on the device (sglm_hip.inference) against the numpy
oracle of tests/infer_cases.py at the engine's own fitted coefficients: n = 4000, p = 126
(6 events x 21 lags), every IRLS family, the three covariance types, the batched call, the
drop-in surface and the refusals that need a design on the device.

Bars (the project's parity bars): relative error of se, scale, df and the group statistics
<= 1e-5 for Normal and <= 1e-4 for the other families; the full covariance is held to the same
bar on the correlation scale, |C - C_ref|_ij / sqrt(C_ref,ii C_ref,jj)."""
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest

import infer_cases as C

pytestmark = pytest.mark.gpu
BAR = {True: 1e-5, False: 1e-4}          # keyed by "the family is Normal"


def _glm(name, alpha=None, **kw):
    import sglm
    fam, power, a0, b0, phi = C.GPU_FAMILIES[name]
    alpha = a0 if alpha is None else alpha
    if name in ("normal", "ridge"):
        return sglm.GLM("Normal", alpha=alpha, l1_ratio=0)
    if name == "tweedie15":
        return sglm.GLM("Tweedie", power=1.5, alpha=alpha)
    if name == "nb2":
        return sglm.GLM("NB2", kappa=kw.get("kappa", power), alpha=alpha)
    return sglm.GLM({"poisson": "Poisson", "gamma": "Gamma", "binomial": "Binomial"}[name],
                    alpha=alpha)


@lru_cache(maxsize=None)
def fitted(name, alpha=None, resp=0, kappa=None):
    X, y, ids, beta = C.gpu_case(name, resp)
    glm = _glm(name, alpha, **({} if kappa is None else {"kappa": kappa}))
    glm.fit(X, y)
    return glm


def reference(name, glm, cov_type="model", scale=None, resp=0, groups=True):
    X, y, ids, _ = C.gpu_case(name, resp)
    fam, power = C.GPU_FAMILIES[name][:2]
    if fam == C.FAM_NB2:
        power = glm.model._kappa()
    obj = glm.model._objective()
    beta = np.r_[glm.coef_, glm.intercept_]
    return C.oracle(C.xt(X), y, fam, power, obj.lam(float(len(y))), beta, cov_type=cov_type,
                    scale=scale, groups=ids if groups else None)


def rel(got, ref):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def compare(label, r, o, bar, cov=True):
    p = len(r.coef)
    fig = dict(se=rel(np.r_[r.se, r.intercept_se], o["se"]), scale=rel(r.scale, o["scale"]),
               df=rel(r.df, o["df"]), stat=rel(r.group_stat, o["stat"]))
    if cov:
        sd = np.sqrt(np.diag(o["cov"]))
        fig["cov"] = float(np.max(np.abs(r.cov - o["cov"]) / np.outer(sd, sd)))
        assert r.cov.shape == (p + 1, p + 1) and np.array_equal(r.cov, r.cov.T)
    print(f"WORST infer {label}: " + " ".join(f"{k} {v:.3e}" for k, v in fig.items())
          + f"  (bar {bar:.0e})")
    assert r.n == o["n"] and np.array_equal(r.group_dof, o["dof"])
    assert max(fig.values()) <= bar, fig
    return fig


@pytest.mark.parametrize("name", list(C.GPU_FAMILIES))
def test_infer_families(engine, name):
    import scipy.special
    X, y, ids, _ = C.gpu_case(name)
    glm = fitted(name)
    coef, icpt = glm.coef_.copy(), glm.intercept_
    score = glm.model.score(X, y)
    r = glm.inference(X, y, groups=ids, return_cov=True)
    o = reference(name, glm)
    compare(name, r, o, BAR[C.GPU_FAMILIES[name][0] == C.FAM_SQUARED])
    assert np.array_equal(r.coef, coef) and r.intercept == icpt
    z = coef / r.se
    assert np.array_equal(r.z, z)
    assert np.allclose(r.pvalues, scipy.special.erfc(np.abs(z) / np.sqrt(2)), rtol=1e-14, atol=0)
    assert np.allclose(r.group_pvalue, scipy.special.gammaincc(r.group_dof / 2, r.group_stat / 2),
                       rtol=1e-14, atol=0)
    assert r.group_ids.tolist() == list(range(C.GPU_M))
    # the fitted model is as it was, bit for bit
    assert np.array_equal(glm.coef_, coef) and glm.intercept_ == icpt
    assert np.array_equal(glm.model.coef_, coef) and glm.model.score(X, y) == score


@pytest.mark.parametrize("name,cov_type,scale", [
    ("poisson", "bayes", None), ("poisson", "robust", None), ("poisson", "model", "pearson"),
    ("poisson", "model", 1.7), ("ridge", "bayes", None), ("ridge", "robust", None),
    ("gamma", "robust", None), ("nb2", "robust", None), ("binomial", "bayes", None)])
def test_infer_cov_types(engine, name, cov_type, scale):
    X, y, ids, _ = C.gpu_case(name)
    glm = fitted(name)
    r = glm.inference(X, y, groups=ids, cov_type=cov_type, scale=scale, return_cov=True)
    o = reference(name, glm, cov_type, scale)
    compare(f"{name} {cov_type} scale={scale}", r, o,
            BAR[C.GPU_FAMILIES[name][0] == C.FAM_SQUARED])


def test_infer_nb2_ml(engine):
    """kappa='ml': inference at the fitted kappa_, taken as known."""
    X, y, ids, _ = C.gpu_case("nb2")
    glm = fitted("nb2", kappa="ml")
    assert abs(glm.model.kappa_ - 0.5) < 0.15
    r = glm.inference(X, y, groups=ids, return_cov=True)
    compare("nb2 ml", r, reference("nb2", glm), BAR[False])


def test_infer_batch_equals_single_calls(engine):
    """Three alphas x two responses in one call: each entry against the oracle and against its
    own single call (the Grams of a batch may split their rows differently: f32 accumulation
    order, 6e-8 relative, times cond(A) ~ 40 -> 1e-5 between the two)."""
    from sglm_hip import inference
    X, _, ids, _ = C.gpu_case("poisson")
    models, ys, keys = [], [], []
    for resp in (0, 1):
        for alpha in (1e-3, 1e-2, 1e-1):
            models.append(fitted("poisson", alpha, resp))
            ys.append(C.gpu_case("poisson", resp)[1])
            keys.append((alpha, resp))
    rs = inference.infer(X, ys, models, groups=ids, return_cov=True)
    assert len(rs) == 6
    worst = 0.0
    for (alpha, resp), glm, yv, r in zip(keys, models, ys, rs):
        compare(f"batch alpha={alpha} resp={resp}", r,
                reference("poisson", glm, resp=resp), BAR[False])
        one = inference.infer(X, yv, glm, groups=ids)
        worst = max(worst, rel(r.se, one.se), rel(r.group_stat, one.group_stat),
                    rel(r.df, one.df))
    print(f"WORST batch vs single: {worst:.3e}")
    assert worst <= 1e-5
    # one shared response vector for several models
    two = inference.infer(X, ys[0], models[:3])
    assert rel(two[1].se, rs[1].se) <= 1e-5 and two[1].group_stat is None and two[1].cov is None


def test_event_wald_and_kernel_bands(engine):
    import sglm_ez
    X, y, ids, _ = C.gpu_case("poisson")
    glm = fitted("poisson")
    assert np.array_equal(sglm_ez.event_groups(X), ids)
    w = sglm_ez.event_wald(X, y, glm)
    assert list(w.index) == [f"ev{a}" for a in range(C.GPU_M)] and w.index.name == "event"
    assert list(w.columns) == ["dof", "wald", "pvalue"] and w["dof"].tolist() == [C.GPU_L] * C.GPU_M
    o = reference("poisson", glm)
    assert rel(w["wald"].values, o["stat"]) <= BAR[False]
    assert w.loc["ev0", "pvalue"] < 1e-8              # the strong kernel
    assert w.loc["ev1", "pvalue"] > 0.01              # the true zero kernel
    b = sglm_ez.kernel_bands(X, y, glm, level=0.95)
    assert list(b.index) == list(X.columns) and list(b.columns) == ["coef", "se", "lo", "hi"]
    assert rel(b["se"].values, o["se"][:-1]) <= BAR[False]
    assert np.allclose((b["hi"] - b["coef"]) / b["se"], 1.959963984540054, rtol=1e-12)
    assert np.allclose((b["coef"] - b["lo"]) / b["se"], 1.959963984540054, rtol=1e-12)
    rob = sglm_ez.event_wald(X, y, glm, cov_type="robust")
    assert rel(rob["wald"].values, reference("poisson", glm, "robust")["stat"]) <= BAR[False]
    # the estimator itself, without the GLM wrapper, and a plain array
    r = glm.model.inference(X.values, y)
    assert rel(r.se, o["se"][:-1]) <= BAR[False] and r.group_stat is None


def test_zero_column_and_over_cap_group(engine):
    """An all-zero column of an unpenalised fit: se NaN, its group loses a degree of freedom;
    a group above the kernel's cap: NaN with a warning."""
    import sglm
    X, y, ids, _ = C.gpu_case("poisson")
    Xz = X.copy()
    Xz.iloc[:, 30] = 0.0
    glm = sglm.GLM("Poisson", alpha=0)
    glm.fit(Xz, y)
    r = glm.inference(Xz, y, groups=ids)
    beta = np.r_[glm.coef_, glm.intercept_]
    o = C.oracle(C.xt(Xz), y, C.FAM_TWEEDIE, 1.0, 0.0, beta, groups=ids)
    assert np.isnan(r.se[30]) and np.isnan(r.z[30]) and np.isnan(o["se"][30])
    assert r.group_dof.tolist() == [21, 20, 21, 21, 21, 21] == o["dof"].tolist()
    keep = np.arange(126) != 30
    assert rel(r.se[keep], o["se"][:-1][keep]) <= BAR[False]
    assert rel(r.group_stat, o["stat"]) <= BAR[False] and rel(r.df, o["df"]) <= BAR[False]
    big = np.where(ids < 4, 0, ids)                   # 84 columns in one group
    with pytest.warns(UserWarning, match="more than 64 columns"):
        rb = fitted("poisson").inference(X, y, groups=big)
    assert np.isnan(rb.group_stat[0]) and np.isnan(rb.group_pvalue[0])
    assert np.all(np.isfinite(rb.group_stat[1:])) and rb.group_dof.tolist() == [84, 21, 21]


def test_device_side_refusals(engine):
    import sglm
    from sglm_hip import estimators as est
    X, y, ids, _ = C.gpu_case("poisson")
    Xs, ys = X.iloc[:600, :42], y[:600]
    yn = C.gpu_case("normal")[1][:600]
    # a mixed design: one continuous column
    Xm = Xs.copy()
    Xm.iloc[:, 3] = np.linspace(0.0, 1.0, 600) ** 2
    glm = sglm.GLM("Poisson", alpha=1e-3)
    glm.fit(Xm, ys)
    with pytest.raises(est.NotYetImplementedError, match="mixed|non-binary"):
        glm.inference(Xm, ys)
    # models fitted with selection penalties
    for model, word in ((sglm.GLM("Poisson", alpha=1e-3, l1_ratio=0.5), "'pn'"),
                        (sglm.GLM("Normal", alpha=1e-3, l1_ratio=0.5), "'cd'"),
                        (sglm.GLM("Normal", alpha=1e-3, l1_ratio=0.5, groups=ids[:42]), "'gcd'")):
        model.fit(Xs, yn if word != "'pn'" else ys)
        with pytest.raises(est.NotYetImplementedError, match=word):
            model.inference(Xs, ys)
    # a dependent column: the model is not identified
    Xd = Xs.copy()
    Xd.iloc[:, 7] = Xd.iloc[:, 5]
    glm = sglm.GLM("Poisson", alpha=0)
    glm.fit(Xd, ys)
    with pytest.raises(ValueError, match="not identified: 1 coordinate"):
        glm.inference(Xd, ys)
