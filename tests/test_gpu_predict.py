"""Pointwise bands of fitted traces end to end on the device (sglm_hip.inference.predict_bands,
DESIGN.md §31) on infer_cases.gpu_case (n = 4000, 6 events x 21 lags) at the engine's own
fitted coefficients: every IRLS family with 'model', Poisson and Normal with 'bayes', 'robust'
and 'cluster' (the trials of cluster_cases).

Bars.  The covariance tests hold |dC_jk| <= bar sd_j sd_k (bar 1e-5 Normal / Ridge, 1e-4
otherwise), hence |dv_i| <= bar (sum_{j in S_i} sd_j)^2 per row: asserted per row from the
oracle's own C, no flat constant (on this design (sum sd_j)^2 / v_i <= 27.4, so the implied
relative bar on eta_se is about 14 bar).  Against the same call's ``inference(return_cov=True)
.cov`` evaluated in longdouble the device result is held to the kernel's rounding bound
(predict_cases), which separates the row pass from C's accuracy; eta is held to the rounding
bound of X~ beta in float64.  Every test prints its worst figures."""
import warnings

import numpy as np
import pandas as pd
import pytest

import cluster_cases as K
import infer_cases as C
import predict_cases as PC
import test_gpu_cluster as TC
import test_gpu_infer as TI

pytestmark = pytest.mark.gpu
BAR = TI.BAR
CASES = [(name, "model") for name in C.GPU_FAMILIES] + \
    [(name, ct) for name in ("poisson", "normal") for ct in ("bayes", "robust", "cluster")]


def setup(name, cov_type):
    """(frame, y, column group ids, fitted glm, oracle, keywords of the covariance type)."""
    if cov_type == "cluster":
        X, y, ids, _, cid = K.gpu_case(name)
        glm = TC.fitted(name)
        return X, y, ids, glm, TC.reference(name, glm), dict(cov_type="cluster", clusters=cid)
    X, y, ids, _ = C.gpu_case(name)
    glm = TI.fitted(name)
    return X, y, ids, glm, TI.reference(name, glm, cov_type), dict(cov_type=cov_type)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def relmax(got, ref):
    return float(np.max(np.abs(np.asarray(got, float) - np.asarray(ref, float))
                        / np.abs(np.asarray(ref, float))))


@pytest.mark.parametrize("name,cov_type", CASES)
def test_predict_bands(engine, name, cov_type):
    X, y, ids, glm, o, kw = setup(name, cov_type)
    fam = C.GPU_FAMILIES[name][0]
    bar = BAR[fam == C.FAM_SQUARED]
    n, p = X.shape
    r = glm.predict_bands(X, y, groups=ids, **kw)
    own = glm.inference(X, y, return_cov=True, **kw).cov
    Xt = C.xt(X)
    beta = np.r_[glm.coef_, glm.intercept_]
    sd = np.sqrt(np.diag(o["cov"]))
    fig = {}
    # the trace: against the oracle's C under the covariance bar, against the engine's own C
    # and X~ beta under the rounding bounds
    eta_o, v_o, eb, _ = PC.traces_rows(Xt, beta, o["cov"])
    _, v_e, _, vb = PC.traces_rows(Xt, beta, own)
    v = PC.ld(r.eta_se) ** 2
    assert np.all(v_o > 0) and np.all(np.isfinite(r.eta_se)) and r.eta.shape == (n,)
    fig["v/bar"] = PC.ratio(v - v_o, bar * (Xt @ sd) ** 2)
    # (the result carries eta_se, not v: the 4 u v is the square root and its square)
    fig["v/own"] = PC.ratio(v - v_e, vb + 4 * PC.U53 * np.asarray(v_e, float))
    fig["eta"] = PC.ratio(PC.ld(r.eta) - eta_o, eb)
    rel = dict(eta_se=relmax(r.eta_se, np.sqrt(np.asarray(v_o, float))))
    # mean, mean_se, lo, hi: host arithmetic on (eta, eta_se)
    mean, mean_se, lo, hi = PC.bands(fam, r.eta, r.eta_se, 0.95)
    for got, want in ((r.mean, mean), (r.mean_se, mean_se), (r.lo, lo), (r.hi, hi)):
        assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert np.all(r.lo < r.mean) and np.all(r.mean < r.hi) and r.level == 0.95
    rel["mean_se"] = relmax(r.mean_se, PC.dmu_deta(fam, np.asarray(eta_o, float))
                            * np.sqrt(np.asarray(v_o, float)))
    # per event
    assert r.group_ids.tolist() == list(range(C.GPU_M)) and r.group_eta.shape == (C.GPU_M, n)
    gw = go = ge = gs = 0.0
    z = PC.zq(0.95)
    for g in range(C.GPU_M):
        cols = np.flatnonzero(ids == g)
        g_eta, gv_o, geb, _ = PC.traces_rows(Xt, beta, o["cov"], cols)
        _, gv_e, _, gvb = PC.traces_rows(Xt, beta, own, cols)
        gv = PC.ld(r.group_se[g]) ** 2
        gw = max(gw, PC.ratio(gv - gv_o, bar * (Xt[:, cols] @ sd[cols]) ** 2))
        go = max(go, PC.ratio(gv - gv_e, gvb + 4 * PC.U53 * np.asarray(gv_e, float)))
        ge = max(ge, PC.ratio(PC.ld(r.group_eta[g]) - g_eta, geb))
        has = Xt[:, cols].any(axis=1)
        assert np.all(bits(r.group_eta[g, ~has]) == 0) and np.all(bits(r.group_se[g, ~has]) == 0)
        gs = max(gs, relmax(r.group_se[g, has], np.sqrt(np.asarray(gv_o, float))[has]))
        # eta -+ z se may cancel: relative to the terms, not to the difference
        tol = 1e-12 * (np.abs(r.group_eta[g]) + z * r.group_se[g])
        assert np.all(np.abs(r.group_lo[g] - (r.group_eta[g] - z * r.group_se[g])) <= tol)
        assert np.all(np.abs(r.group_hi[g] - (r.group_eta[g] + z * r.group_se[g])) <= tol)
    fig.update({"gv/bar": gw, "gv/own": go, "geta": ge})
    rel["group_se"] = gs
    print(f"WORST predict {name} {cov_type}: " + " ".join(f"{k} {v:.3e}" for k, v in fig.items())
          + "  (ratios to their bounds)  rel: "
          + " ".join(f"{k} {v:.3e}" for k, v in rel.items()) + f"  (bar {bar:.0e})")
    assert max(fig.values()) <= 1.0, fig


def test_holdout_batch_and_levels(engine):
    from sglm_hip import inference
    X, y, ids, glm, o, kw = setup("poisson", "model")
    n = len(y)
    full = glm.predict_bands(X, y)
    # X_new of other rows, in another order: the oracle on those rows, and the bits of the same
    # rows of X (a row's result depends on its bits alone)
    pick = np.random.default_rng(41).permutation(n)[:700]
    Xn = X.iloc[pick]
    h = glm.predict_bands(X, y, X_new=Xn)
    assert h.eta.shape == (700,)
    assert np.array_equal(bits(h.eta), bits(full.eta[pick])) and np.array_equal(bits(h.eta_se), bits(full.eta_se[pick]))
    Xt = C.xt(Xn)
    beta = np.r_[glm.coef_, glm.intercept_]
    sd = np.sqrt(np.diag(o["cov"]))
    eta_o, v_o, eb, _ = PC.traces_rows(Xt, beta, o["cov"])
    w = PC.ratio(PC.ld(h.eta_se) ** 2 - v_o, BAR[False] * (Xt @ sd) ** 2)
    print(f"WORST predict holdout: v/bar {w:.3e} eta {PC.ratio(PC.ld(h.eta) - eta_o, eb):.3e}")
    assert w <= 1.0 and PC.ratio(PC.ld(h.eta) - eta_o, eb) <= 1.0
    hr = glm.predict_bands(X, y, X_new=Xn, rows=[699, 0, 0])
    assert np.array_equal(bits(hr.eta_se), bits(h.eta_se[[699, 0, 0]]))
    # rows of X itself
    rr = glm.predict_bands(X, y, rows=[5, 5, 3, n - 1], groups=ids)
    fg = glm.predict_bands(X, y, groups=ids)
    assert np.array_equal(bits(rr.eta_se), bits(full.eta_se[[5, 5, 3, n - 1]]))
    assert np.array_equal(bits(rr.group_se), bits(fg.group_se[:, [5, 5, 3, n - 1]]))
    assert np.array_equal(bits(fg.eta_se), bits(full.eta_se))
    # nested levels
    half = glm.predict_bands(X, y, level=0.5)
    assert np.all(full.lo < half.lo) and np.all(half.lo < half.mean) and np.all(half.hi < full.hi)
    assert np.array_equal(bits(half.eta_se), bits(full.eta_se)) and half.level == 0.5
    # three Ridge alphas in one call: the bits of the single calls
    Xr, yr, _, _ = C.gpu_case("ridge")
    models = [TI.fitted("ridge", a) for a in (5.0, 25.0, 125.0)]
    rs = inference.predict_bands(Xr, yr, models, groups=ids)
    assert len(rs) == 3
    for m, b in zip(models, rs):
        one = m.predict_bands(Xr, yr, groups=ids)
        for key in ("eta", "eta_se", "mean", "mean_se", "lo", "hi", "group_eta", "group_se"):
            assert np.array_equal(bits(getattr(one, key)), bits(getattr(b, key))), key
    assert not np.array_equal(rs[0].eta_se, rs[2].eta_se)


def test_drop_in_frames(engine):
    import sglm_ez
    X, y, ids, glm, o, kw = setup("poisson", "model")
    n = len(y)
    Xi = X.set_index(pd.Index(np.arange(n) * 2 + 7, name="t"))
    fb = sglm_ez.fitted_bands(Xi, y, glm)
    assert fb.shape == (n, 6) and list(fb.columns) == ["mean", "mean_se", "lo", "hi", "eta", "eta_se"]
    assert fb.index.equals(Xi.index)
    r = glm.predict_bands(X, y, groups=ids)
    assert np.array_equal(bits(fb["eta_se"].to_numpy()), bits(r.eta_se))
    ec = sglm_ez.event_contributions(Xi, y, glm)
    events = [f"ev{a}" for a in range(C.GPU_M)]
    assert ec.shape == (n, 4 * C.GPU_M) and ec.index.equals(Xi.index)
    assert ec.columns.names == ["event", None]
    assert list(ec.columns) == [(e, k) for e in events for k in ("eta", "se", "lo", "hi")]
    assert np.array_equal(bits(ec[("ev3", "se")].to_numpy()), bits(r.group_se[3]))
    # the events' predictors and the intercept add up to the trace: both sides are float64 sums
    # of the same |beta_j| terms, each within the eta rounding bound (m + 2) u sum |terms|
    parts = ec.xs("eta", axis=1, level=1).to_numpy()
    total = PC.ld(parts).sum(axis=1) + PC.LD(glm.intercept_)
    Xt = C.xt(X)
    terms = Xt @ np.abs(np.r_[glm.coef_, glm.intercept_])
    m = Xt.sum(axis=1)
    w = PC.ratio(total - PC.ld(fb["eta"].to_numpy()), 2 * (m + 2) * PC.U53 * terms)
    print(f"WORST predict contributions sum: {w:.3e} (of 2 (m + 2) u sum |terms|)")
    assert w <= 1.0
    # rows
    part = sglm_ez.event_contributions(Xi, y, glm, rows=slice(100, 300))
    assert part.index.equals(Xi.index[100:300]) and part.shape == (200, 4 * C.GPU_M)
    assert np.array_equal(bits(part.to_numpy()), bits(ec.iloc[100:300].to_numpy()))
    fr = sglm_ez.fitted_bands(Xi, y, glm, rows=[9, 2], level=0.5)
    assert fr.index.tolist() == [25, 11] and np.array_equal(bits(fr["eta"].to_numpy()), bits(r.eta[[9, 2]]))
    # holdout frame: its own index
    fh = sglm_ez.fitted_bands(Xi, y, glm, X_new=Xi.iloc[50:80])
    assert fh.index.equals(Xi.index[50:80])
    assert np.array_equal(bits(fh["eta_se"].to_numpy()), bits(r.eta_se[50:80]))


def test_inference_is_untouched_and_large_groups_warn(engine):
    X, y, ids, glm, o, kw = setup("gamma", "model")
    before = glm.inference(X, y, groups=ids, return_cov=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        glm.predict_bands(X, y, groups=ids)
    with pytest.warns(UserWarning, match="more than 64 columns") as rec:
        big = glm.predict_bands(X, y, groups=np.r_[np.zeros(65, int), np.ones(X.shape[1] - 65, int)])
    assert sum("more than 64 columns" in str(w.message) for w in rec) == 1
    assert np.all(np.isnan(big.group_eta[0])) and np.all(np.isnan(big.group_se[0]))
    assert np.all(np.isfinite(big.group_se[1])) and np.all(np.isfinite(big.eta_se))
    after = glm.inference(X, y, groups=ids, return_cov=True)
    for key in ("se", "z", "pvalues", "group_stat", "group_pvalue", "cov"):
        assert np.array_equal(bits(getattr(before, key)), bits(getattr(after, key))), key
    assert before.scale == after.scale and before.df == after.df


def test_design_refusals_on_the_device(engine):
    from sglm_hip import estimators as est
    X, y, ids, glm, o, kw = setup("normal", "model")
    Xc = np.asarray(X, dtype=np.float64).copy()
    Xc[:, 3] = np.linspace(0, 1, len(y))                    # a continuous column: a mixed design
    with pytest.raises(est.NotYetImplementedError, match="mixed|non-binary"):
        glm.predict_bands(Xc, y)
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        glm.predict_bands(X, y, X_new=Xc[:10])
