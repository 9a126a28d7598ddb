"""Cluster-robust inference end to end on the device (sglm_hip.inference, cov_type='cluster';
DESIGN.md §30) against the longdouble oracle of tests/cluster_cases.py at the engine's own fitted
coefficients: n = 4000, p = 126, 97 trials of 20-60 rows with a per-trial random effect, every
IRLS family.

Bars: those of tests/test_gpu_infer.py (relative error of se and the group statistics, and the
covariance on the correlation scale: 1e-5 Normal / Ridge, 1e-4 the other families).  The meat is
float64 from the f32 predictor, whose effect on these errors is <= 3e-8 (CPU, every family), so
what the bars hold is the f32-accumulated Fisher Gram in A, as for the other covariance types.

Two comparisons are bitwise or near it, and are made where the bread is bitwise too: a Normal /
Ridge fit's Gram is the exact integer one, the same whatever the row order or the batch, so the
row-permuted call differs from the sorted one only by the float64 summation order of the meat
(1e-12), and the batched call equals its single calls bit for bit.  (A log- or logit-link Gram is
accumulated in f32 in an order that depends on both: 6e-8 relative, times cond(A) -- see
test_gpu_infer.test_infer_batch_equals_single_calls -- which is no property of the clustering.)"""
import warnings
from functools import lru_cache

import numpy as np
import pytest

import cluster_cases as K
import infer_cases as C
import test_gpu_infer as TI

pytestmark = pytest.mark.gpu
BAR = TI.BAR
rel = TI.rel
G = K.GPU_G                              # trials of the cases (97)


@lru_cache(maxsize=None)
def fitted(name, alpha=None):
    X, y, gids, beta, cid = K.gpu_case(name)
    glm = TI._glm(name, alpha)
    glm.fit(X, y)
    return glm


def reference(name, glm, clusters=None, correction=True):
    X, y, gids, _, cid = K.gpu_case(name)
    fam, power = C.GPU_FAMILIES[name][:2]
    obj = glm.model._objective()
    beta = np.r_[glm.coef_, glm.intercept_]
    return K.oracle(C.xt(X), y, fam, power, obj.lam(float(len(y))), beta,
                    cid if clusters is None else clusters, correction=correction, groups=gids)


def compare(label, r, o, bar):
    sd = np.sqrt(np.diag(o["cov"]))
    fig = dict(se=rel(np.r_[r.se, r.intercept_se], o["se"]), stat=rel(r.group_stat, o["stat"]),
               cov=float(np.max(np.abs(r.cov - o["cov"]) / np.outer(sd, sd))))
    print(f"WORST cluster {label}: " + " ".join(f"{k} {v:.3e}" for k, v in fig.items())
          + f"  (bar {bar:.0e})")
    assert r.n == o["n"] and np.array_equal(r.group_dof, o["dof"]) and r.n_clusters == o["G"]
    assert np.array_equal(r.cov, r.cov.T)
    assert max(fig.values()) <= bar, fig
    return fig


@pytest.mark.parametrize("name", list(C.GPU_FAMILIES))
def test_cluster_families(engine, name):
    import scipy.special
    X, y, gids, _, cid = K.gpu_case(name)
    glm = fitted(name)
    coef = glm.coef_.copy()
    r = glm.inference(X, y, cov_type="cluster", clusters=cid, groups=gids, return_cov=True)
    o = reference(name, glm)
    compare(name, r, o, BAR[C.GPU_FAMILIES[name][0] == C.FAM_SQUARED])
    assert r.n_clusters == G and np.array_equal(glm.coef_, coef)
    assert np.array_equal(r.z, coef / r.se)
    assert np.allclose(r.group_pvalue, scipy.special.gammaincc(r.group_dof / 2, r.group_stat / 2),
                       rtol=1e-14, atol=0)
    # not HC0 (ratio 1 if it were; >= 1.3 at the generating coefficients, test_cluster_cpu)
    hc0 = glm.inference(X, y, cov_type="robust")
    assert hc0.n_clusters is None and r.intercept_se >= 1.1 * hc0.intercept_se


def test_correction_is_exactly_kappa(engine):
    from sglm_hip import inference
    X, y, gids, _, cid = K.gpu_case("poisson")
    glm = fitted("poisson")
    r = glm.inference(X, y, cov_type="cluster", clusters=cid, groups=gids, return_cov=True)
    r0 = glm.inference(X, y, cov_type="cluster", clusters=cid, groups=gids, return_cov=True,
                       cluster_correction=False)
    kap = inference.cluster_kappa(G, 4000.0, 127)
    assert kap == pytest.approx(float(K.kappa(G, 4000, 127)), rel=1e-15)
    assert np.array_equal(r.cov, r0.cov * kap)
    assert np.array_equal(np.r_[r.se, r.intercept_se], np.sqrt(np.diag(r0.cov) * kap))
    assert np.array_equal(r.group_stat, r0.group_stat / kap)
    compare("poisson CR0", r0, reference("poisson", glm, correction=False), BAR[False])


def test_rows_in_any_order(engine):
    """Fit once; the rows of X, y and the ids permuted together give the clustered covariance of
    the sorted rows within 1e-12 (Normal: see the module docstring), through R = n single-row-ish
    runs merged per cluster instead of G contiguous ones."""
    X, y, gids, _, cid = K.gpu_case("normal")
    glm = fitted("normal")
    a = glm.inference(X, y, cov_type="cluster", clusters=cid, groups=gids, return_cov=True)
    perm = np.random.default_rng(8).permutation(len(y))
    Xp = X.iloc[perm].reset_index(drop=True)
    from sglm_hip import inference
    runs = inference.cluster_runs(cid[perm], len(y))
    assert runs.G == G and runs.R > 3500 and runs.coff is not None
    b = glm.inference(Xp, y[perm], cov_type="cluster", clusters=cid[perm], groups=gids,
                      return_cov=True)
    sd = np.sqrt(np.diag(a.cov))
    fig = (rel(b.se, a.se), float(np.max(np.abs(b.cov - a.cov) / np.outer(sd, sd))),
           rel(b.group_stat, a.group_stat))
    print(f"WORST permuted rows vs sorted: se {fig[0]:.3e} cov {fig[1]:.3e} stat {fig[2]:.3e}")
    assert max(fig) <= 1e-12
    # string labels in another order: the same clusters
    names = np.array([f"t{v:02d}" for v in G - 1 - cid])
    c = glm.inference(X, y, cov_type="cluster", clusters=names, groups=gids, return_cov=True)
    assert np.array_equal(c.cov, a.cov)
    compare("normal permuted", b, reference("normal", glm), BAR[True])


def test_batch_equals_single_calls_bitwise(engine):
    from sglm_hip import inference
    X, y, gids, _, cid = K.gpu_case("ridge")
    models = [fitted("ridge", alpha) for alpha in (25.0, 5.0, 100.0)]
    rs = inference.infer(X, y, models, groups=gids, cov_type="cluster", clusters=cid,
                         return_cov=True)
    assert len(rs) == 3
    for glm, r in zip(models, rs):
        one = inference.infer(X, y, glm, groups=gids, cov_type="cluster", clusters=cid,
                              return_cov=True)
        assert np.array_equal(r.cov, one.cov) and np.array_equal(r.se, one.se)
        assert np.array_equal(r.group_stat, one.group_stat) and r.n_clusters == G
        compare(f"ridge batch alpha={glm.model.alpha}", r, reference("ridge", glm), BAR[True])
    assert not np.array_equal(rs[0].se, rs[1].se)


def test_event_wald_and_kernel_bands(engine):
    import sglm_ez
    from sglm_hip import inference
    X, y, gids, _, cid = K.gpu_case("poisson")
    glm = fitted("poisson")
    r = inference.infer(X, y, glm, groups=gids, cov_type="cluster", clusters=cid)
    w = sglm_ez.event_wald(X, y, glm, cov_type="cluster", clusters=cid)
    assert np.array_equal(w["wald"].values, r.group_stat)
    assert np.array_equal(w["pvalue"].values, r.group_pvalue) and w["dof"].tolist() == [21] * 6
    b = sglm_ez.kernel_bands(X, y, glm, cov_type="cluster", clusters=cid)
    assert np.array_equal(b["se"].values, r.se)
    b0 = sglm_ez.kernel_bands(X, y, glm, cov_type="cluster", clusters=cid,
                              cluster_correction=False)
    assert np.all(b0["se"].values < b["se"].values)
    assert w.loc["ev0", "pvalue"] < 1e-8              # the strong kernel survives clustering


def test_fewer_clusters_than_a_kernel_has_lags(engine):
    X, y, gids, _, cid = K.gpu_case("poisson")
    glm = fitted("poisson")
    few = np.arange(len(y)) // 334                    # G = 12 < 21
    assert len(np.unique(few)) == 12
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r = glm.inference(X, y, cov_type="cluster", clusters=few, groups=gids)
    mine = [w for w in rec if "Wald statistics are NaN" in str(w.message)]
    assert len(mine) == 1 and issubclass(mine[0].category, UserWarning)
    assert "6 group test(s)" in str(mine[0].message) and "G - 1 = 11" in str(mine[0].message)
    assert np.all(np.isnan(r.group_stat)) and np.all(np.isnan(r.group_pvalue))
    assert r.group_dof.tolist() == [21] * 6 and r.n_clusters == 12
    assert np.all(np.isfinite(r.se)) and np.isfinite(r.intercept_se) and np.all(r.se > 0)
    o = K.oracle(C.xt(X), y, C.FAM_TWEEDIE, 1.0, glm.model._objective().lam(4000.0),
                 np.r_[glm.coef_, glm.intercept_], few, groups=gids)
    assert np.all(np.isnan(o["stat"])) and rel(np.r_[r.se, r.intercept_se], o["se"]) <= BAR[False]
    # the status itself, from the batched driver
    from sglm_hip import engine as E
    from sglm_hip import inference
    d = glm.model._design(X.values)
    prob = E.Problem(d, [np.asarray(y, np.float64)], [np.ones(d.n, np.uint8)])
    obj = glm.model._objective()
    goff, gcols = inference.group_lists(gids, 126)[1:3]
    res = inference.infer_problem(prob, [obj.family], [obj.power], [obj.lam(4000.0)], [True],
                                  [glm.coef_], [glm.intercept_], [0], [0], goff, gcols, "cluster",
                                  runs=inference.cluster_runs(few, 4000))
    assert res["status"].tolist() == [[3] * 6] and np.all(np.isnan(res["stat"]))


@pytest.mark.parametrize("name", list(C.GPU_FAMILIES))
def test_singleton_clusters_are_robust(engine, name):
    """clusters = arange(n) without the correction is HC0.  'robust' carries m s^2 as an f32
    weight (three bf16 planes, f32 Gram accumulation); the clustered meat is float64: 1e-6
    relative for Normal / Ridge, 1e-5 otherwise."""
    X, y, gids, _, cid = K.gpu_case(name)
    glm = fitted(name)
    a = glm.inference(X, y, cov_type="cluster", clusters=np.arange(len(y)),
                      cluster_correction=False, groups=gids, return_cov=True)
    b = glm.inference(X, y, cov_type="robust", groups=gids, return_cov=True)
    sd = np.sqrt(np.diag(b.cov))
    fig = (rel(a.se, b.se), float(np.max(np.abs(a.cov - b.cov) / np.outer(sd, sd))),
           rel(a.group_stat, b.group_stat))
    bar = 1e-6 if C.GPU_FAMILIES[name][0] == C.FAM_SQUARED else 1e-5
    print(f"WORST singleton clusters vs robust {name}: se {fig[0]:.3e} cov {fig[1]:.3e} "
          f"stat {fig[2]:.3e}  (bar {bar:.0e})")
    assert a.n_clusters == 4000 and max(fig) <= bar


def test_other_cov_types_are_untouched(engine):
    """'model' and 'robust' before and after a clustered call in one process: the same bits."""
    X, y, gids, _, cid = K.gpu_case("nb2")
    glm = fitted("nb2")
    before = [glm.inference(X, y, cov_type=ct, groups=gids, return_cov=True)
              for ct in ("model", "robust")]
    glm.inference(X, y, cov_type="cluster", clusters=cid, groups=gids, return_cov=True)
    glm.inference(X, y, cov_type="cluster", clusters=np.arange(len(y)) % 50, groups=gids)
    after = [glm.inference(X, y, cov_type=ct, groups=gids, return_cov=True)
             for ct in ("model", "robust")]
    for a, b in zip(before, after):
        assert np.array_equal(a.cov, b.cov) and np.array_equal(a.se, b.se)
        assert np.array_equal(a.group_stat, b.group_stat) and a.scale == b.scale and a.df == b.df
        assert a.n_clusters is None and b.n_clusters is None
