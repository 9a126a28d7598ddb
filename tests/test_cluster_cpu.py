"""Cluster-robust covariance without a device: the oracle of tests/cluster_cases.py against HC0,
its invariances and a case worked by hand; the host-side run / CSR builder; every refusal; the
C ABI names; and the cases themselves (clustering must matter in them)."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import cluster_cases as K
import infer_cases as C
from conftest import ROOT


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a, float) - np.asarray(b, float))) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("fam,power", [(C.FAM_SQUARED, 0.0), (C.FAM_TWEEDIE, 1.0),
                                       (C.FAM_NB2, 0.5)])
def test_singleton_clusters_are_hc0(fam, power):
    Xt, y, ids, beta = C.small_case(fam, power)
    n = Xt.shape[0]
    o = K.oracle(Xt, y, fam, power, 2.0, beta, np.arange(n), correction=False, groups=ids)
    r = C.oracle(Xt, y, fam, power, 2.0, beta, cov_type="robust", groups=ids)
    assert relmax(o["cov"], r["cov"]) <= 1e-12 and relmax(o["se"], r["se"]) <= 1e-12
    assert relmax(o["stat"], r["stat"]) <= 1e-11 and np.array_equal(o["dof"], r["dof"])
    assert o["kappa"] == 1.0 and o["G"] == n


def test_invariant_to_labels_and_row_order():
    Xt, y, ids, beta = C.small_case(C.FAM_TWEEDIE, 1.0)
    n = Xt.shape[0]
    rng = np.random.default_rng(12)
    cid = K.trial_ids(rng, n, 5, 15)
    a = K.oracle(Xt, y, C.FAM_TWEEDIE, 1.0, 1.0, beta, cid, groups=ids)
    relabel = rng.permutation(int(cid.max()) + 1)
    names = np.array([f"trial{v:03d}" for v in relabel])[cid]          # strings, another order
    b = K.oracle(Xt, y, C.FAM_TWEEDIE, 1.0, 1.0, beta, names, groups=ids)
    assert relmax(b["cov"], a["cov"]) <= 1e-13 and b["G"] == a["G"]
    perm = rng.permutation(n)
    c = K.oracle(Xt[perm], y[perm], C.FAM_TWEEDIE, 1.0, 1.0, beta, cid[perm], groups=ids)
    assert relmax(c["cov"], a["cov"]) <= 1e-12 and relmax(c["stat"], a["stat"]) <= 1e-11
    # and it is not HC0
    r = C.oracle(Xt, y, C.FAM_TWEEDIE, 1.0, 1.0, beta, cov_type="robust")
    assert relmax(a["cov"], r["cov"]) > 1e-2


def test_two_clusters_two_columns_by_hand():
    """x~ rows (1,1), (0,1), (1,1), (0,1), clusters 0 0 1 1, Normal at beta = 0 with y = -s,
    s = (1, -2, 3, 1):  A = [[2, 2], [2, 4]], A^-1 = [[1, -.5], [-.5, .5]], g_0 = (1, -1),
    g_1 = (3, 4), M = [[10, 11], [11, 17]], A^-1 M A^-1 = [[3.25, -1], [-1, 1.25]], and
    kappa = 2/1 * 3/(4 - 2) = 3."""
    Xt = np.array([[1.0, 1.0], [0.0, 1.0], [1.0, 1.0], [0.0, 1.0]])
    s = np.array([1.0, -2.0, 3.0, 1.0])
    beta = np.zeros(2)
    o = K.oracle(Xt, -s, C.FAM_SQUARED, 0.0, 0.0, beta, [0, 0, 1, 1], correction=False)
    assert np.allclose(o["M"], [[10, 11], [11, 17]], rtol=0, atol=1e-14)
    assert np.allclose(o["cov"], [[3.25, -1.0], [-1.0, 1.25]], rtol=0, atol=1e-14)
    o3 = K.oracle(Xt, -s, C.FAM_SQUARED, 0.0, 0.0, beta, ["b", "b", "a", "a"])
    assert o3["kappa"] == 3.0
    assert np.allclose(o3["cov"], [[9.75, -3.0], [-3.0, 3.75]], rtol=0, atol=1e-14)
    assert np.allclose(o3["se"], np.sqrt([9.75, 3.75]), rtol=1e-15)


def test_kappa_value():
    from sglm_hip import inference as inf
    assert float(K.kappa(99, 4000, 127)) == pytest.approx(99 / 98 * 3999 / 3873, rel=1e-15)
    assert inf.cluster_kappa(99, 4000.0, 127) == pytest.approx(99 / 98 * 3999 / 3873, rel=1e-15)
    assert inf.cluster_kappa(2, 4, 2) == 3.0
    # a multiplicity mask: n is the sum of the multiplicities
    Xt, y, ids, beta = C.small_case(C.FAM_TWEEDIE, 1.0)
    m = np.r_[np.full(200, 2.0), np.ones(200)]
    o = K.oracle(Xt, y, C.FAM_TWEEDIE, 1.0, 0.0, beta, np.arange(400) // 10, m=m)
    assert o["n"] == 600 and o["kappa"] == pytest.approx(40 / 39 * 599 / (600 - 7), rel=1e-15)


@pytest.mark.parametrize("name", list(C.GPU_FAMILIES))
def test_clustering_matters_in_the_cases(name):
    """At the generating coefficients the clustered intercept s.e. is >= 1.3 x HC0's in every
    family (measured 1.36, Binomial, to 2.60): the cases cannot pass with 'robust' in place."""
    fam, power = C.GPU_FAMILIES[name][:2]
    X, y, gids, beta, cid = K.gpu_case(name)
    assert cid.shape == (C.GPU_N,) and np.all(np.diff(cid) >= 0)
    lens = np.bincount(cid)
    assert lens[:-1].min() >= 20 and lens.max() <= 60 and len(lens) == K.GPU_G == 97
    lam = C.lam_of(name, len(y))
    o = K.oracle(C.xt(X), y, fam, power, lam, beta, cid)
    r = C.oracle(C.xt(X), y, fam, power, lam, beta, cov_type="robust")
    ratio = o["se"] / r["se"]
    print(f"RATIO cluster/HC0 se {name}: intercept {ratio[-1]:.3f} kernels "
          f"{ratio[:-1].min():.3f} .. {ratio[:-1].max():.3f}")
    assert ratio[-1] >= 1.3


# ------------------------------------------------------------------------------ the run builder
def check_runs(ids):
    from sglm_hip import inference as inf
    r = inf.cluster_runs(ids, len(ids))
    G, roff, rc, coff, cruns = K.runs_of(ids)
    assert (r.G, r.R) == (G, len(rc))
    assert r.roff.dtype == np.int32 and np.array_equal(r.roff, roff)
    if len(rc) == G:
        assert r.coff is None and r.cruns is None
    else:
        assert r.coff.dtype == np.int32 and r.cruns.dtype == np.int32
        assert np.array_equal(r.coff, coff) and np.array_equal(r.cruns, cruns)
    return r


def test_run_builder():
    r = check_runs(np.repeat(np.arange(7), [3, 1, 40, 2, 33, 1, 5]))    # time order, a single row
    assert r.R == r.G == 7 and r.roff.tolist() == [0, 3, 4, 44, 46, 79, 80, 85]
    r = check_runs(np.arange(50) % 6)                                   # interleaved
    assert r.R == 50 and r.G == 6 and r.cruns[:3].tolist() == [0, 6, 12]
    r = check_runs(np.array(["s2", "s2", "s10", "s10", "s10", "s2", "a"]))     # strings
    assert r.G == 3 and r.R == 4 and r.roff.tolist() == [0, 2, 5, 6, 7]
    assert r.coff.tolist() == [0, 1, 2, 4] and r.cruns.tolist() == [3, 1, 0, 2]
    r = check_runs(np.array([5, 3, 3, 9]))                              # first seen != sorted
    assert r.coff is None and r.G == 3
    # a Series, an index level, a list
    from sglm_hip import inference as inf
    ids = np.repeat([4, 1, 4], [2, 3, 2])
    want = inf.cluster_runs(ids, 7)
    mi = pd.MultiIndex.from_arrays([ids, np.arange(7)], names=["trial", "t"])
    for form in (pd.Series(ids), mi.get_level_values("trial"), ids.tolist(), ids[:, None]):
        got = inf.cluster_runs(form, 7)
        assert (got.G, got.R) == (2, 3) and np.array_equal(got.roff, want.roff)
        assert np.array_equal(got.cruns, want.cruns)


# ------------------------------------------------------------------------------ refusals
def _fitted(est, p=5):
    est._set_fitted(np.arange(p, dtype=np.float64) / 7, 0.25, 3)
    return est


def test_refusals_without_a_device(monkeypatch):
    from sglm_hip import estimators as est
    from sglm_hip import inference as inf
    X, y = np.zeros((8, 5)), np.zeros(8)
    ids = np.arange(8) // 2
    model = _fitted(est.PoissonRegressor(alpha=0.1))
    with pytest.raises(ValueError, match="needs clusters="):
        model.inference(X, y, cov_type="cluster")
    for ct in ("model", "bayes", "robust"):
        with pytest.raises(ValueError, match="cov_type='cluster' only"):
            model.inference(X, y, cov_type=ct, clusters=ids)
    for bad in (ids[:7], np.r_[ids, 9], np.zeros((8, 2))):
        with pytest.raises(ValueError, match="one label per row"):
            model.inference(X, y, cov_type="cluster", clusters=bad)
    with pytest.raises(ValueError, match="at least 2 clusters"):
        model.inference(X, y, cov_type="cluster", clusters=np.zeros(8, int))
    for bad in (np.r_[np.nan, np.arange(7.0)], np.array([None, "a", "a", "b", "b", "b", "c", "c"],
                                                         dtype=object),
                pd.Series(["a", None, "a", "b", "b", "b", "c", "c"]),
                pd.Series([1.0, 2.0, np.nan, 1.0, 1.0, 2.0, 2.0, 2.0])):
        with pytest.raises(ValueError, match="NaN or None"):
            model.inference(X, y, cov_type="cluster", clusters=bad)
    with pytest.raises(ValueError, match="cov_type must be one of"):
        model.inference(X, y, cov_type="clustered", clusters=ids)
    # what infer refuses today stays refused, and the batched call and the wrapper reach the checks
    with pytest.raises(est.NotYetImplementedError, match="'cd'"):
        _fitted(est.Lasso(0.1)).inference(X, y, cov_type="cluster", clusters=ids)
    with pytest.raises(ValueError, match="at least 2 clusters"):
        inf.infer(X, y, [model, _fitted(est.Ridge(1.0))], cov_type="cluster",
                  clusters=["a"] * 8)
    import sglm
    glm = sglm.GLM("Poisson", alpha=0.1)
    glm._set_fitted(np.zeros(5), 0.0)
    with pytest.raises(ValueError, match="needs clusters="):
        glm.inference(X, y, cov_type="cluster")
    # run scores of one fit beyond SGLM_INFER_BYTES: refused by the number of runs
    monkeypatch.setattr(inf, "INFER_BYTES", 8.0 * 256 * 7)
    with pytest.raises(est.NotYetImplementedError, match="8 runs"):
        model.inference(X, y, cov_type="cluster", clusters=np.arange(8) % 2)
    assert inf.check_run_bytes(inf.cluster_runs(ids, 8), 256) is None      # 4 runs fit


def test_surface_and_exports():
    from sglm_hip import _lib
    from sglm_hip import inference as inf
    r = inf.Inference(coef=np.zeros(1), intercept=0.0, se=np.zeros(1), intercept_se=0.0,
                      z=np.zeros(1), pvalues=np.zeros(1), scale=1.0, df=1.0, n=1.0)
    assert r.n_clusters is None
    assert sorted(inf.COV_TYPES) == ["bayes", "cluster", "model", "robust"]
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sglm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sglm_infer_scores", "sglm_cluster_scores", "sglm_cluster_meat",
                 "sglm_cluster_meat_work_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.sglm_cluster_meat_work_bytes(512, 3, 99) == 3 * 99 * 512 * 8
