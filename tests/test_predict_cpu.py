"""The host side of the fitted-trace bands (sglm_hip.inference.predict_bands)
without a device: the oracle of tests/predict_cases.py against a brute-force loop, the
inverse-link intervals, every refusal that is raised before a launch, the normalisation of
``rows``, the result's fields and the C ABI entries."""
import os
import re
import types

import numpy as np
import pytest

import infer_cases as C
import predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("fam,power", [(C.FAM_SQUARED, 0.0), (C.FAM_TWEEDIE, 1.0)])
def test_oracle_against_brute_force(fam, power):
    Xt, y, ids, beta = C.small_case(fam, power)
    Xt = Xt[:60]
    cov = C.oracle(C.small_case(fam, power)[0], y, fam, power, 0.5, beta)["cov"]
    eta, v = PC.traces(Xt, beta, cov)
    eta_b, v_b = PC.brute(Xt, beta, cov)
    eta_r, v_r, eb, vb = PC.traces_rows(Xt, beta, cov)
    eb2, vb2 = PC.bounds(Xt, beta, cov)
    tiny = 64 * np.finfo(PC.LD).eps
    for a, b in ((eta, eta_b), (v, v_b), (eta_r, eta_b), (v_r, v_b)):
        assert np.max(np.abs(a - b)) <= tiny * np.max(np.abs(b))
    assert np.allclose(eb, eb2, rtol=1e-12, atol=0) and np.allclose(vb, vb2, rtol=1e-12, atol=0)
    assert np.all(v > 0)
    # float64 recursive summation stays inside the bound the kernels are held to
    v64 = np.einsum("ij,jk,ik->i", Xt, cov, Xt)
    assert PC.ratio(PC.ld(v64) - v, vb) <= 1.0
    # per group: the groups' predictors and the intercept add up to eta
    parts = [PC.traces(Xt, beta, cov, np.flatnonzero(ids == g))[0] for g in np.unique(ids)]
    assert np.max(np.abs(sum(parts) + beta[-1] - eta)) <= tiny * np.max(np.abs(eta))
    # a one-column group: v = C_jj on the rows that have the bit, 0 elsewhere
    e1, v1 = PC.traces(Xt, beta, cov, [2])
    assert np.array_equal(np.asarray(v1 != 0), Xt[:, 2] != 0)
    assert np.allclose(np.asarray(v1, float)[Xt[:, 2] != 0], cov[2, 2], rtol=1e-15)


def test_pack_rbits_layout():
    """The numpy packer of the kernel tests follows the header's fragment order."""
    X = np.zeros((3, 70))
    X[0, 0] = X[0, 1] = X[1, 33] = X[2, 69] = 1
    r = PC.pack_rbits(X, 64, 128)
    assert r.shape == (2, 64, 2)
    assert r[0, 0, 0] == (1 << 0) | (1 << 16) and r[0, 0, 1] == 0      # elements 0 and 1
    assert r[0, 1, 1] == 1 << 16 and r[0, 1, 0] == 0                    # element 33: rho = 1
    assert r[1, 2, 0] == 1 << 18                                        # element 5: 2 + 16
    assert not r[:, 3:].any()


# ------------------------------------------------------------------------------ links
@pytest.mark.parametrize("fam", [C.FAM_SQUARED, C.FAM_TWEEDIE, C.FAM_BINOMIAL, C.FAM_NB2])
def test_link_intervals(fam):
    from sglm_hip import inference as inf
    eta = np.r_[-50.0, np.linspace(-6, 6, 25), 50.0]
    se = np.linspace(0.05, 2.0, eta.size)
    for level in (0.5, 0.95):
        z = inf.level_quantile(level)
        assert abs(z - PC.zq(level)) <= 1e-12
        mean, mean_se, lo, hi = inf.link_bands(fam, eta, se, z)
        ref = PC.bands(fam, eta, se, level)
        for got, want in zip((mean, mean_se, lo, hi), ref):
            assert np.allclose(got, want, rtol=1e-12, atol=0)
        assert np.all(np.isfinite(np.r_[mean, mean_se, lo, hi]))
        # monotone inverse links: strictly ordered, but for the logistic function at eta = 50,
        # where 1 - 2e-22 is 1.0 in float64 (never beyond it)
        assert np.all(lo[:-1] < mean[:-1]) and np.all(mean[:-1] < hi[:-1])
        assert lo[-1] <= mean[-1] <= hi[-1] and (fam == C.FAM_BINOMIAL or lo[-1] < hi[-1])
        if fam == C.FAM_BINOMIAL:
            assert np.all(lo > 0) and np.all(hi <= 1) and np.all(hi[:-1] < 1)
            assert np.all(mean_se >= 0) and mean_se[0] > 0 and mean_se[-1] > 0
        elif fam != C.FAM_SQUARED:
            assert np.all(lo > 0) and np.all(mean_se > 0)
        else:
            assert np.array_equal(mean, eta) and np.array_equal(mean_se, se)
    m95 = inf.link_bands(fam, eta, se, inf.level_quantile(0.95))
    m50 = inf.link_bands(fam, eta, se, inf.level_quantile(0.5))
    assert np.all(m95[2][:-1] < m50[2][:-1]) and np.all(m50[3][:-1] < m95[3][:-1])     # nested
    assert m95[2][-1] <= m50[2][-1] and m50[3][-1] <= m95[3][-1]


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
            _fitted(model).predict_bands(X, y)
        with pytest.raises(est.NotYetImplementedError, match=word):
            inf.predict_bands(X, y, [_fitted(est.Ridge(1.0)), model])
    with pytest.raises(est.NotYetImplementedError, match="4095"):
        _fitted(est.Ridge(1.0), p=5000).predict_bands(np.zeros((8, 5000)), y)
    with pytest.raises(AttributeError, match="not fitted"):
        est.PoissonRegressor().predict_bands(X, y)
    with pytest.raises(ValueError, match="cov_type"):
        _fitted(est.Ridge(1.0)).predict_bands(X, y, cov_type="hc3")
    with pytest.raises(ValueError, match="scale"):
        _fitted(est.Ridge(1.0)).predict_bands(X, y, scale=-1.0)
    with pytest.raises(ValueError, match="clusters"):
        _fitted(est.Ridge(1.0)).predict_bands(X, y, cov_type="cluster")
    with pytest.raises(ValueError, match="different numbers"):
        inf.predict_bands(X, y, [_fitted(est.Ridge(1.0)), _fitted(est.Ridge(1.0), p=4)])
    # the new refusals, each before any launch (there is no device here to launch on)
    m = _fitted(est.Ridge(1.0))
    for level in (0.0, 1.0, -0.1, 1.5, float("nan"), "0.9"):
        with pytest.raises(ValueError, match="level"):
            m.predict_bands(X, y, level=level)
    with pytest.raises(ValueError, match="X_new has 4 features"):
        m.predict_bands(X, y, X_new=np.zeros((3, 4)))
    Xn = np.zeros((3, 5))
    Xn[1, 2] = 0.5
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        m.predict_bands(X, y, X_new=Xn)
    for rows in ([0, 8], [-1], np.array([3, 9, 1])):
        with pytest.raises(ValueError, match="rows must lie in"):
            m.predict_bands(X, y, rows=rows)
    with pytest.raises(ValueError, match="rows must lie in \\[0, 3\\)"):
        m.predict_bands(X, y, X_new=np.zeros((3, 5)), rows=[3])
    with pytest.raises(ValueError, match="rows must be"):
        m.predict_bands(X, y, rows=[0.5, 1.0])
    with pytest.raises(ValueError, match="rows must be"):
        m.predict_bands(X, y, rows=[[0, 1]])
    # the wrappers reach the same checks
    import pandas as pd
    import sglm
    import sglm_ez
    glm = sglm.GLM("Normal", alpha=0.1, l1_ratio=0.5)
    glm._set_fitted(np.zeros(5), 0.0)
    with pytest.raises(est.NotYetImplementedError, match="'cd'"):
        glm.predict_bands(X, y)
    ok = sglm.GLM("Normal", alpha=0.1, l1_ratio=0)
    ok._set_fitted(np.zeros(5), 0.0)
    with pytest.raises(ValueError, match="level"):
        ok.predict_bands(X, y, level=2)
    F = pd.DataFrame(X, columns=["a", "a_1", "a_2", "b", "b_1"])
    with pytest.raises(ValueError, match="level"):
        sglm_ez.fitted_bands(F, y, ok, level=1.0)
    with pytest.raises(ValueError, match="rows must lie in"):
        sglm_ez.event_contributions(F, y, ok, rows=[8])


def test_output_size_refusal(monkeypatch):
    from sglm_hip import estimators as est
    from sglm_hip import inference as inf
    monkeypatch.setattr(inf, "INFER_BYTES", 1000.0)
    assert inf.check_band_bytes(10, 5) == 960
    with pytest.raises(est.NotYetImplementedError, match="1.01e\\+03 bytes"):
        inf.check_band_bytes(9, 6)
    X, y = np.zeros((8, 5)), np.zeros(8)
    with pytest.raises(est.NotYetImplementedError, match="SGLM_INFER_BYTES"):
        _fitted(est.Ridge(1.0)).predict_bands(X, y, groups=[0, 1, 2, 3, 4], rows=[0] * 11)
    assert inf.check_band_bytes(11, 0) == 176       # the same rows without the groups fit


def test_design_refusals():
    from sglm_hip import estimators as est
    from sglm_hip import inference as inf
    ok = dict(slab=None, cont=None, xbits=object(), P=256, p=100)
    # _resolve_design: the one place predict_bands and infer take the fitted design through
    for change, word in ((dict(slab=(0, 10, 20)), "row-sharded"), (dict(cont=object()), "mixed"),
                         (dict(xbits=None), "non-binary"), (dict(P=4352, p=4200), "4095")):
        d = types.SimpleNamespace(**{**ok, **change})
        model = types.SimpleNamespace(_design=lambda X, d=d: d)
        with pytest.raises(est.NotYetImplementedError, match=word):
            inf._resolve_design([(model, None)], None, d.p)
    d = types.SimpleNamespace(**ok)
    with pytest.raises(ValueError, match="100 features"):
        inf._resolve_design([(types.SimpleNamespace(_design=lambda X: d), None)], None, 99)


# ------------------------------------------------------------------------------ rows, fields
def test_rows_normalisation():
    from sglm_hip import inference as inf
    assert inf.normalize_rows(None, 10) is None
    for rows, want in ((slice(2, 5), [2, 3, 4]), (slice(None, None, 4), [0, 4, 8]),
                       (slice(8, 20), [8, 9]), (slice(-2, None), [8, 9]), (slice(5, 5), []),
                       ([5, 5, 3, 9], [5, 5, 3, 9]), (np.array([9, 0], np.int64), [9, 0]),
                       ((1,), [1]), ([], [])):
        got = inf.normalize_rows(rows, 10)
        assert got.dtype == np.int32 and got.flags.c_contiguous and got.tolist() == want
    for rows in ([10], [-1], [0, 10, 1]):
        with pytest.raises(ValueError, match="\\[0, 10\\)"):
            inf.normalize_rows(rows, 10)
    for rows in (3, [0.0], [[1]], [True, False]):
        with pytest.raises(ValueError, match="rows must be"):
            inf.normalize_rows(rows, 10)


def test_fields_and_surface():
    import sglm
    import sglm_ez
    from sglm_hip import estimators as est
    from sglm_hip import inference as inf
    fields = [f.name for f in inf.PredictionBands.__dataclass_fields__.values()]
    assert fields == ["eta", "eta_se", "mean", "mean_se", "lo", "hi", "level", "group_ids",
                      "group_eta", "group_se", "group_lo", "group_hi"]
    z = np.zeros(2)
    pb = inf.PredictionBands(z, z, z, z, z, z, 0.9)
    assert pb.group_ids is None and pb.group_hi is None and pb.level == 0.9
    # Inference is as it was
    assert [f.name for f in inf.Inference.__dataclass_fields__.values()][-1] == "cov"
    assert callable(sglm.GLM.predict_bands) and callable(est._EngineRegressor.predict_bands)
    assert callable(sglm_ez.fitted_bands) and callable(sglm_ez.event_contributions)
    import inspect
    sig = inspect.signature(inf.predict_bands)
    assert list(sig.parameters) == ["X", "y", "models", "X_new", "rows", "groups", "level",
                                    "cov_type", "scale", "clusters", "cluster_correction"]
    assert sig.parameters["level"].default == 0.95 and sig.parameters["cov_type"].default == "model"
    # infer_problem's public arguments are as they were; the hand-over is keyword-only in spirit
    names = list(inspect.signature(inf.infer_problem).parameters)
    assert names[:17] == ["prob", "fams", "powers", "lams", "icpts", "coefs", "intercepts", "resps",
                          "masks", "goff", "gcols", "cov_type", "scale", "return_cov", "runs",
                          "cluster_correction", "_on_chunk"]


def test_exports():
    from sglm_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sglm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sglm_predict_rows", "sglm_predict_groups"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["sglm_predict_rows"][1]) == 15
    assert len(_lib.SIGNATURES["sglm_predict_groups"][1]) == 17
    assert list(_lib.SIGNATURES)[-2:] == ["sglm_predict_rows", "sglm_predict_groups"]
