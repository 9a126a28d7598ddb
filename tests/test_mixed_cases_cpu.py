"""CPU sanity checks of the inputs, references and bounds that tests/test_gpu_mixed_kernels.py
holds csrc/mixed.hip to (tests/mixed_cases.py): if a plain float64 np.dot of the same inputs
does not sit inside a bound against the np.longdouble sum, the inputs or the bound are wrong,
not the kernel."""
import numpy as np
import pytest

import mixed_cases as mc
from oracle import glm_ref


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def test_longdouble_is_wider_than_float64():
    assert mc.have_longdouble()


@pytest.mark.parametrize("n,k,wmode", mc.GRAM_CASES)
def test_gram_float64_dot_inside_bound(n, k, wmode):
    c = mc.gram_case(n, k, wmode)
    assert np.all(c["bound"] > 0)
    assert mc.ratio(mc.gram_float64(c), c["ref"], c["bound"]) <= 1.0


@pytest.mark.parametrize("mode,n,k,nq,indep", mc.XTR_CASES)
def test_xtr_float64_dot_inside_bound(mode, n, k, nq, indep):
    c = mc.xtr_case(mode, n, k, nq, indep)
    assert np.all(c["bound"] > 0)
    assert mc.ratio(mc.xtr_float64(c), c["ref"], c["bound"]) <= 1.0
    # the padding rows of R hold finite non-zero junk, those of C zeros
    val = np.asarray(c["val"], dtype=np.float64)
    assert np.all(val[:, n:] != 0) and np.all(c["C"][:, n:] == 0) and np.all(np.isfinite(val))


@pytest.mark.parametrize("n,k,nq", [(33795, 5, 11), (3, 1, 1)])
def test_pieces_reconstruct_r(n, k, nq):
    """The generated planes: hi + mid + lo == R exactly (float64 and f32 sums alike), and every
    piece is needed (dropping lo changes R)."""
    c = mc.xtr_case(2, n, k, nq, False)
    Rf = c["Rf"]
    pl = mc.bf16_bits_to_f32(c["R"]).astype(np.float64)
    assert np.array_equal((pl[0] + pl[1]) + pl[2], Rf.astype(np.float64))
    assert np.array_equal(np.asarray(c["val"], dtype=np.float64), Rf.astype(np.float64))
    if n > 100:
        assert np.mean(pl[2] != 0) > 0.9 and np.mean(pl[1] != 0) > 0.9
    # bf16 round trip of the helper: representable values are kept, ties go to even
    x = np.array([1.0, -2.5, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20],
                 dtype=np.float32)
    assert np.array_equal(mc.bf16_bits_to_f32(mc.f32_to_bf16_bits(x)),
                          np.array([1.0, -2.5, 1.0, 1.015625, 1.0078125], dtype=np.float32))


def test_independent_pieces_differ_from_split():
    c = mc.xtr_case(2, 33795, 5, 11, True)
    pl = mc.bf16_bits_to_f32(c["R"]).astype(np.float64)
    assert np.array_equal(np.asarray(c["val"], dtype=np.float64), (pl[0] + pl[1]) + pl[2])
    assert np.mean(np.abs(pl[1]) > 2.0 ** -7 * np.abs(pl[0])) > 0.5     # no rounding residue


@pytest.mark.parametrize("name", [c[0] for c in mc.ETA_CASES if c[2] <= 16])
def test_eta_float64_dot_inside_bound(name):
    c = mc.eta_case(name)
    got = mc.eta_float64(c)
    assert mc.eta_ratio(c, got) <= 1.0
    # an unlisted slot exists wherever the buffer has more rows than fits
    assert c["rows"] == c["nb"] or np.setdiff1d(np.arange(c["rows"]), c["slots"]).size > 0


def test_oracle_stable_under_row_permutation():
    """The float64 oracle reproduces itself on the k = 5 design at the bars the GPU fits are
    held to (1e-5 OLS, 1e-4 Poisson) when the rows are permuted: the design is well enough
    conditioned for those bars to test the engine, not the oracle."""
    c = mc.design_case(5)
    X = c["X"]
    assert np.linalg.cond(np.hstack([X, np.ones((c["n"], 1))])) < 1e3
    perm = np.random.default_rng(7).permutation(c["n"])
    w0, b0 = glm_ref.fit_ols(X, c["y"])
    w1, b1 = glm_ref.fit_ols(X[perm], c["y"][perm])
    assert rel(w1, w0) < 1e-5 * 1e-3 and abs(b1 - b0) < 1e-5 * 1e-3
    w0, b0 = glm_ref.fit_tweedie_newton(X, c["ypois"], 1e-3, 1.0)
    w1, b1 = glm_ref.fit_tweedie_newton(X[perm], c["ypois"][perm], 1e-3, 1.0)
    assert rel(w1, w0) < 1e-4 * 1e-3 and abs(b1 - b0) < 1e-4 * 1e-3


@pytest.mark.parametrize("k", [5, 80])
def test_design_case_layout(k):
    c = mc.design_case(k)
    X = c["X"]
    nonbin = np.flatnonzero(~((X == 0) | (X == 1)).all(axis=0))
    assert np.array_equal(nonbin, c["cpos"]) and nonbin.size == k
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    assert np.any(np.diff(nonbin) > 1)                                   # interleaved
