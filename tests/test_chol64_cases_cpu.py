"""CPU checks of the cases that tests/test_gpu_chol64_kernels.py holds csrc/chol64.hip and
csrc/chol64_drop.hip to (tests/chol64_cases.py): the plain float64 numpy transcription of every
algorithm sits inside every bound against the np.longdouble references, no rank decision is taken
on a knife edge except the deliberate powers-of-two one (whose intermediates are exact), and the
references do not depend on the order of the kept coordinates.  If one of these fails, the cases
or the bounds are wrong, not the kernels."""
import numpy as np
import pytest

import chol64_cases as cc

pytestmark = pytest.mark.skipif(not cc.have_longdouble(),
                                reason="np.longdouble is not wider than float64 by 7 bits here")
LD = cc.LD


def test_longdouble_eps():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


def test_ratio_zero_handling():
    assert cc.ratio([0.0, 1.0], [0.0, 1.0], [0.0, 0.0]) == 0.0
    assert cc.ratio([1e-300], [0.0], [0.0]) == np.inf
    assert cc.ratio([np.nan], [0.0], [0.0]) == np.inf
    assert not cc.ratio([np.nan], [0.0], [1.0]) <= 1.0
    assert cc.ratio([1.5], [1.0], [1.0]) == 0.5


# ------------------------------------------------------------------------------ factor
@pytest.mark.parametrize("name", list(cc.FACTOR_CASES))
def test_factor_transcription(name):
    c = cc.factor_case(name)
    P, tol = c["P"], c["tol"]
    assert np.all(c["state"][:, c["p"] + 1:] == cc.EXCL)
    for f in range(3):
        U, state, piv = cc.factor_f64(c["A"][f], c["dshift"][c["dsrc"][f]] < 0, tol)
        assert np.array_equal(state, c["state"][f])
        assert cc.factor_structure(U, state) == []
        assert cc.factor_ratio(c["A"][f], state, U) <= 1.0
        # no decision near the threshold
        assert np.all(piv[state == cc.DEP] < 1e-3 * tol)
        assert np.all(piv[state == cc.KEPT] > 1e3 * tol)
    nd = c["counts"][:, 0]
    assert nd[1] == 0 and nd[0] == nd[2] == len(c["nullvecs"])
    if P > 64:
        assert nd[0] >= 6
    assert (c["state"][0][c["p"]] == cc.DEP) == c["onehot"]
    # the null vectors of the construction are null vectors of the Gram
    G = cc.sym_upper(c["H"][1])
    for v in c["nullvecs"].values():
        assert not np.any(G @ v)


@pytest.mark.parametrize("which", cc.TOL_EDGE)
def test_tol_edge_is_exact(which):
    c = cc.tol_edge_case(which)
    a, b = c["a"], c["b"]
    for tol, dep in zip(c["tols"], (True, False)):
        U, state, piv = cc.factor_f64(c["A"], c["excl"], tol)
        assert state[b] == (cc.DEP if dep else cc.KEPT) and piv[b] == 0.5
        assert np.array_equal(U, c["U"])
        K = np.flatnonzero(state == cc.KEPT)
        assert np.array_equal((U.T @ U)[np.ix_(K, K)], c["A"][np.ix_(K, K)])
        assert U[a, b] * U[a, b] + 1.0 == c["A"][b, b]
    assert c["tols"][0] * 2.0 == 1.0 and c["tols"][1] * 2.0 == np.nextafter(1.0, 0.0)


def test_mixed_factor_transcription():
    c = cc.mixed_factor_case()
    assert not np.any(np.isnan(c["A"]))
    assert np.mean(c["S"][:, :, :c["p"]] != np.round(c["S"][:, :, :c["p"]])) > 0.95
    for f in range(2):
        U, state, piv = cc.factor_f64(c["A"][f], c["dshift"][c["dsrc"][f]] < 0, c["tol"])
        assert np.array_equal(state, c["state"][f])
        assert cc.factor_ratio(c["A"][f], state, U) <= 1.0
        assert np.all(piv[state == cc.DEP] < 1e-3 * c["tol"])
        assert np.all(piv[state == cc.KEPT] > 1e3 * c["tol"])
        if c["dsrc"][f] == 1:                         # unpenalised: A[0][0] = 1024 exactly
            assert np.array_equal(U[0, state != cc.EXCL], c["A"][f][0, state != cc.EXCL] / 32.0)
    # the copies the rule does not select differ, in the last bit
    S, cp = c["S"][0], c["cpos"]
    assert S[0, 0] == np.nextafter(S[1, 70], np.inf) and S[2, 70] == np.nextafter(S[0, 130], np.inf)
    assert c["A"][0][0, 70] == S[1, 70] and c["A"][0][70, 130] == S[0, 130]
    assert len(set(np.asarray(cp) // 64)) == 3


# ------------------------------------------------------------------------------ solves, residual
@pytest.mark.parametrize("P", cc.SOLVE_PS)
def test_solve_transcription(P):
    c = cc.solve_case(P)
    for f in range(2):
        assert np.all(np.isnan(c["U"][f][np.tril_indices(P, -1)]))
        for q in range(2):
            x = cc.solve_f64(c["U"][f], c["state"][f], c["g"][q])
            assert cc.solve_ratio(c["U"][f], c["state"][f], x, c["g"][q]) <= 1.0
            x32 = x.astype(np.float32).astype(np.float64)
            assert cc.solve_ratio(c["U"][f], c["state"][f], x32, c["g"][q], f32=True) <= 1.0
            assert cc.solve_ratio(c["U"][f], c["state"][f], x32, c["g"][q]) > 1.0


@pytest.mark.parametrize("mixed", [False, True])
def test_resid_transcription(mixed):
    c = cc.resid_case(192, mixed)
    assert cc.ratio(cc.resid_f64(c), c["ref"], c["bound"]) <= 1.0
    assert len({tuple(r) for r in c["lamp"]}) == c["rows"]


# ------------------------------------------------------------------------------ minnorm, drop
@pytest.mark.parametrize("name", cc.MINNORM_CASES)
def test_minnorm_transcription(name):
    c, fc = cc.minnorm_case(name), cc.factor_case(name)
    for q, (fit, f) in enumerate(zip(c["fits"], c["fsrc"])):
        print(f"minnorm {name} fit {q}: e_ref {c['e_ref'][q]:.3e} floor {c['floor'][q]:.3e}")
        assert cc.ratio(c["trans"][q], c["ref"][q], c["bound"][q]) <= 1.0 / 16
        ref = c["ref"][q]
        off = fc["state"][f] >= cc.EXCL
        assert np.array_equal(ref[off].astype(np.float64), c["beta"][fit][off])
        G = cc.ld(cc.sym_upper(fc["H"][fc["hsrc"][f]]))
        assert np.max(np.abs(G @ (ref - cc.ld(c["beta"][fit])))) <= 2.0 ** -55 * np.max(G)
    assert np.array_equal(c["ref"][1].astype(np.float64), c["beta"][c["fits"][1]])


@pytest.mark.parametrize("name", cc.DROP_CASES)
def test_drop_transcription(name):
    c = cc.drop_case(name)
    assert [e is None for e in c["expect"]] == [c["status"][p] == 2 for p in c["psrc"]]
    for q in range(c["nq"]):
        if c["expect"][q] is None:
            continue
        keep, ref, bound, e, floor, sset = cc.drop_expected(c, q, int(c["gsrc"][q]))
        print(f"drop {name} q {q}: e_ref {e:.3e} floor {floor:.3e}")
        assert e <= bound / 16 and keep.size + len(set(sset) - {7, 150}) <= c["P"]


def test_structured_factor_matches_dense():
    """The O(P) longdouble products and substitutions of RankOneUpper against dense longdouble
    ones at P = 256, and the P = 8192 checks on a small copy."""
    c = cc.big_case(256, (130, 200))
    R, U, g = c["R"], c["U"], c["g"]
    assert np.array_equal(np.triu(np.outer(R.a, R.b), 1), np.triu(U, 1))     # exact products
    Ul = cc.ld(U)
    tiny = 2.0 ** -58
    assert np.max(np.abs(R.mul(g) - Ul @ cc.ld(g))) < tiny * np.max(np.abs(g)) * 4
    assert np.max(np.abs(R.tmul(g) - Ul.T @ cc.ld(g))) < tiny * np.max(np.abs(g)) * 4
    y = R.ainv(g)
    assert np.max(np.abs(Ul.T @ (Ul @ y) - cc.ld(g))) < tiny * np.max(np.abs(g)) * 16
    keep = c["keep"]
    ref = cc.ld_spd_solve((Ul.T @ Ul)[np.ix_(keep, keep)], g[keep])
    assert np.max(np.abs(ref - c["ref"])) < tiny * 64 * np.max(np.abs(ref))
    assert c["e_ref"] <= c["bound"] / 16
    x = cc.solve_f64(U, np.zeros(256, np.uint8), g)
    assert R.solve_ratio(x, g) <= 1.0
    assert R.solve_ratio(x.astype(np.float32).astype(np.float64), g, f32=True) <= 1.0


# ------------------------------------------------------------------------------ permutations
def test_references_stable_under_permutation():
    """A symmetric permutation of the kept coordinates changes each longdouble reference by less
    than 2^-60 of its size."""
    eps = 2.0 ** -60
    rng = np.random.default_rng(50)
    # residual: permute the coordinates of one fit
    c = cc.resid_case(192, False)
    q, fit, f = 0, c["fits"][0], c["fsrc"][0]
    G = cc.assemble(c["H"][c["hsrc"][f]], None, None)
    ex = c["dshift"][fit] < 0
    xs = np.where(ex, 0.0, c["x"][fit])
    perm = rng.permutation(192)
    gx, agx = cc._ld_matvec(G[np.ix_(perm, perm)], xs[perm])
    r = cc.ld(c["c"][c["csrc"][q]])[perm] - (gx + cc.ld(c["lamp"][fit])[perm] * cc.ld(xs)[perm])
    r = np.where(ex[perm], 0.0, r)
    scale = np.abs(cc.ld(c["c"][c["csrc"][q]]))[perm] + agx
    d = float(np.max(np.abs(r - c["ref"][q][perm]) / scale))
    print(f"resid permutation: {d / eps:.3f} x 2^-60")
    assert d < eps
    # minnorm: permute the coefficients (the intercept stays)
    m, fc = cc.minnorm_case("p320"), cc.factor_case("p320")
    p, P = m["p"], m["P"]
    perm = np.r_[rng.permutation(p), np.arange(p, P)]
    N = np.array(list(fc["nullvecs"].values()))
    r = cc.minnorm_ref(N[:, perm], p, m["beta"][m["fits"][0]][perm])
    d = float(np.max(np.abs(r - m["ref"][0][perm])) / np.max(np.abs(r)))
    print(f"minnorm permutation: {d / eps:.3f} x 2^-60")
    assert d < eps
    # drop: permute the kept coordinates of the reduced system
    c = cc.drop_case("k41")
    keep, ref, *_ = cc.drop_expected(c, 1, 0)
    U, state, _ = cc.drop_factors()
    f = c["expect"][1][0]
    K, Uk = cc.kept_block(U[f], state[f])
    A = cc.ld(Uk).T @ cc.ld(Uk)
    sel = np.flatnonzero(np.isin(K, keep))
    sp = rng.permutation(sel)
    r = cc.ld_spd_solve(A[np.ix_(sp, sp)], cc.drop_rhs()[0][K[sp]])
    r = r[np.argsort(K[sp])]                     # back to ascending order
    d = float(np.max(np.abs(r - ref)) / np.max(np.abs(ref)))
    print(f"drop permutation: {d / eps:.3f} x 2^-60")
    assert d < eps
