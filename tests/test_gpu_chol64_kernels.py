"""The float64 chain of csrc/chol64.hip and csrc/chol64_drop.hip, entry point by entry point through
the C ABI, against np.longdouble references: factor (pure 0/1 and mixed), the two solves, the
Gram-space residual, the minimum-norm projection and the drop-set solves, at P = 64 / 192 / 320
(one block; the first size whose trailing update walks a second tile row; three tile rows and
more rows than waves in every partial sum), the residual once at P = 3328 and the solves once at
P = 8192 (the LDS opt-in edges), then two fits through the drop-in GLM.

Inputs, references, transcriptions and the derived bounds are in tests/chol64_cases.py, its CPU
checks in tests/test_chol64_cases_cpu.py.  Every test prints its worst error / bound as a RATIO
line.  Unwritten outputs hold sentinels; work buffers have the queried size plus
a 4 KiB guard that must keep its sentinel."""
import numpy as np
import pytest

import chol64_cases as cc
from oracle import glm_ref

pytestmark = pytest.mark.gpu
SENT, ISENT, BSENT = cc.SENT, cc.ISENT, cc.BSENT
TOL_GAUSS = 1e-5


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def bits(a):
    """The bit patterns of a float array (bitwise comparisons, NaN-safe)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def work_with_guard(torch, nbytes, fill=SENT):
    """float64 tensor of the queried work size (filled with ``fill``) and a 4 KiB sentinel guard."""
    assert nbytes % 8 == 0
    w = torch.full(((nbytes + cc.GUARD) // 8,), SENT, dtype=torch.float64, device="cuda")
    w[:nbytes // 8] = fill
    return w


def guard_intact(work, nbytes):
    g = work[nbytes // 8:].cpu().numpy()
    return g.size == cc.GUARD // 8 and np.array_equal(bits(g), bits(np.full_like(g, SENT)))


# ------------------------------------------------------------------------------ factor
def _factor(torch, c, tol=None, mixed=False):
    """Run the factor of a case on sentinel-filled outputs -> device tensors and host copies."""
    from sglm_hip import _lib
    P, nf = c["P"], c["H"].shape[0] if "nf" not in c else c["nf"]
    t = dict(H=dev(torch, c["H"]), ds=dev(torch, c["dshift"]), lp=dev(torch, c["lamp"]),
             hsrc=dev(torch, c.get("hsrc", np.zeros(nf, np.int32))),
             dsrc=dev(torch, c.get("dsrc", np.zeros(nf, np.int32))))
    t["U"] = torch.full((nf, P, P), SENT, dtype=torch.float64, device="cuda")
    t["state"] = torch.full((nf, P), BSENT, dtype=torch.uint8, device="cuda")
    t["nulls"] = torch.full((nf, P), ISENT, dtype=torch.int32, device="cuda")
    t["counts"] = torch.full((nf, 2), ISENT, dtype=torch.int32, device="cuda")
    wb = _lib.query("sglm_chol64_work_bytes", P, nf)
    t["work"] = work_with_guard(torch, wb)
    tol = c["tol"] if tol is None else tol
    if mixed:
        t["S"], t["cmap"] = dev(torch, c["S"]), dev(torch, c["cmap"])
        _lib.call("sglm_chol64_factor_mixed", ptr(t["H"]), P, ptr(t["hsrc"]), ptr(t["ds"]),
                  ptr(t["lp"]), ptr(t["dsrc"]), nf, tol, ptr(t["S"]), c["k"], ptr(t["cmap"]),
                  ptr(t["U"]), ptr(t["state"]), ptr(t["nulls"]), ptr(t["counts"]),
                  ptr(t["work"]), 0)
    else:
        _lib.call("sglm_chol64_factor", ptr(t["H"]), P, ptr(t["hsrc"]), ptr(t["ds"]), ptr(t["lp"]),
                  ptr(t["dsrc"]), nf, tol, ptr(t["U"]), ptr(t["state"]), ptr(t["nulls"]),
                  ptr(t["counts"]), ptr(t["work"]), 0)
    torch.cuda.synchronize()
    assert guard_intact(t["work"], wb)
    h = {k: t[k].cpu().numpy() for k in ("U", "state", "nulls", "counts")}
    return t, h


def _check_factor(c, h, label):
    """state, nulls, counts exact; both backward bounds; the exact structure of U."""
    nf = h["U"].shape[0]
    assert np.array_equal(h["state"], c["state"])
    assert np.array_equal(h["counts"], c["counts"])
    worst = 0.0
    for f in range(nf):
        nd = c["counts"][f][0]
        assert np.array_equal(h["nulls"][f][:nd], c["nulls"][f])
        assert np.all(h["nulls"][f][nd:] == ISENT)
        assert cc.factor_structure(h["U"][f], h["state"][f]) == []
        worst = max(worst, cc.factor_ratio(c["A"][f], h["state"][f], h["U"][f]))
    print(f"RATIO factor {label}: {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(cc.FACTOR_CASES))
def test_factor(engine, torch_mod, name):
    """nf = 3 on hsrc = [1, 0, 1], dsrc = [2, 0, 1]: two unpenalised factors (different interior
    exclusions) and a ridge one, lamp given or NULL; copies across and at block edges, a sum over
    two blocks, a copy of a dropped copy, zero columns at block edges, and (p320, p192_nolamp) a
    one-hot triple that makes the intercept the dependent pivot.  The strict lower triangle of H
    is NaN."""
    c = cc.factor_case(name)
    _, h = _factor(torch_mod, c)
    _check_factor(c, h, name)


@pytest.mark.parametrize("which", cc.TOL_EDGE)
def test_factor_tol_edge(engine, torch_mod, which):
    """A Schur complement of exactly 1.0 on a diagonal of 2.0: dependent at tol = 0.5 ("<= tol *
    diagonal"), kept with U_bb == 1.0 at the next float64 below; in the first columns of a block
    and right after a panel and a trailing update (coordinates 63, 64)."""
    c = cc.tol_edge_case(which)
    P, b = c["P"], c["b"]
    for tol, dep in zip(c["tols"], (True, False)):
        _, h = _factor(torch_mod, c, tol=tol)
        state = np.where(c["excl"], cc.EXCL, cc.KEPT).astype(np.uint8)
        if dep:
            state[b] = cc.DEP
        assert np.array_equal(h["state"][0], state), (tol, h["state"][0][[c["a"], b]])
        assert h["counts"][0].tolist() == [int(dep), int(dep)]
        assert h["nulls"][0][:1].tolist() == ([b] if dep else [ISENT])
        assert np.array_equal(bits(np.triu(h["U"][0])), bits(c["U"]))
        assert cc.factor_structure(h["U"][0], h["state"][0]) == []


def test_factor_mixed(engine, torch_mod):
    """k = 3 continuous coordinates in three blocks of P = 192 read from S[f] (indexed by the
    factor, hsrc = [1, 0]); their rows and columns of H are NaN.  Row 0 of the unpenalised factor
    is A[0][.] / 32 exactly, which shows that a continuous-continuous entry comes from the S row
    of the smaller index (the other copy differs in its last bit); the continuous copy 130 of 70
    and the 0/1 copy 64 of 10 are dependent."""
    c = cc.mixed_factor_case()
    _, h = _factor(torch_mod, c, mixed=True)
    assert not np.any(np.isnan(h["U"]))
    _check_factor(c, h, "mixed")
    on = c["state"][0] != cc.EXCL
    assert np.array_equal(bits(h["U"][0][0, on]), bits(c["A"][0][0, on] / 32.0))


# ------------------------------------------------------------------------------ solves
@pytest.mark.parametrize("P", cc.SOLVE_PS)
def test_solves(engine, torch_mod, P):
    """nq = 5 over two host-built factors (dependent, excluded and zero coordinates; NaN everywhere
    below the diagonal), fits / fsrc / gsrc non-identity, gsrc NULL once; solve_add onto a
    non-zero x twice (bitwise) against the from-zero result (one rounding)."""
    torch = torch_mod
    from sglm_hip import _lib
    c = cc.solve_case(P)
    U, st, g = dev(torch, c["U"]), dev(torch, c["state"]), dev(torch, c["g"])
    fits, fsrc, gsrc = dev(torch, c["fits"]), dev(torch, c["fsrc"]), dev(torch, c["gsrc"])
    nq, rows = c["nq"], cc.SOLVE_ROWS
    other = np.setdiff1d(np.arange(rows), c["fits"])
    # sglm_chol64_solve
    delta = torch.full((rows, P), SENT, dtype=torch.float32, device="cuda")
    _lib.call("sglm_chol64_solve", ptr(U), P, ptr(st), ptr(fits), ptr(fsrc), nq, ptr(g),
              ptr(delta), 0)
    torch.cuda.synchronize()
    dl = delta.cpu().numpy()
    worst = 0.0
    for fit, f in zip(c["fits"], c["fsrc"]):
        x = -dl[fit].astype(np.float64)
        worst = max(worst, cc.solve_ratio(c["U"][f], c["state"][f], x, c["g"][fit], f32=True))
        assert np.all(dl[fit][c["state"][f] != cc.KEPT] == 0.0)
    print(f"RATIO solve P={P}: {worst:.3e}")
    assert worst <= 1.0
    assert np.array_equal(bits(dl[other]), bits(np.full((other.size, P), SENT, np.float32)))

    def add(start, gs):
        x = torch.full((rows, P), SENT, dtype=torch.float64, device="cuda")
        x[fits.long()] = dev(torch, start)[fits.long()]
        _lib.call("sglm_chol64_solve_add", ptr(U), P, ptr(st), ptr(fits), ptr(fsrc), ptr(gs), nq,
                  ptr(g), ptr(x), 0)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        assert np.array_equal(bits(xh[other]), bits(np.full((other.size, P), SENT)))
        return xh

    zero = np.zeros((rows, P))
    for gs, rhs, label in ((gsrc, c["gsrc"], "gsrc"), (None, c["fits"], "gsrc=NULL")):
        xh = add(zero, gs)
        worst = 0.0
        for fit, f, r in zip(c["fits"], c["fsrc"], rhs):
            worst = max(worst, cc.solve_ratio(c["U"][f], c["state"][f], xh[fit], c["g"][r]))
            off = c["state"][f] != cc.KEPT
            assert np.array_equal(bits(xh[fit][off]), bits(zero[fit][off]))
        print(f"RATIO solve_add P={P} {label}: {worst:.3e}")
        assert worst <= 1.0
    x_zero = add(zero, gsrc)
    x_a, x_b = add(c["x0"], gsrc), add(c["x0"], gsrc)
    assert np.array_equal(bits(x_a), bits(x_b))
    worst = 0.0
    for fit, f in zip(c["fits"], c["fsrc"]):
        off = c["state"][f] != cc.KEPT
        assert np.array_equal(bits(x_a[fit][off]), bits(c["x0"][fit][off]))
        d = cc.ld(x_a[fit]) - cc.ld(c["x0"][fit])
        worst = max(worst, cc.ratio(d, x_zero[fit], cc.U53 * np.abs(x_a[fit])))
    print(f"RATIO solve_add P={P} onto x0: {worst:.3e}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------ residual
def _resid(torch, c):
    from sglm_hip import _lib
    P = c["P"]
    t = {k: dev(torch, c[k]) for k in ("H", "S", "cmap", "hsrc", "fits", "fsrc", "csrc", "c",
                                        "lamp", "dshift", "x")}
    r = torch.full((c["rows"], P), SENT, dtype=torch.float64, device="cuda")
    _lib.call("sglm_chol64_resid", ptr(t["H"]), P, ptr(t["hsrc"]), ptr(t["S"]), c["k"],
              ptr(t["cmap"]), ptr(t["fits"]), ptr(t["fsrc"]), ptr(t["csrc"]), c["nq"], ptr(t["c"]),
              ptr(t["lamp"]), ptr(t["dshift"]), ptr(t["x"]), ptr(r), 0)
    torch.cuda.synchronize()
    got = r.cpu().numpy()
    worst = cc.ratio(got[c["fits"]], c["ref"], c["bound"])
    for fit in c["fits"]:
        assert np.all(got[fit][c["dshift"][fit] < 0] == 0.0)
    other = np.setdiff1d(np.arange(c["rows"]), c["fits"])
    assert np.array_equal(bits(got[other]), bits(np.full((other.size, P), SENT)))
    return worst


@pytest.mark.parametrize("mixed", [False, True])
def test_resid(engine, torch_mod, mixed):
    """P = 192, nq = 4 over two Grams (hsrc = [1, 0]), lamp / dshift / x / r by fit, c by csrc, all
    rows different; with S / cmap (k = 3, the continuous rows and columns of H NaN) and without.
    The lower triangle of H is NaN."""
    worst = _resid(torch_mod, cc.resid_case(192, mixed))
    print(f"RATIO resid P=192 mixed={int(mixed)}: {worst:.3e}")
    assert worst <= 1.0


def test_resid_p3328(engine, torch_mod):
    """The smallest P (multiple of 64) whose dynamic LDS, 20 B per coordinate, passes 64 KiB."""
    assert 3328 * 20 > 65536 >= 3264 * 20
    worst = _resid(torch_mod, cc.resid_case(3328, False))
    print(f"RATIO resid P=3328: {worst:.3e}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------ minnorm
@pytest.mark.parametrize("name", cc.MINNORM_CASES)
def test_minnorm(engine, torch_mod, name):
    """On the device factor of the P = 192 / 320 factor cases (6 / 9 dependents over the blocks:
    the four-wave loops of the orthogonalisation and the projection wrap; p320 with the intercept
    dependent), three fits through fits = [2, 0, 3], fsrc = [0, 1, 2], the middle one on the ridge
    factor (nd = 0: bitwise unchanged).  Bound 16 max(e_ref, P u max|ref|), see chol64_cases."""
    torch = torch_mod
    from sglm_hip import _lib
    fc, c = cc.factor_case(name), cc.minnorm_case(name)
    P, p, nf = c["P"], c["p"], 3
    t, h = _factor(torch, fc)
    _check_factor(fc, h, name + " (for minnorm)")
    beta = dev(torch, c["beta"])
    fits, fsrc = dev(torch, c["fits"]), dev(torch, c["fsrc"])
    wb = _lib.query("sglm_chol64_minnorm_work_bytes", P, nf)
    work = work_with_guard(torch, wb)
    _lib.call("sglm_chol64_minnorm", ptr(t["U"]), P, p, ptr(t["state"]), ptr(t["nulls"]),
              ptr(t["counts"]), nf, ptr(fits), ptr(fsrc), 3, ptr(beta), ptr(work), 0)
    torch.cuda.synchronize()
    got = beta.cpu().numpy()
    assert guard_intact(work, wb)
    assert np.array_equal(bits(got[1]), bits(c["beta"][1]))              # a row not in fits
    copies = cc._structure(P)[0]
    for q, (fit, f) in enumerate(zip(c["fits"], c["fsrc"])):
        old, new, bound = c["beta"][fit], got[fit], c["bound"][q]
        r = cc.ratio(new, c["ref"][q], bound)
        print(f"RATIO minnorm {name} fit {q}: {r:.3e} (e_ref {c['e_ref'][q]:.2e}, "
              f"floor {c['floor'][q]:.2e})")
        assert r <= 1.0
        st = fc["state"][f]
        assert np.array_equal(bits(new[st >= cc.EXCL]), bits(old[st >= cc.EXCL]))
        if fc["counts"][f][0] == 0:
            assert np.array_equal(bits(new), bits(old))
            continue
        for d, s in copies:
            assert abs(new[d] - new[s]) <= bound, (d, s)
        G = cc.ld(cc.sym_upper(fc["H"][fc["hsrc"][f]]))
        gd = np.abs(G @ (cc.ld(new) - cc.ld(old)))
        rg = cc.err_ratio(gd, bound * np.abs(G).sum(axis=1).astype(np.float64))
        print(f"RATIO minnorm {name} fit {q} fitted values: {rg:.3e}")
        assert rg <= 1.0


# ------------------------------------------------------------------------------ drop sets
@pytest.mark.parametrize("name", cc.DROP_CASES)
def test_drop(engine, torch_mod, name):
    """Three host-built factors at P = 192 (one with two excluded coordinates, one with a
    dependent coordinate: status 2), pg non-identity.  k64: sets of length 0, 64 = kmax, one
    wholly in the last block, one holding an excluded coordinate of its factor, one longer than
    kmax (status 2).  k41: a set of 5 in a table padded with -1 and an index out of range, and
    one of 41.  k1: kmax = 1.  x starts non-zero, the work buffer as NaN; gsrc given and NULL.
    Status 1 (a non-positive pivot of T) needs a non-finite or indefinite factor and is left
    out: it is not to be provoked with non-finite input."""
    torch = torch_mod
    from sglm_hip import _lib
    c = cc.drop_case(name)
    P, kmax, npair, nq, rows = c["P"], c["kmax"], c["npair"], c["nq"], c["rows"]
    assert kmax <= _lib.query("sglm_chol64_drop_kmax")
    t = {k: dev(torch, c[k]) for k in ("U", "state", "counts", "pf", "pg", "sets", "lens", "fits",
                                        "fsrc", "gsrc", "psrc")}
    wb = _lib.query("sglm_chol64_drop_work_bytes", P, npair, kmax)
    work = work_with_guard(torch, wb, fill=float("nan"))
    status = torch.full((npair,), ISENT, dtype=torch.int32, device="cuda")
    _lib.call("sglm_chol64_drop_prep", ptr(t["U"]), P, ptr(t["state"]), ptr(t["counts"]),
              ptr(t["pf"]), ptr(t["pg"]), npair, ptr(t["sets"]), ptr(t["lens"]), kmax, ptr(work),
              ptr(status), 0)
    torch.cuda.synchronize()
    assert np.array_equal(status.cpu().numpy(), c["status"])
    assert guard_intact(work, wb)
    # every status-0 pair's W and factor of T are written in full (the zero rows of W above the
    # set's first block included): only the status-2 pairs' parts keep their NaN
    skipped = int(np.sum(c["status"] == 2))
    assert int(torch.isnan(work[:wb // 8]).sum()) == skipped * (P * kmax + 64 * 64)
    g_rows = c["c"][np.arange(rows) % 3]                 # gsrc = NULL: the fit's own row

    def solve(gs, g):
        x = dev(torch, c["x0"])
        _lib.call("sglm_chol64_drop_solve_add", ptr(t["U"]), P, ptr(t["state"]), ptr(t["fits"]),
                  ptr(t["fsrc"]), ptr(gs), ptr(t["psrc"]), nq, ptr(g), ptr(x), ptr(t["pg"]), npair,
                  ptr(t["sets"]), ptr(t["lens"]), kmax, ptr(work), ptr(status), 0)
        torch.cuda.synchronize()
        return x.cpu().numpy()

    runs = (("gsrc", t["gsrc"], dev(torch, c["c"]), c["gsrc"]),
            ("gsrc=NULL", None, dev(torch, g_rows), c["fits"] % 3))
    for label, gs, g, rhs in runs:
        got, again = solve(gs, g), solve(gs, g)
        assert np.array_equal(bits(got), bits(again))
        other = np.setdiff1d(np.arange(rows), c["fits"])
        assert np.array_equal(bits(got[other]), bits(c["x0"][other]))
        worst = 0.0
        for q, fit in enumerate(c["fits"]):
            if c["expect"][q] is None:
                assert np.array_equal(bits(got[fit]), bits(c["x0"][fit]))
                continue
            keep, ref, bound, _, _, sset = cc.drop_expected(c, q, int(rhs[q]))
            d = cc.ld(got[fit][keep]) - cc.ld(c["x0"][fit][keep])
            worst = max(worst, cc.ratio(d, ref, bound))
            assert np.array_equal(bits(got[fit][sset]), bits(np.zeros(sset.size)))
            rest = np.setdiff1d(np.arange(P), np.r_[keep, sset])
            assert np.array_equal(bits(got[fit][rest]), bits(c["x0"][fit][rest]))
        print(f"RATIO drop {name} {label}: {worst:.3e}")
        assert worst <= 1.0
    assert guard_intact(work, wb)


# ------------------------------------------------------------------------------ P = 8192
def test_solves_and_drop_p8192(engine, torch_mod):
    """The header's limit: the solve kernel asks for exactly 64 KiB of dynamic LDS plus its static
    arrays, the drop solve for 72 KiB.  A dense, diagonally dominant factor with an exact
    rank-one strict upper part (O(P) longdouble references), nq = 1: solve, solve_add, then
    drop_prep + drop_solve_add with one set of two coordinates.  Bounds as at the small sizes."""
    torch = torch_mod
    from sglm_hip import _lib
    c = cc.big_case()
    P, R = c["P"], c["R"]
    U = dev(torch, c["U"][None])
    del c["U"]
    st = torch.zeros((1, P), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    i0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    g = dev(torch, c["g"][None])
    delta = torch.full((1, P), SENT, dtype=torch.float32, device="cuda")
    _lib.call("sglm_chol64_solve", ptr(U), P, ptr(st), ptr(i0), ptr(i0), 1, ptr(g), ptr(delta), 0)
    torch.cuda.synchronize()
    r = R.solve_ratio(-delta.cpu().numpy()[0].astype(np.float64), c["g"], f32=True)
    print(f"RATIO solve P=8192: {r:.3e}")
    assert r <= 1.0
    x = torch.zeros((1, P), dtype=torch.float64, device="cuda")
    _lib.call("sglm_chol64_solve_add", ptr(U), P, ptr(st), ptr(i0), ptr(i0), None, 1, ptr(g),
              ptr(x), 0)
    torch.cuda.synchronize()
    r = R.solve_ratio(x.cpu().numpy()[0], c["g"])
    print(f"RATIO solve_add P=8192: {r:.3e}")
    assert r <= 1.0
    kmax = 2
    sets = dev(torch, c["sset"][None])
    lens = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    wb = _lib.query("sglm_chol64_drop_work_bytes", P, 1, kmax)
    work = work_with_guard(torch, wb, fill=float("nan"))
    status = torch.full((1,), ISENT, dtype=torch.int32, device="cuda")
    _lib.call("sglm_chol64_drop_prep", ptr(U), P, ptr(st), ptr(counts), ptr(i0), ptr(i0), 1,
              ptr(sets), ptr(lens), kmax, ptr(work), ptr(status), 0)
    x = dev(torch, c["x0"][None])
    _lib.call("sglm_chol64_drop_solve_add", ptr(U), P, ptr(st), ptr(i0), ptr(i0), None, ptr(i0), 1,
              ptr(g), ptr(x), ptr(i0), 1, ptr(sets), ptr(lens), kmax, ptr(work), ptr(status), 0)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0]
    assert guard_intact(work, wb)
    got = x.cpu().numpy()[0]
    keep = c["keep"]
    r = cc.ratio(cc.ld(got[keep]) - cc.ld(c["x0"][keep]), c["ref"], c["bound"])
    print(f"RATIO drop P=8192: {r:.3e} (e_ref {c['e_ref']:.2e}, floor {c['floor']:.2e})")
    assert r <= 1.0
    assert np.array_equal(bits(got[c["sset"]]), bits(np.zeros(2)))


# ------------------------------------------------------------------------------ through the engine
def test_engine_ols_intercept_dependent(engine):
    """600 x 20 with a one-hot triple (the intercept is the dependent pivot) and a copied column,
    OLS against the float64 lstsq oracle; the one-hot coefficients' sum is pinned separately."""
    import sglm
    c = cc.engine_case()
    glm = sglm.GLM("Normal", alpha=0)
    glm.fit(c["X"], c["y"])
    w, b = glm_ref.fit_ols(c["X"], c["y"])
    assert rel(glm.coef_, w) < TOL_GAUSS
    assert abs(glm.intercept_ - b) < TOL_GAUSS * max(1.0, abs(b))
    oh = list(c["onehot"])
    assert abs(np.sum(glm.coef_[oh]) - np.sum(w[oh])) < 1e-9
    d, s = c["copy"]
    assert abs(glm.coef_[d] - glm.coef_[s]) < 1e-9


def test_engine_ridge_same_design(engine):
    import sglm
    c = cc.engine_case()
    glm = sglm.GLM("Normal", alpha=0.5, l1_ratio=0)
    glm.fit(c["X"], c["y"])
    w, b = glm_ref.fit_ridge(c["X"], c["y"], 0.5)
    assert rel(glm.coef_, w) < TOL_GAUSS
    assert abs(glm.intercept_ - b) < TOL_GAUSS * max(1.0, abs(b))
