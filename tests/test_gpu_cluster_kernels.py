"""The entry points of csrc/cluster.hip through the C ABI against float64 / np.longdouble numpy
references at the smallest shapes that can break them: sglm_infer_scores (every family, masks
with multiplicities, non-contiguous slots, a tail that is no multiple of 32), sglm_cluster_scores
(n no multiple of 32, one and two column blocks, runs of 1, 31, 32 and 33 rows, runs that end in
mid-word, a run across several tiles and segments, one run over all rows, every row its own run,
three fits of mixed families under two masks, more fits than share a pass) and sglm_cluster_meat
(G no multiple of 4 or of the staged 32, G < 4, the merge of interleaved runs, P = 256 and 512).

The bounds are rounding bounds (u = 2^-53, so 2u = 2^-52):
  scores   |s - s_ref| <= 1e-12 m (|t1| + |t2|), s = t1 - t2 -- the bar of the Pearson sums in
           tests/test_gpu_infer_kernels.py, relative to the terms whose difference s is;
  S        |S - S_ref| <= len_r 2u sum |terms| per run and column (recursive summation);
  M        |M - M_ref| <= (G + 2) 2u sum_c |g_c||g_c|^T entrywise, plus what the error of the
           g_c (the merge's, or S's in the chained test) propagates: sum_c dg_c|g_c|^T +
           |g_c|dg_c^T + dg_c dg_c^T.
Every test prints its worst ratio to the bound (DESIGN.md §30 records them)."""
import numpy as np
import pytest

import chol64_cases as cc
import infer_cases as C
import test_gpu_infer_kernels as IK

pytestmark = pytest.mark.gpu
SENT = cc.SENT
U52 = 2.0 ** -52
SCORE_BAR = 1e-12
bits, dev, ptr = IK.bits, IK.dev, IK.ptr


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


# ------------------------------------------------------------------------------ sglm_infer_scores
def run_scores_rows(torch, fam, power, c, slots, n, ld):
    from sglm_hip import _lib
    eta, Y, M, fr, fm = c
    B = len(slots)
    s = torch.full((B + 1, ld), SENT, dtype=torch.float64, device="cuda")
    d = [dev(torch, a) for a in (np.array(slots, np.int32), eta, Y, M, fr, fm)]   # kept alive
    _lib.call("sglm_infer_scores", fam, float(power), n, ld, B, *map(ptr, d), ptr(s), 0)
    torch.cuda.synchronize()
    sh = s.cpu().numpy()
    assert np.all(sh[B] == SENT)
    return sh[:B]


@pytest.mark.parametrize("name,fam,power", IK.ROW_FAMILIES)
def test_infer_scores(engine, torch_mod, name, fam, power):
    c = IK.rows_case(fam, power)
    eta, Y, M, fr, fm = c
    n, ld = IK.N_ROWS, IK.LD_ROWS
    s = run_scores_rows(torch_mod, fam, power, c, IK.SLOTS, n, ld)
    s2 = run_scores_rows(torch_mod, fam, power, c, IK.SLOTS, n, ld)
    assert np.array_equal(bits(s), bits(s2))
    assert np.all(np.isfinite(s)) and np.all(s[:, n:] == 0)
    kap = float(np.float32(power))
    worst = 0.0
    for q, k in enumerate(IK.SLOTS):
        e64 = eta[k, :n].astype(np.float64)
        y64, m64 = Y[fr[k], :n].astype(np.float64), M[fm[k], :n].astype(np.float64)
        ref = C.ld(m64) * C.score_resid(fam, C.LD(kap), C.ld(y64), C.ld(e64))
        t1, t2 = C.score_terms(fam, kap, y64, e64)
        mag = m64 * (np.abs(t1) + np.abs(t2))
        assert np.all(s[q, :n][m64 == 0] == 0)
        worst = max(worst, cc.err_ratio(np.abs(C.ld(s[q, :n]) - ref), mag))
        # alone (another launch geometry in the fit dimension): the same bits
        one = run_scores_rows(torch_mod, fam, power, c, (k,), n, ld)
        assert np.array_equal(bits(one[0]), bits(s[q]))
    print(f"WORST infer_scores {name}: {worst:.3e} (bar {SCORE_BAR:.0e})")
    assert worst <= SCORE_BAR
    if fam == C.FAM_BINOMIAL:                       # |eta| up to 100: finite, of the right sign
        q = IK.SLOTS.index(4)
        assert np.all(np.abs(s[q, :201]) <= 3.0)


# ------------------------------------------------------------------------------ designs and runs
def make_design(n, P, p, seed):
    """(dense 0/1 X~ [n][P] float64, xbits [P][ld/32] uint32, ld): columns < p at rate 0.06, one
    dense column, one empty column, the ones column at p, zero padding columns and rows."""
    rng = np.random.default_rng([31, seed, n, P])
    ld = (n + 1 + 255) // 256 * 256
    X = np.zeros((P, ld), np.uint8)
    X[:p, :n] = rng.random((p, n)) < 0.06
    X[3, :n] = rng.random(n) < 0.5
    X[7, :] = 0
    X[p, :n] = 1
    words = np.packbits(X.reshape(P, ld // 32, 32), axis=2, bitorder="little")
    xbits = np.ascontiguousarray(words).view("<u4")[:, :, 0].copy()
    assert (xbits[p, 0] & 1) == 1 and xbits.shape == (P, ld // 32)
    return X[:, :n].T.astype(np.float64), xbits, ld


def run_layout(kind, n):
    """roff of the layout: 'mixed' run lengths 1, 31, 32, 33, ... (ends in mid-word, a run of
    1300 rows across tiles and segments), 'one' run over all rows, 'rows' every row its own."""
    if kind == "one":
        return np.array([0, n], np.int32)
    if kind == "rows":
        return np.arange(n + 1, dtype=np.int32)
    lens, pat, i = [], [1, 31, 32, 33, 1, 1, 7, 64, 90, 2, 1300, 3, 513, 40, 1, 29], 0
    while sum(lens) < n:
        L = pat[i % len(pat)]
        lens.append(min(L, 600) if n < 2000 else L)
        i += 1
    roff = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n)
    return np.unique(roff).astype(np.int32)


def mixed_scores(torch, n, ld, seed):
    """s [3][ld] float64 from the device: a Normal, a Poisson and a Binomial fit under two row
    masks with multiplicities 0, 1 and 2 (sglm_infer_scores, checked above)."""
    rng = np.random.default_rng([32, seed, n])
    eta = np.zeros((3, ld), np.float32)
    eta[:, :n] = rng.normal(0, 1.0, (3, n)).astype(np.float32)
    Y = np.zeros((3, ld), np.float32)
    Y[0, :n] = rng.normal(0, 2, n)
    Y[1, :n] = rng.poisson(1.5, n)
    Y[2, :n] = rng.random(n) < 0.4
    M = np.zeros((2, ld), np.uint8)
    M[0, :n] = rng.integers(1, 3, n)
    M[1, :n] = rng.integers(0, 3, n)
    fr, fm = np.array([0, 1, 2], np.int32), np.array([0, 1, 0], np.int32)
    rows = [run_scores_rows(torch, fam, pw, (eta, Y, M, fr, fm), (k,), n, ld)[0]
            for k, (fam, pw) in enumerate([(C.FAM_SQUARED, 0.0), (C.FAM_TWEEDIE, 1.0),
                                           (C.FAM_BINOMIAL, 0.0)])]
    s = np.stack(rows)
    assert np.any(M[1, :n] == 2) and np.any(M[1, :n] == 0) and np.all(s[:, n:] == 0)
    return s


def cluster_scores(torch, xbits, ld, P, n, s, roff):
    from sglm_hip import _lib
    B, R = s.shape[0], len(roff) - 1
    S = torch.full((B * R * P + 512,), SENT, dtype=torch.float64, device="cuda")
    d = [dev(torch, a) for a in (xbits, s, roff)]
    _lib.call("sglm_cluster_scores", ptr(d[0]), ld, P, n, ptr(d[1]), B, ptr(d[2]), R, ptr(S), 0)
    torch.cuda.synchronize()
    Sh = S.cpu().numpy()
    assert np.all(Sh[B * R * P:] == SENT)
    return Sh[:B * R * P].reshape(B, R, P)


def scores_reference(X, s, roff):
    """(S_ref, bound) [R][P] in longdouble / float64 of one fit: sums of X[i][j] s[i] over the runs."""
    n = X.shape[0]
    T = C.ld(X) * C.ld(s[:n])[:, None]
    ref = np.add.reduceat(T, roff[:-1], axis=0)
    mag = np.add.reduceat(np.abs(T), roff[:-1], axis=0)
    return ref, (np.diff(roff)[:, None] * U52 * mag).astype(np.float64)


@pytest.mark.parametrize("kind", ["mixed", "one", "rows"])
@pytest.mark.parametrize("n,P,p", [(1000, 256, 250), (4099, 512, 500)])
def test_cluster_scores(engine, torch_mod, n, P, p, kind):
    X, xbits, ld = make_design(n, P, p, 1)
    roff = run_layout(kind, n)
    R = len(roff) - 1
    if kind == "mixed":
        lens = set(np.diff(roff).tolist())
        assert {1, 31, 32, 33} <= lens and max(lens) >= 600 and np.any(roff[1:-1] % 32 != 0)
    s = mixed_scores(torch_mod, n, ld, 1)
    S = cluster_scores(torch_mod, xbits, ld, P, n, s, roff)
    assert np.array_equal(bits(S), bits(cluster_scores(torch_mod, xbits, ld, P, n, s, roff)))
    worst = 0.0
    for q in range(3):
        ref, bound = scores_reference(X, s[q], roff)
        worst = max(worst, cc.ratio(S[q], ref, bound))
        assert np.all(S[q][:, 7] == 0) and np.all(S[q][:, p + 1:] == 0)
        one = cluster_scores(torch_mod, xbits, ld, P, n, s[q:q + 1], roff)
        assert np.array_equal(bits(one[0]), bits(S[q]))          # alone: the same bits
    if kind == "rows":                                           # one term per sum: exact
        assert np.array_equal(S[1], X * s[1, :n][:, None])
    # the ones column: the run sums of s
    assert cc.ratio(S[0][:, p], np.add.reduceat(C.ld(s[0, :n]), roff[:-1]),
                    np.diff(roff) * U52 * np.add.reduceat(np.abs(s[0, :n]), roff[:-1])) <= 1.0
    print(f"RATIO cluster_scores n={n} P={P} {kind} R={R}: {worst:.3e}")
    assert worst <= 1.0


def test_cluster_scores_more_fits_than_share_a_pass(engine, torch_mod):
    """Seven fits (two passes over the planes): each equals its single launch bit for bit; runs
    that cover only rows 5 .. 900 leave the other rows unread."""
    n, P, p = 1000, 256, 250
    X, xbits, ld = make_design(n, P, p, 2)
    s3 = mixed_scores(torch_mod, n, ld, 2)
    s = np.concatenate([s3, s3[::-1], s3[1:2]])
    roff = np.array([5, 6, 37, 500, 533, 900], np.int32)
    S = cluster_scores(torch_mod, xbits, ld, P, n, s, roff)
    S3 = cluster_scores(torch_mod, xbits, ld, P, n, s3, roff)
    for q, src in enumerate([0, 1, 2, 2, 1, 0, 1]):
        assert np.array_equal(bits(S[q]), bits(S3[src]))
    Xz = X.copy()
    Xz[:5] = 0
    Xz[900:] = 0
    ref, bound = scores_reference(Xz, s3[0], np.array([0, 6, 37, 500, 533, 1000]))
    assert cc.ratio(S3[0], ref, bound) <= 1.0


def test_cluster_scores_refuses_bad_runs(engine, torch_mod):
    from sglm_hip import _lib
    n, P, p = 1000, 256, 250
    X, xbits, ld = make_design(n, P, p, 2)
    s = np.zeros((1, ld))
    for roff in ([0, 10, 10, 1000], [0, 500, 400, 1000], [0, 500, 1001], [-1, 500, 1000]):
        with pytest.raises(_lib.HipEngineError, match="run"):
            cluster_scores(torch_mod, xbits, ld, P, n, s, np.array(roff, np.int32))


# ------------------------------------------------------------------------------ sglm_cluster_meat
def cluster_meat(torch, S, coff, cruns, G):
    from sglm_hip import _lib
    B, R, P = S.shape
    Mo = torch.full((B * P * P + 512,), SENT, dtype=torch.float64, device="cuda")
    wb = _lib.query("sglm_cluster_meat_work_bytes", P, B, G)
    assert wb == B * G * P * 8
    work = torch.full((wb // 8 + 512,), SENT, dtype=torch.float64, device="cuda") \
        if coff is not None else None
    d = [dev(torch, a) for a in (S, coff, cruns)]
    _lib.call("sglm_cluster_meat", ptr(d[0]), P, B, R, ptr(d[1]), ptr(d[2]), G, ptr(Mo),
              ptr(work), 0)
    torch.cuda.synchronize()
    Mh = Mo.cpu().numpy()
    assert np.all(Mh[B * P * P:] == SENT)
    if work is not None:
        assert np.all(work[wb // 8:].cpu().numpy() == SENT)
    return Mh[:B * P * P].reshape(B, P, P)


def meat_reference(S, dS, rc, G):
    """(M_ref longdouble, entrywise bound) of one fit from its run scores S [R][P] (error bound dS,
    or None when S is the kernel's exact input) and the cluster rc[r] of every run."""
    R, P = S.shape
    g, mag, dg = np.zeros((G, P), C.LD), np.zeros((G, P), C.LD), np.zeros((G, P), C.LD)
    np.add.at(g, rc, C.ld(S))
    np.add.at(mag, rc, np.abs(C.ld(S)))
    if dS is not None:
        np.add.at(dg, rc, C.ld(dS))
    dg += (np.bincount(rc, minlength=G)[:, None] * U52) * mag * (R != G)      # the merge's sums
    ag = np.abs(g)
    bound = (G + 2) * U52 * (ag.T @ ag) + dg.T @ ag + ag.T @ dg + dg.T @ dg
    return g.T @ g, bound.astype(np.float64)


def check_meat(torch, S, dS, rc, G, label):
    B, R, P = S.shape
    coff = cruns = None
    if R != G:
        cruns = np.argsort(rc, kind="stable").astype(np.int32)
        coff = np.r_[0, np.cumsum(np.bincount(rc, minlength=G))].astype(np.int32)
    M = cluster_meat(torch, S, coff, cruns, G)
    assert np.array_equal(bits(M), bits(cluster_meat(torch, S, coff, cruns, G)))
    worst = 0.0
    for q in range(B):
        ref, bound = meat_reference(S[q], None if dS is None else dS[q], rc, G)
        worst = max(worst, cc.ratio(M[q], ref, bound))
        assert np.array_equal(bits(M[q]), bits(M[q].T.copy()))               # bitwise symmetric
        one = cluster_meat(torch, S[q:q + 1], coff, cruns, G)
        assert np.array_equal(bits(one[0]), bits(M[q]))                      # alone: the same bits
    print(f"RATIO cluster_meat {label} P={P} R={R} G={G}: {worst:.3e}")
    assert worst <= 1.0
    return M


@pytest.mark.parametrize("P,R,G", [(256, 37, 37), (512, 130, 130), (256, 3, 3), (256, 1000, 37),
                                   (512, 301, 130)])
def test_cluster_meat(engine, torch_mod, P, R, G):
    rng = np.random.default_rng([33, P, R, G])
    S = rng.normal(0, 1, (3, R, P)) * (rng.random((3, R, P)) < 0.4)
    S[:, :, 9] = 0.0
    S[1] *= 1e3
    rc = np.arange(R) % G
    if R != G:                      # interleaved, and unequal numbers of runs per cluster
        rc[R // 2:] = rng.integers(0, G, R - R // 2)
        assert len(np.unique(rc)) == G
    M = check_meat(torch_mod, S, None, rc, G, "interleaved" if R != G else "single runs")
    assert np.all(M[:, 9, :] == 0) and np.all(M[:, :, 9] == 0)
    # an asymmetric probe of the MFMA maps: one cluster e_a + 2 e_b gives exactly the 2 x 2 block
    Sp = np.zeros((1, G, P))
    Sp[0, G - 1, 17], Sp[0, G - 1, 200] = 1.0, 2.0
    Mp = cluster_meat(torch_mod, Sp, None, None, G)[0]
    want = np.zeros((P, P))
    want[17, 17], want[17, 200], want[200, 17], want[200, 200] = 1.0, 2.0, 2.0, 4.0
    assert np.array_equal(Mp, want)


@pytest.mark.parametrize("kind", ["trials", "interleaved"])
def test_scores_then_meat_against_the_rows(engine, torch_mod, kind):
    """The chain on n = 1000: M against the longdouble sum_c g_c g_c^T formed from the rows, the
    bound carrying the run sums' own rounding."""
    n, P, p, G = 1000, 256, 250, 41
    X, xbits, ld = make_design(n, P, p, 3)
    s = mixed_scores(torch_mod, n, ld, 3)
    if kind == "trials":
        roff = np.unique(np.r_[0, np.sort(np.random.default_rng(5).choice(
            np.arange(1, n), G - 1, replace=False)), n]).astype(np.int32)
        rc = np.arange(G)
    else:
        roff, rc = np.arange(n + 1, dtype=np.int32), np.arange(n) % G
    S = cluster_scores(torch_mod, xbits, ld, P, n, s, roff)
    refs = [scores_reference(X, s[q], roff) for q in range(3)]
    Sref = np.stack([r[0] for r in refs])
    dS = np.stack([r[1] for r in refs])
    from sglm_hip import _lib
    coff = cruns = None
    if kind != "trials":
        cruns = np.argsort(rc, kind="stable").astype(np.int32)
        coff = np.r_[0, np.cumsum(np.bincount(rc, minlength=G))].astype(np.int32)
    M = cluster_meat(torch_mod, S, coff, cruns, G)
    worst = 0.0
    for q in range(3):
        ref, bound = meat_reference(Sref[q], dS[q], rc, G)
        # the same matrix straight from the rows
        cid = np.repeat(rc, np.diff(roff))
        g = np.zeros((G, P), C.LD)
        np.add.at(g, cid, C.ld(X) * C.ld(s[q, :n])[:, None])
        assert np.max(np.abs(g.T @ g - ref)) <= 1e-15 * np.max(np.abs(ref))
        worst = max(worst, cc.ratio(M[q], ref, bound))
    print(f"RATIO scores -> meat {kind}: {worst:.3e}")
    assert worst <= 1.0
