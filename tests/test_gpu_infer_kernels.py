"""The three entry points of csrc/infer.hip through the C ABI against float64 / np.longdouble
references (tests/infer_cases.py): sglm_infer_rows (every family, both modes, a tail that is no
multiple of 4 or 32, masks with multiplicities 0..3, non-contiguous slots), sglm_chol64_inverse
(one tile, the first off-diagonal tile, an interior accumulation; excluded, zero and dependent
coordinates at tile edges; NaN below the diagonal of U) and sglm_cov_groups (groups of 1, 41 and
the cap, a non-contiguous group, an over-cap group, every cov_type, lam = 0 and > 0).  Every test
prints its worst figure (DESIGN.md §28 records them next to the bars)."""
import numpy as np
import pytest

import chol64_cases as cc
import infer_cases as C

pytestmark = pytest.mark.gpu
SENT = cc.SENT

# f32 weight against the float64 weight at the same f32 eta.  Measured worst relative distance
# on the MI355X over the cases below: mode 0 (m v) 2.773e-7 (binomial), mode 1 (m s^2, relative
# to m (|t1| + |t2|)^2 with s = t1 - t2) 3.201e-7 (NB2, kappa = 1) -- a few ulp (2^-24 = 6e-8) of
# expf and the divisions after it.  The bars are 4 x those.
ROWS_BAR = {0: 4 * 2.773e-7, 1: 4 * 3.201e-7}
TINY = 2.0 ** -100                       # weights below it are written as 0

ROW_FAMILIES = [("normal", C.FAM_SQUARED, 0.0), ("poisson", C.FAM_TWEEDIE, 1.0),
                ("gamma", C.FAM_TWEEDIE, 2.0), ("tweedie15", C.FAM_TWEEDIE, 1.5),
                ("binomial", C.FAM_BINOMIAL, 0.0), ("nb2_tiny", C.FAM_NB2, 2.0 ** -20),
                ("nb2_one", C.FAM_NB2, 1.0)]
N_ROWS, LD_ROWS, SLOTS = 2001, 2048, (4, 1, 6)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


# ------------------------------------------------------------------------------ sglm_infer_rows
def rows_case(fam, power):
    rng = np.random.default_rng([77, fam, int(power * 8)])
    n, ld = N_ROWS, LD_ROWS
    eta = np.zeros((8, ld), np.float32)
    eta[:, :n] = rng.normal(0, 1.5, (8, n)).astype(np.float32)
    if fam == C.FAM_BINOMIAL:                       # |eta| up to 100 on one slot
        eta[4, :201] = np.linspace(-100, 100, 201).astype(np.float32)
    Y = np.zeros((2, ld), np.float32)
    for r in range(2):
        if fam == C.FAM_SQUARED:
            Y[r, :n] = rng.normal(0, 2, n)
        elif fam == C.FAM_BINOMIAL:
            Y[r, :n] = rng.random(n) < 0.4
        elif fam == C.FAM_TWEEDIE and power != 1.0:
            Y[r, :n] = rng.gamma(2.0, 1.0, n)
        else:
            Y[r, :n] = rng.poisson(1.5, n)
    M = np.zeros((2, ld), np.uint8)
    M[0, :n] = rng.integers(0, 4, n)
    M[1, :n] = rng.integers(0, 4, n) * (rng.random(n) < 0.7)
    fit_resp = np.array([0, 1, 0, 0, 1, 0, 0, 1], np.int32)
    fit_mask = np.array([0, 0, 0, 0, 1, 0, 1, 0], np.int32)
    return eta, Y, M, fit_resp, fit_mask


def run_rows(torch, fam, power, mode, c, sums=True):
    from sglm_hip import _lib
    eta, Y, M, fr, fm = c
    B = len(SLOTS)
    Wp = torch.full((3 * B + 1, LD_ROWS), SENT, dtype=torch.float32, device="cuda")
    S = torch.full((B + 1, 2), SENT, dtype=torch.float64, device="cuda") if sums else None
    wb = _lib.query("sglm_infer_rows_work_bytes", B, LD_ROWS)
    work = torch.full((wb // 8 + 8,), SENT, dtype=torch.float64, device="cuda")
    d = [dev(torch, a) for a in (np.array(SLOTS, np.int32), eta, Y, M, fr, fm)]   # kept alive
    _lib.call("sglm_infer_rows", fam, float(power), mode, N_ROWS, LD_ROWS, B, *map(ptr, d),
              ptr(Wp), ptr(S), ptr(work) if sums else None, 0)
    torch.cuda.synchronize()
    Wh = Wp.cpu().numpy()
    assert np.all(Wh[3 * B] == np.float32(SENT)) and np.all(work[wb // 8:].cpu().numpy() == SENT)
    Sh = None
    if sums:
        Sh = S.cpu().numpy()
        assert np.all(Sh[B] == SENT)
    return Wh[:3 * B].reshape(3, B, LD_ROWS), None if Sh is None else Sh[:B]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,fam,power", ROW_FAMILIES)
def test_infer_rows(engine, torch_mod, name, fam, power, mode):
    c = rows_case(fam, power)
    eta, Y, M, fr, fm = c
    n = N_ROWS
    Wp, S = run_rows(torch_mod, fam, power, mode, c)
    Wp2, S2 = run_rows(torch_mod, fam, power, mode, c)
    assert np.array_equal(bits(Wp), bits(Wp2)) and np.array_equal(bits(S), bits(S2))
    assert np.all(Wp >= 0) and np.all(np.isfinite(Wp))
    assert np.all(bits(Wp) & 0xFFFF == 0)                       # every piece is a bf16 value
    assert np.all(Wp[:, :, n:] == 0)
    w = (Wp[0] + Wp[1]) + Wp[2]                                 # f32 sums, exact by construction
    assert w.dtype == np.float32
    assert np.array_equal(Wp[0].astype(np.float64) + Wp[1] + Wp[2], w.astype(np.float64))
    worst = 0.0
    kap = float(np.float32(power))
    for q, k in enumerate(SLOTS):
        e64 = eta[k, :n].astype(np.float64)
        y64, m64 = Y[fr[k], :n].astype(np.float64), M[fm[k], :n].astype(np.float64)
        mu, v, V = C.mean_weight_var(fam, kap, e64)
        if mode == 0:
            ref = m64 * v
            mag = ref
        else:
            s = C.score_resid(fam, kap, y64, e64)
            t1, t2 = C.score_terms(fam, kap, y64, e64)
            ref = m64 * s * s
            mag = m64 * (np.abs(t1) + np.abs(t2)) ** 2
        got = w[q, :n].astype(np.float64)
        assert np.all(got[m64 == 0] == 0)
        assert np.all(got[ref < TINY / 2] == 0)                 # flushed, never NaN
        big = ref >= 2 * TINY
        worst = max(worst, float(np.max(np.abs(got[big] - ref[big]) / mag[big])))
        # the Pearson sums against longdouble
        terms = C.ld(m64) * (C.ld(y64) - C.ld(mu)) ** 2 / C.ld(V)
        assert abs(C.LD(S[q, 0]) - terms.sum()) <= 1e-12 * float(np.abs(terms).sum())
        assert S[q, 1] == m64.sum()
    print(f"WORST infer_rows {name} mode {mode}: {worst:.3e} (bar {ROWS_BAR[mode]:.3e})")
    assert worst <= ROWS_BAR[mode]
    if fam == C.FAM_BINOMIAL and mode == 0:
        q = SLOTS.index(4)
        ext = np.abs(eta[4, :201]) >= 90
        assert ext.sum() >= 20 and np.all(w[q, :201][ext] == 0)


def test_infer_rows_without_sums(engine, torch_mod):
    c = rows_case(C.FAM_TWEEDIE, 1.0)
    a, _ = run_rows(torch_mod, C.FAM_TWEEDIE, 1.0, 0, c, sums=True)
    b, s = run_rows(torch_mod, C.FAM_TWEEDIE, 1.0, 0, c, sums=False)
    assert s is None and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------ sglm_chol64_inverse
def inverse_case(P):
    rng = np.random.default_rng([55, P])
    edge = sorted({0, 63, 64, P - 1} & set(range(P)))
    U0, s0, _ = cc.host_factor(rng, P, excl=edge[0::2], zero=edge[1::2])
    U1, s1, _ = cc.host_factor(rng, P, dep=(5, P - 2))
    return np.stack([U0, U1]), np.stack([s0, s1])


@pytest.mark.parametrize("P", [64, 128, 192])
def test_chol64_inverse(engine, torch_mod, P):
    from sglm_hip import _lib
    torch = torch_mod
    U, state = inverse_case(P)
    assert np.isnan(U[0][P - 1, 0])                              # garbage below the diagonal
    nf = 2
    Ud, sd = dev(torch, U), dev(torch, state)
    A = torch.full((nf * P * P + 512,), SENT, dtype=torch.float64, device="cuda")
    wb = _lib.query("sglm_chol64_inverse_work_bytes", P, nf)
    assert wb == nf * P * P * 8
    work = torch.full((wb // 8 + 512,), SENT, dtype=torch.float64, device="cuda")
    _lib.call("sglm_chol64_inverse", ptr(Ud), P, ptr(sd), nf, ptr(A), ptr(work), 0)
    torch.cuda.synchronize()
    Ah = A.cpu().numpy()
    assert np.all(Ah[nf * P * P:] == SENT) and np.all(work[wb // 8:].cpu().numpy() == SENT)
    Ah = Ah[:nf * P * P].reshape(nf, P, P)
    # the same matrix by sglm_chol64_solve_add on identity columns
    X = torch.zeros((nf * P, P), dtype=torch.float64, device="cuda")
    g = torch.eye(P, dtype=torch.float64, device="cuda")
    fits = torch.arange(nf * P, dtype=torch.int32, device="cuda")
    fsrc = torch.arange(nf, dtype=torch.int32, device="cuda").repeat_interleave(P).contiguous()
    gsrc = torch.arange(P, dtype=torch.int32, device="cuda").repeat(nf).contiguous()
    _lib.call("sglm_chol64_solve_add", ptr(Ud), P, ptr(sd), ptr(fits), ptr(fsrc), ptr(gsrc),
              nf * P, ptr(g), ptr(X), 0)
    torch.cuda.synchronize()
    Xh = X.cpu().numpy().reshape(nf, P, P)
    worst = cross = 0.0
    for f in range(nf):
        ref, bound = C.inverse_bound(U[f], state[f])
        off = state[f] != C.KEPT
        assert np.all(bits(Ah[f][off, :]) == 0) and np.all(bits(Ah[f][:, off]) == 0)
        assert np.array_equal(bits(Ah[f]), bits(Ah[f].T.copy()))
        worst = max(worst, cc.ratio(Ah[f], ref, bound))
        K = np.flatnonzero(~off)
        cross = max(cross, cc.err_ratio(np.abs(Ah[f] - Xh[f])[np.ix_(K, K)],
                                        2 * bound[np.ix_(K, K)]))
    print(f"RATIO chol64_inverse P={P}: {worst:.3e}  (vs solve_add columns: {cross:.3e})")
    assert worst <= 1.0 and cross <= 1.0


# ------------------------------------------------------------------------------ sglm_cov_groups
COV_P, COV_p = 192, 180
COV_ZERO = 20                            # a column of the 41-group that one factor marks zero


def cov_groups_layout():
    """Groups over the 180 coefficients: one column, 41 columns, the cap (64), 65 (over the cap)
    and a non-contiguous group of 9 (every other column of the rest plus column 0's neighbour)."""
    ids = np.empty(COV_p, np.int64)
    ids[0] = 0
    ids[1:42] = 1
    ids[42:106] = 2
    ids[106:171] = 3
    ids[171:180] = 4
    ids[[172, 174, 176, 178]] = 5                                # groups 4 and 5 interleave
    return ids


def cov_case():
    rng = np.random.default_rng(4242)
    P, p = COV_P, COV_p
    K = np.arange(p + 1)
    J = cc._spd(rng, p + 1) * 50.0
    lams = np.array([0.0, 3.5, 3.5])
    Ainv = np.zeros((3, P, P))
    state = np.full((3, P), C.EXCL, np.uint8)
    for f in range(3):
        A = J + np.diag(np.r_[np.full(p, lams[f]), 0.0])
        Ainv[f] = C.embed(C.ld_inv(A).astype(np.float64), K, P)
        state[f, K] = C.KEPT
    # fit 2: fit 1's inverse with one coordinate's row and column zeroed and marked a zero column
    Ainv[2][COV_ZERO, :] = 0.0
    Ainv[2][:, COV_ZERO] = 0.0
    state[2, COV_ZERO] = C.ZERO
    M = np.zeros((3, P, P))
    Mk = cc._spd(rng, p + 1) * 30.0
    for f in range(3):
        M[f][np.ix_(K, K)] = Mk
    beta = np.zeros((3, P))
    beta[:, :p + 1] = rng.normal(0, 0.2, (1, p + 1))
    scale = np.array([0.7, 1.3, 1.3])
    return Ainv, state, M, lams, scale, beta


@pytest.mark.parametrize("cov_type", ["model", "bayes", "robust"])
def test_cov_groups(engine, torch_mod, cov_type):
    from sglm_hip import _lib
    torch = torch_mod
    P, p = COV_P, COV_p
    Ainv, state, M, lams, scale, beta = cov_case()
    ids = cov_groups_layout()
    gid, goff, gcols = C.csr(ids)
    ng, nfit = len(gid), 3
    ct = {"model": 0, "bayes": 1, "robust": 2}[cov_type]
    kmax = _lib.query("sglm_cov_groups_kmax")
    assert kmax == 64 and np.diff(goff).tolist() == [1, 41, 64, 65, 5, 4]

    def run(want_cov):
        var = torch.full((nfit + 1, P), SENT, dtype=torch.float64, device="cuda")
        stat = torch.full((nfit + 1, ng), SENT, dtype=torch.float64, device="cuda")
        dof = torch.full((nfit + 1, ng), cc.ISENT, dtype=torch.int32, device="cuda")
        status = torch.full((nfit + 1, ng), cc.ISENT, dtype=torch.int32, device="cuda")
        cov = torch.full((nfit * P * P + 512,), SENT, dtype=torch.float64, device="cuda") \
            if want_cov else None
        d = {k: dev(torch, a) for k, a in dict(A=Ainv, st=state, M=M if ct == 2 else None,
                                               lam=lams, sc=scale, b=beta, go=goff,
                                               gc=gcols).items()}      # kept alive
        _lib.call("sglm_cov_groups", ptr(d["A"]), P, p, None, ptr(d["st"]), ptr(d["M"]), ct, nfit,
                  ptr(d["lam"]), ptr(d["sc"]), ptr(d["b"]), ptr(d["go"]), ptr(d["gc"]), ng,
                  ptr(var), ptr(stat), ptr(dof), ptr(status), ptr(cov), 0)
        torch.cuda.synchronize()
        out = [t.cpu().numpy() for t in (var, stat, dof, status)]
        assert np.all(out[0][nfit] == SENT) and np.all(out[1][nfit] == SENT)
        assert np.all(out[2][nfit] == cc.ISENT) and np.all(out[3][nfit] == cc.ISENT)
        ch = None
        if want_cov:
            ch = cov.cpu().numpy()
            assert np.all(ch[nfit * P * P:] == SENT)
            ch = ch[:nfit * P * P].reshape(nfit, P, P)
        return [o[:nfit] for o in out] + [ch]

    var, stat, dof, status, cov = run(True)
    var2, stat2, dof2, status2, _ = run(False)
    assert np.array_equal(bits(var), bits(var2)) and np.array_equal(bits(stat), bits(stat2))
    assert np.array_equal(dof, dof2) and np.array_equal(status, status2)
    wv = ws = wc = 0.0
    for f in range(nfit):
        kept = np.flatnonzero(state[f] == C.KEPT)
        Cf, Ef, _, _ = C.cov_block_bounds(Ainv[f], M[f], lams[f], scale[f], p, cov_type, kept,
                                          beta[f][kept])
        wv = max(wv, cc.ratio(var[f][kept], np.diag(Cf), np.diag(Ef)))
        assert np.all(var[f][state[f] != C.KEPT] == 0)
        wc = max(wc, cc.ratio(cov[f][np.ix_(kept, kept)], Cf, Ef))
        assert np.array_equal(bits(cov[f]), bits(cov[f].T.copy()))
        off = state[f] != C.KEPT
        assert np.all(cov[f][off, :] == 0) and np.all(cov[f][:, off] == 0)
        assert np.array_equal(bits(np.diag(cov[f])), bits(var[f]))
        for g in range(ng):
            cols = gcols[goff[g]:goff[g + 1]]
            ck = cols[state[f][cols] == C.KEPT]
            assert dof[f, g] == ck.size
            if cols.size > kmax:
                assert np.isnan(stat[f, g]) and status[f, g] == 2
                continue
            _, _, sref, sb = C.cov_block_bounds(Ainv[f], M[f], lams[f], scale[f], p, cov_type, ck,
                                                beta[f][ck])
            assert status[f, g] == 0
            ws = max(ws, abs(stat[f, g] - sref) / sb)
    # the zero column: the 41-group of fit 2 has 40 degrees of freedom, the others keep theirs
    assert dof[1].tolist() == [1, 41, 64, 65, 5, 4] and dof[2].tolist() == [1, 40, 64, 65, 5, 4]
    if cov_type == "bayes":                  # no sum runs over the zeroed coordinate: same bits
        others = [0, 2, 4, 5]
        assert np.array_equal(bits(stat[1][others]), bits(stat[2][others]))
    print(f"RATIO cov_groups {cov_type}: var {wv:.3e} cov {wc:.3e} stat {ws:.3e}")
    assert wv <= 1.0 and wc <= 1.0 and ws <= 1.0


def test_cov_groups_non_positive_pivot(engine, torch_mod):
    """A block that is not positive definite reports status 1 and NaN (here: -A^-1 as input)."""
    from sglm_hip import _lib
    torch = torch_mod
    P, p = COV_P, COV_p
    Ainv, state, M, lams, scale, beta = cov_case()
    gid, goff, gcols = C.csr(cov_groups_layout())
    ng = len(gid)
    var = torch.zeros((1, P), dtype=torch.float64, device="cuda")
    stat = torch.zeros((1, ng), dtype=torch.float64, device="cuda")
    dof = torch.zeros((1, ng), dtype=torch.int32, device="cuda")
    status = torch.zeros((1, ng), dtype=torch.int32, device="cuda")
    d = [dev(torch, a) for a in (-Ainv[:1], state[:1], scale[:1], beta[:1], goff, gcols)]
    _lib.call("sglm_cov_groups", ptr(d[0]), P, p, None, ptr(d[1]), None, 1, 1, None, ptr(d[2]),
              ptr(d[3]), ptr(d[4]), ptr(d[5]), ng, ptr(var), ptr(stat), ptr(dof), ptr(status),
              None, 0)
    torch.cuda.synchronize()
    assert status.cpu().numpy()[0].tolist() == [1, 1, 1, 2, 1, 1]
    assert np.all(np.isnan(stat.cpu().numpy()))
