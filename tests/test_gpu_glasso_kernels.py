"""sglm_group_bound / sglm_group_cd_shared on float64 Q and q built in numpy, against the numpy
block-descent oracle of glasso_cases (no other HIP route is involved).

Bars: coefficients within 1e-5 relative max-norm of the oracle (the project's Gaussian bar; the
measured distances are printed and sit many orders below it), zero groups identical and exact
0.0, float64 KKT violation relative to lam_g below 1e-6 (the bar of test_gpu_c5), a second
call bitwise equal, gamma >= lambda_max(Q_gg) by eigvalsh."""
import numpy as np
import pytest

import glasso_cases as C

pytestmark = pytest.mark.gpu

TOL = 1e-10
MAX_SWEEPS = 10000
COEF_BAR = 1e-5
KKT_BAR = 1e-6


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()    # a writable copy


def bound(engine, Qs, goff, gcols):
    """gamma [nq][ng] (host) of the stacked Q [nq][p][p]."""
    import torch
    from sglm_hip import _lib
    nq, p = Qs.shape[0], Qs.shape[1]
    ng = len(goff) - 1
    Qd, go, gc = _dev(Qs, np.float64), _dev(goff, np.int32), _dev(gcols, np.int32)
    gam = torch.empty((nq, ng), dtype=torch.float64, device="cuda")
    _lib.call("sglm_group_bound", Qd.data_ptr(), p, nq, go.data_ptr(), gc.data_ptr(), ng,
              gam.data_ptr(), engine._stream())
    return gam.cpu().numpy()


def descend(engine, Qs, qidx, q, goff, gcols, lam_scale, l2, calls=1):
    """(w [nfit][p], sweeps [nfit]) per call of sglm_group_cd_shared on host arrays."""
    import torch
    from sglm_hip import _lib
    nq, p = Qs.shape[0], Qs.shape[1]
    ng, nfit = len(goff) - 1, len(qidx)
    Qd, go, gc = _dev(Qs, np.float64), _dev(goff, np.int32), _dev(gcols, np.int32)
    gam = torch.empty((nq, ng), dtype=torch.float64, device="cuda")
    _lib.call("sglm_group_bound", Qd.data_ptr(), p, nq, go.data_ptr(), gc.data_ptr(), ng,
              gam.data_ptr(), engine._stream())
    qi, qd = _dev(qidx, np.int32), _dev(q, np.float64)
    ls, l2d = _dev(lam_scale, np.float64), _dev(l2, np.float64)
    out = []
    for _ in range(calls):
        w = torch.full((nfit, p), np.nan, dtype=torch.float64, device="cuda")
        sw = torch.full((nfit,), -1, dtype=torch.int32, device="cuda")
        _lib.call("sglm_group_cd_shared", Qd.data_ptr(), p, qi.data_ptr(), nfit, qd.data_ptr(),
                  go.data_ptr(), gc.data_ptr(), ng, gam.data_ptr(), ls.data_ptr(),
                  l2d.data_ptr(), MAX_SWEEPS, TOL, w.data_ptr(), sw.data_ptr(), engine._stream())
        out.append((w.cpu().numpy(), sw.cpu().numpy()))
    return out


def check_fit(tag, Q, q, ls, l2, goff, gcols, w, sw, w_ref):
    """The per-fit assertions; returns (distance, KKT violation)."""
    assert np.all(np.isfinite(w)), tag
    assert 1 <= sw < MAX_SWEEPS, (tag, sw)
    scale = float(np.max(np.abs(w_ref)))
    dist = float(np.max(np.abs(w - w_ref))) / scale if scale else float(np.max(np.abs(w)))
    viol = C.kkt(Q, q, ls, l2, goff, gcols, w)
    zk, zr = C.zero_groups(w, goff, gcols), C.zero_groups(w_ref, goff, gcols)
    print(f"{tag}: sweeps {sw}, |w - oracle| / |oracle| {dist:.2e}, KKT {viol:.2e}, "
          f"zero groups {int(zk.sum())}/{zk.size}")
    assert dist <= COEF_BAR, (tag, dist)
    assert np.array_equal(zk, zr), (tag, zk, zr)
    for g in np.flatnonzero(zr):                     # exact 0.0 (not -0.0 either)
        c = gcols[goff[g]:goff[g + 1]]
        assert np.all(w[c] == 0.0) and not np.any(np.signbit(w[c])), (tag, g)
    assert viol <= KKT_BAR, (tag, viol)
    return dist, viol


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_against_the_oracle(engine, name):
    """Every case (p = 30 6x5; 96 8x12; 257 with sizes {1, 3, 40, 64, 70, 79}, two groups
    interleaved; 640 with a 300-wide group, wider than the 256-thread workgroup): seven fits of
    one Q -- alphas x {l2 = 0, l2 > 0} and an alpha at which every group is zero."""
    Q, q, xm, ym, n, goff, gcols = C.gram(name)
    pen = [(a, rho) for rho in C.RHOS for a in C.ALPHAS] + [(C.ALPHA_ALL_ZERO, 1.0)]
    ls = np.array([a * rho * n for a, rho in pen])
    l2 = np.array([a * (1 - rho) * n for a, rho in pen])
    gam = bound(engine, Q[None], goff, gcols)[0]
    for g in range(len(goff) - 1):
        c = gcols[goff[g]:goff[g + 1]]
        lmax = float(np.linalg.eigvalsh(Q[np.ix_(c, c)])[-1])
        print(f"{name} group {g} (k = {len(c)}): gamma / lambda_max = {gam[g] / lmax:.3f}")
        assert gam[g] >= lmax, (name, g, gam[g], lmax)
    (w, sw), (w2, sw2) = descend(engine, Q[None], np.zeros(len(pen), np.int32),
                                 np.tile(q, (len(pen), 1)), goff, gcols, ls, l2, calls=2)
    assert np.array_equal(w.view(np.uint64), w2.view(np.uint64)) and np.array_equal(sw, sw2)
    for f, (a, rho) in enumerate(pen):
        check_fit(f"{name} alpha={a} rho={rho}", Q, q, ls[f], l2[f], goff, gcols, w[f],
                  int(sw[f]), C.solution(name, a, rho)[0])
    assert sw[-1] == 1 and np.all(w[-1] == 0.0)          # every group zero: one sweep


def test_singleton_groups(engine):
    """Every column its own group: the ElasticNet objective (oracle with singleton groups)."""
    name = "8x12"
    Q, q, xm, ym, n, _, _ = C.gram(name)
    p = Q.shape[0]
    goff, gcols = C.csr(np.arange(p))
    pen = [(a, rho) for rho in C.RHOS for a in C.ALPHAS]
    ls = np.array([a * rho * n for a, rho in pen])
    l2 = np.array([a * (1 - rho) * n for a, rho in pen])
    gam = bound(engine, Q[None], goff, gcols)[0]
    assert np.array_equal(gam, np.diag(Q))               # a singleton's bound is exact
    (w, sw), = descend(engine, Q[None], np.zeros(len(pen), np.int32), np.tile(q, (len(pen), 1)),
                       goff, gcols, ls, l2)
    for f, (a, rho) in enumerate(pen):
        check_fit(f"singletons alpha={a} rho={rho}", Q, q, ls[f], l2[f], goff, gcols, w[f],
                  int(sw[f]), C.solution(name, a, rho, singletons=True)[0])


def test_many_fits_two_grams(engine):
    """27 fits on two Q (with / without centring), three right-hand sides each: full multi-fit
    workgroups, one that straddles the two Q, and a partly filled last one; fits of one
    workgroup differ in alpha and right-hand side."""
    from sglm_hip import _lib
    Qs, fits, goff, gcols = C.many_fits()
    fpw = _lib.query("sglm_group_cd_fits_per_wg", Qs.shape[1])
    nfit = len(fits)
    assert nfit == 27 and nfit > 2 * fpw and nfit % fpw and 13 % fpw     # straddle + partial
    (w, sw), (w2, sw2) = descend(engine, Qs, np.array([f[0] for f in fits], np.int32),
                                 np.stack([f[1] for f in fits]), goff, gcols,
                                 np.array([f[2] for f in fits]), np.array([f[3] for f in fits]),
                                 calls=2)
    assert np.array_equal(w.view(np.uint64), w2.view(np.uint64)) and np.array_equal(sw, sw2)
    worst = 0.0
    for f, (qi, q, ls, l2) in enumerate(fits):
        w_ref, _ = C.gmd(Qs[qi], q, ls, l2, goff, gcols)
        worst = max(worst, check_fit(f"fit {f} (Q {qi})", Qs[qi], q, ls, l2, goff, gcols, w[f],
                                     int(sw[f]), w_ref)[0])
    assert sw[12] == 1 and sw[25] == 1
    print(f"27 fits: worst distance {worst:.2e}")


def test_duplicated_column_inside_a_group(engine):
    """rho = 1 and a column duplicated inside a group: Q is singular and the minimiser is not
    unique, so the fit is held to the KKT bar and to finiteness only."""
    X, y, ids = C.case("6x5")
    X = X.copy()
    X[:, 1] = X[:, 0]                                    # both in group 0
    n = X.shape[0]
    Q, q, xm, ym = C.centred(X, y)
    goff, gcols = C.csr(ids)
    alphas = (0.002, 0.01)
    ls = np.array([a * n for a in alphas])
    (w, sw), = descend(engine, Q[None], np.zeros(2, np.int32), np.tile(q, (2, 1)), goff, gcols,
                       ls, np.zeros(2))
    for f in range(2):
        assert np.all(np.isfinite(w[f])) and 1 <= sw[f] < MAX_SWEEPS
        viol = C.kkt(Q, q, ls[f], 0.0, goff, gcols, w[f])
        print(f"duplicated column alpha={alphas[f]}: sweeps {sw[f]}, KKT {viol:.2e}")
        assert viol <= KKT_BAR


def test_bad_arguments_return_the_error_status(engine):
    import torch
    from sglm_hip import _lib
    lib = _lib.load()
    p, ng = 6, 2
    Q = torch.eye(p, dtype=torch.float64, device="cuda")
    q = torch.ones((1, p), dtype=torch.float64, device="cuda")
    go = torch.tensor([0, 3, 6], dtype=torch.int32, device="cuda")
    gc = torch.arange(p, dtype=torch.int32, device="cuda")
    gam = torch.ones((1, ng), dtype=torch.float64, device="cuda")
    one = torch.ones(1, dtype=torch.float64, device="cuda")
    qi = torch.zeros(1, dtype=torch.int32, device="cuda")
    w = torch.full((1, p), 7.0, dtype=torch.float64, device="cuda")
    sw = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = engine._stream()
    EINVAL = 1

    def cd(p_=p, Q_=Q, gc_=gc, go_=go, w_=w):
        return lib.sglm_group_cd_shared(Q_.data_ptr() if Q_ is not None else None, p_,
                                        qi.data_ptr(), 1, q.data_ptr(), go_.data_ptr(),
                                        gc_.data_ptr() if gc_ is not None else None, ng,
                                        gam.data_ptr(), one.data_ptr(), one.data_ptr(), 100, TOL,
                                        w_.data_ptr() if w_ is not None else None, sw.data_ptr(), s)

    def bd(p_=p, Q_=Q, gc_=gc, go_=go, gam_=gam):
        return lib.sglm_group_bound(Q_.data_ptr() if Q_ is not None else None, p_, 1,
                                    go_.data_ptr(), gc_.data_ptr() if gc_ is not None else None,
                                    ng, gam_.data_ptr() if gam_ is not None else None, s)

    assert cd() == 0 and bd() == 0                       # the arguments are good as they stand
    torch.cuda.synchronize()
    assert sw.item() >= 1
    assert cd(p_=4097) == EINVAL and bd(p_=4097) == EINVAL
    assert b"4096" in lib.sglm_last_error()
    assert cd(Q_=None) == EINVAL and cd(gc_=None) == EINVAL and cd(w_=None) == EINVAL
    assert bd(Q_=None) == EINVAL and bd(gc_=None) == EINVAL and bd(gam_=None) == EINVAL
    bad = gc.clone()
    bad[4] = p                                           # a column index out of range
    assert cd(gc_=bad) == EINVAL and bd(gc_=bad) == EINVAL
    assert b"gcols" in lib.sglm_last_error()
    dup = gc.clone()
    dup[4] = 0                                           # a column listed twice
    assert cd(gc_=dup) == EINVAL
    off = torch.tensor([0, 3, 5], dtype=torch.int32, device="cuda")      # does not end at p
    assert cd(go_=off) == EINVAL and bd(go_=off) == EINVAL
    torch.cuda.synchronize()
