"""The kernels of csrc/cd.hip on the MI355X against the longdouble oracles of tests/cd_cases.py,
each export called directly through sglm_hip._lib.call.

sglm_enet_cd_grouped / sglm_enet_cd_shared run with tol = 0 and max_sweeps = S in {1, 3}: all
forms do the same fixed work, and tests/test_cd_cases_cpu.py shows that no sweep count of the
cases hangs on rounding.  The coefficients are held to 1e-9 max|w_ref| per fit (the bar of
test_gpu_tweedie_enet.py for the other CD kernels), the sweep counts and the dead column exactly,
and the lane and reg forms to each other bit for bit.
  lane form (enet_cd_lane_kernel<8,512,4,2>, the default) and reg form (SGLM_CD_FPW=4) at p in
  {1, 7, 511, 512, 513, 1025, 2047, 2048}: owner registers 0..3 (p > 512, 1024, 1536), the
  depth-2 row ring at odd and even p and at its last two rows, 11 workgroups (11 % 8 != 0: the
  XCD remap must be a bijection, with wg_q not sorted) and 3;
  multi form (the only one there) at p = 2049 (fpw 4) and p = 2262 (fpw 2);
  shared form at p in {7, 513, 4071}.
sglm_center_gram: 4 * 2^-53 (|G_ab| + |G_ap G_bp| / n) per entry (the product of two counts is
exact; one division, one subtraction).  sglm_gram_ss: (pa + 64) 2^-53 of the terms' magnitudes.
Outputs are allocated poisoned; rows no call names must come back untouched."""
import numpy as np
import pytest

import cd_cases as C

pytestmark = pytest.mark.gpu

def _grouped(E, lib, torch, p, S, fpw, sparse, nfit):
    """one sglm_enet_cd_grouped call on cd_case(p, nfit); returns (w, sweeps) by fit, and checks
    that the two rows no workgroup names are untouched"""
    Qs, fit_q, q, l1, l2 = C.cd_case(p, nfit)
    assert lib.query("sglm_enet_cd_fits_per_wg", p) == fpw
    rows, spare = C.fit_rows(nfit)
    wg_fits, wg_q = C.layout(fit_q, rows, fpw, sparse)
    nb = nfit + 2
    qb = np.full((nb, p), np.nan)
    l1b, l2b = np.full(nb, np.nan), np.full(nb, np.nan)
    qb[rows], l1b[rows], l2b[rows] = q, l1, l2
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)
    Qd, qd, l1d, l2d = t(Qs), t(qb), t(l1b), t(l2b)
    wf, wq = t(wg_fits), t(wg_q)
    w = torch.full((nb, p), float("nan"), dtype=torch.float64, device=dev)
    sw = torch.full((nb,), 0x7f7f7f7f, dtype=torch.int32, device=dev)
    lib.call("sglm_enet_cd_grouped", E._p(Qd), p, E._p(wf), wg_fits.shape[0], fpw, E._p(wq),
             E._p(qd), E._p(l1d), E._p(l2d), S, 0.0, E._p(w), E._p(sw), None)
    torch.cuda.synchronize()
    w, sw = w.cpu().numpy(), sw.cpu().numpy()
    assert np.isnan(w[spare]).all() and (sw[spare] == 0x7f7f7f7f).all()
    return w[rows], sw[rows], wg_fits.shape[0]


def _check(p, S, nfit, w, sw, tag):
    w_ref, sw_ref, ratios = C.cd_reference(p, S, nfit)
    q, l1 = C.cd_case(p, nfit)[2:4]
    assert np.isfinite(w).all()
    scale = np.abs(w_ref).max(axis=1)
    err = np.abs(w - w_ref).max(axis=1)
    worst = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    print(f"\n[cd {tag}] p={p} S={S}: worst |w - w_ref| / max|w_ref| = {worst:.3e} "
          f"(bar {C.BAR_W:.0e})")
    if p > 1:                                               # no sweep count hangs on rounding
        assert all(r == [np.inf] or min(r) > 1e-6 for r in ratios)
    assert (err <= C.BAR_W * scale).all(), (err / np.maximum(scale, 1e-300)).max()
    assert np.array_equal(sw, sw_ref), (sw, sw_ref)
    zero = l1 > np.abs(q).max(axis=1)
    assert zero.any() and not w[zero].any() and (sw[zero] == 1).all()
    dc = C.dead_column(p)
    if dc is not None:
        assert not w[:, dc].any()
    return worst


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("p", C.P_REG)
def test_grouped_lane_and_reg_forms(engine, monkeypatch, p, S):
    import torch
    from sglm_hip import _lib
    E = engine
    out = {}
    for form, fpw in (("lane", 8), ("reg", 4)):
        if fpw == 4:
            monkeypatch.setenv("SGLM_CD_FPW", "4")
        else:
            monkeypatch.delenv("SGLM_CD_FPW", raising=False)
        for sparse in (True, False):
            w, sw, nwg = _grouped(E, _lib, torch, p, S, fpw, sparse, 19)
            assert nwg == {(8, True): 11, (8, False): 3, (4, True): 11, (4, False): 6}[fpw, sparse]
            _check(p, S, 19, w, sw, f"{form} nwg={nwg}")
            out[form, sparse] = w
    # per coordinate the arithmetic and the fold order of the two forms are the same
    # (csrc/cd.hip, enet_cd_lane_kernel), whatever the workgroup a fit runs in
    ref = out["lane", True].tobytes()
    assert all(v.tobytes() == ref for v in out.values())


@pytest.mark.parametrize("p,fpw", [(2049, 4), (2262, 2)])
def test_grouped_multi_form(engine, monkeypatch, p, fpw):
    """2048 < p <= 4070 reaches only enet_cd_multi_kernel ((2 fpw + 1) p doubles of LDS)."""
    import torch
    from sglm_hip import _lib
    monkeypatch.delenv("SGLM_CD_FPW", raising=False)
    w, sw, nwg = _grouped(engine, _lib, torch, p, 1, fpw, False, 5)
    assert nwg == {4: 2, 2: 4}[fpw]
    _check(p, 1, 5, w, sw, f"multi<{fpw}> nwg={nwg}")


@pytest.mark.parametrize("p,nfit,sweeps", [(7, 19, (1, 3)), (513, 19, (1, 3)), (4071, 2, (1,))])
def test_shared_form(engine, p, nfit, sweeps):
    import torch
    from sglm_hip import _lib
    E = engine
    Qs, fit_q, q, l1, l2 = C.cd_case(p, nfit)
    rows, spare = C.fit_rows(nfit)
    nb = nfit + 2
    # sglm_enet_cd_shared runs fits 0 .. nfit-1 of its arrays: the call covers every row, the
    # two spare ones with an all-zero problem (l1 above max|q|) on Q 0
    qb = np.zeros((nb, p))
    l1b, l2b = np.ones(nb), np.ones(nb)
    qidx = np.zeros(nb, dtype=np.int32)
    qb[rows], l1b[rows], l2b[rows], qidx[rows] = q, l1, l2, fit_q
    t = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    Qd, qd, l1d, l2d, qi = t(Qs), t(qb), t(l1b), t(l2b), t(qidx)
    for S in sweeps:
        w = torch.full((nb + 1, p), float("nan"), dtype=torch.float64, device="cuda")
        sw = torch.full((nb + 1,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
        _lib.call("sglm_enet_cd_shared", E._p(Qd), p, E._p(qi), nb, E._p(qd), E._p(l1d),
                  E._p(l2d), S, 0.0, E._p(w), E._p(sw), None)
        torch.cuda.synchronize()
        w, sw = w.cpu().numpy(), sw.cpu().numpy()
        assert np.isnan(w[nb]).all() and sw[nb] == 0x7f7f7f7f       # past the last fit
        assert not w[spare].any() and (sw[spare] == 1).all()
        _check(p, S, nfit, w[rows], sw[rows], "shared")


@pytest.mark.parametrize("center", [0, 1])
@pytest.mark.parametrize("p", [1, 37, 255])
def test_center_gram(engine, p, center):
    import torch
    from sglm_hip import _lib
    E = engine
    H = C.center_case(p)
    nm = len(C.CG_GRAM_OF)
    Hd = torch.from_numpy(np.array(H)).cuda()
    go = torch.from_numpy(np.array(C.CG_GRAM_OF)).cuda()
    Q = torch.full((nm + 1, p, p), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("sglm_center_gram", E._p(Hd), C.CG_P, p, E._p(go), nm, center, E._p(Q), None)
    torch.cuda.synchronize()
    Q = Q.cpu().numpy()
    assert np.isnan(Q[nm]).all()
    Q = Q[:nm]
    Qr, bound = C.center_oracle(H, p, C.CG_GRAM_OF, center)
    assert np.isfinite(Q).all()                             # the NaN lower triangle is not read
    assert np.array_equal(Q, Q.transpose(0, 2, 1))
    assert not Q[1].any()                                   # the empty mask: G_pp = 0, no centring
    err = np.abs(Q.astype(C.LD) - Qr).astype(np.float64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"\n[center_gram] p={p} center={center}: worst got/bound = {ratio:.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("pa", C.GS_PA)
def test_gram_ss(engine, pa):
    import torch
    from sglm_hip import _lib
    E = engine
    H, grp_off, fits, beta, c, cidx, yy, w1 = C.gram_ss_case(pa)
    nfit = len(yy)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    Hd, go, gs, fd, bd, cd, ci, yd = (t(H), t(grp_off), t(C.GS_SLOT), t(fits), t(beta), t(c),
                                      t(cidx), t(yy))
    ss = torch.full((nfit + 3,), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(_lib.query("sglm_gram_ss_work_bytes", pa, nfit), dtype=torch.uint8,
                       device="cuda")
    _lib.call("sglm_gram_ss", E._p(Hd), C.GS_P, pa, E._p(gs), E._p(go), 3, max(C.GS_GROUPS),
              E._p(fd), nfit, E._p(bd), E._p(cd), E._p(ci), E._p(yd), E._p(ss), E._p(work), None)
    torch.cuda.synchronize()
    ss = ss.cpu().numpy()
    assert np.isnan(ss[nfit:]).all()
    ss = ss[:nfit]
    raw, bound = C.gram_ss_oracle(H, pa, grp_off, fits, beta, c, cidx, yy)
    assert raw[w1] == -1 and ss[w1] == 0.0 and not np.signbit(ss[w1])
    ref = np.maximum(raw, 0)
    err = np.abs(ss.astype(C.LD) - ref).astype(np.float64)
    print(f"\n[gram_ss] pa={pa}: worst got/bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(ss).all() and (err <= bound).all()
