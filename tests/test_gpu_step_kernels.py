"""The mask-sum and step-control kernels of csrc/api.hip on the MI355X against the oracles of
tests/step_cases.py, each export called directly through sglm_hip._lib.call, and two end-to-end
A/B runs of the engine switches that route through two of them.

sglm_mask_stats: count and min exact (count 0 and min +inf for an empty mask), slot 3 exactly 0
for power < 0, the three sums within 1e-12 sum m|term| (the bar test_gpu_nb2ml_kernels.py holds
the same two-level fixed-order reduction to).  sglm_eta_axpy_max: dmax exactly the float32 max,
eta within 2^-23 (|eta| + |t deta|).  sglm_aa_step: the bound of step_cases.aa_oracle for the
accepted fit, everything else bit for bit.  sglm_step_decide: bit for bit (the kernel's _rn
intrinsics follow the host's operand order; the trial steps are powers of two).
Outputs are allocated poisoned (NaN, 0x7f bytes); what a call does not name must stay so."""
import numpy as np
import pytest

import step_cases as C

pytestmark = pytest.mark.gpu

POISON_I32 = 0x7f7f7f7f


def _t(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@pytest.mark.parametrize("n", C.MS_N)
def test_mask_stats(engine, n):
    import torch
    from sglm_hip import _lib
    E = engine
    worst = 0.0
    for power in C.MS_POWERS:
        M, Y, K = C.mask_stats_case(n, power >= 2)
        F, R, ldm = M.shape[0], Y.shape[0], M.shape[1]
        ref, mag = C.mask_stats_oracle(M, Y, K, n, power)
        Md, Yd, Kd = _t(torch, M), _t(torch, Y), _t(torch, K)
        out = torch.full((R + 1, F, 5), float("nan"), dtype=torch.float64, device="cuda")
        work = torch.empty(_lib.query("sglm_mask_stats_work_bytes", F, R, n), dtype=torch.uint8,
                           device="cuda")
        _lib.call("sglm_mask_stats", E._p(Md), ldm, F, E._p(Yd), R, n, E._p(Kd), float(power),
                  E._p(out), E._p(work), None)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.isnan(out[R]).all()
        out = out[:R]
        assert np.array_equal(out[:, :, 0], ref[:, :, 0].astype(np.float64)), power
        assert np.array_equal(out[:, :, 4], ref[:, :, 4].astype(np.float64)), power
        assert not out[:, 2, :4].any() and np.isposinf(out[:, 2, 4]).all()      # the empty mask
        if power < 0:
            assert not out[:, :, 3].any() and not np.signbit(out[:, :, 3]).any()
        err = np.abs(out[:, :, 1:4].astype(C.LD) - ref[:, :, 1:4])
        assert (err <= C.MS_BAR * mag).all(), (power, (err / np.maximum(mag, 1e-300)).max())
        nz = mag > 0
        if nz.any():
            worst = max(worst, float((err[nz] / mag[nz]).max()))
    print(f"\n[mask_stats] n={n}: worst |sum - ref| / sum m|term| = {worst:.3e} "
          f"(bar {C.MS_BAR:.0e})")


@pytest.mark.parametrize("n", C.EA_N)
def test_eta_axpy_max(engine, n):
    import torch
    from sglm_hip import _lib
    E = engine
    ld, eta, deta, M = C.eta_axpy_case(n)
    e64, bound, dmax_ref = C.eta_axpy_oracle(n, eta, deta, M)
    ed, dd, Md = _t(torch, eta), _t(torch, deta), _t(torch, M)
    st, fm = _t(torch, C.EA_STEP), _t(torch, C.EA_FIT_MASK)
    dmax = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.call("sglm_eta_axpy_max", n, ld, 3, E._p(st), E._p(dd), E._p(Md), E._p(fm), E._p(ed),
              E._p(dmax), None)
    torch.cuda.synchronize()
    got, dmax = ed.cpu().numpy(), dmax.cpu().numpy()
    assert got[3].tobytes() == eta[3].tobytes()                     # a fit no call names
    assert got[:, n:].tobytes() == eta[:, n:].tobytes()             # rows [n, ld)
    assert got[1].tobytes() == eta[1].tobytes() and dmax[1] == 0.0  # step 0
    assert np.isnan(dmax[3])
    assert dmax[:3].tobytes() == dmax_ref.tobytes(), (dmax, dmax_ref)
    err = np.abs(got[:3, :n].astype(np.float64) - e64)
    nz = bound > 0
    print(f"\n[eta_axpy_max] n={n}: worst |eta - ref| / bound = "
          f"{float((err[nz] / bound[nz]).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("P,p", C.AA_SHAPES)
def test_aa_step(engine, P, p):
    import torch
    from sglm_hip import _lib
    E = engine
    delta, raw, used, gtot, rm = C.aa_case(P, p)
    o = C.aa_oracle(P, p, delta, raw, used, gtot)
    dd, rd, ud, gd, md = (_t(torch, a) for a in (delta, raw, used, gtot, rm))
    # named, so that they live until the kernel has run (a temporary's block is reused at once)
    slots, sel, tprev = _t(torch, C.AA_SLOTS), _t(torch, C.AA_SEL), _t(torch, C.AA_TPREV)
    _lib.call("sglm_aa_step", P, p, len(C.AA_SLOTS), E._p(slots), E._p(sel), E._p(tprev),
              E._p(dd), E._p(rd), E._p(ud), E._p(gd), E._p(md), None)
    torch.cuda.synchronize()
    d1, r1, u1, g1, m1 = (a.cpu().numpy() for a in (dd, rd, ud, gd, md))
    assert u1.tobytes() == used.tobytes() and g1.tobytes() == gtot.tobytes()
    for k in sorted(set(range(C.AA_NSLOT)) - set(C.AA_SLOTS)):      # slots no fit names
        for new, old in ((d1, delta), (r1, raw), (u1, used), (m1, rm)):
            assert new[k].tobytes() == old[k].tobytes(), k
    for q, x in enumerate(o):
        k = C.AA_SLOTS[q]
        assert r1[k].tobytes() == delta[k].tobytes(), C.AA_KINDS[q]          # raw_prev = f
        assert (m1[k, 0], m1[k, 1]) == tuple(np.float32(v) for v in x["rm"]), C.AA_KINDS[q]
        if not x["good"]:
            assert d1[k].tobytes() == delta[k].tobytes(), C.AA_KINDS[q]
    acc = o[0]
    k = C.AA_SLOTS[0]
    assert acc["good"] and d1[k].tobytes() != delta[k].tobytes()
    err = np.abs(d1[k].astype(np.float64) - acc["dnew"])
    print(f"\n[aa_step] P={P} p={p}: accepted fit worst |d - ref| / bound = "
          f"{float((err / acc['bound']).max()):.3f}")
    assert (err <= acc["bound"]).all()


@pytest.mark.parametrize("legacy", [0, 1])
@pytest.mark.parametrize("nts", [5, 12])
@pytest.mark.parametrize("na", C.SD_NA)
def test_step_decide(engine, na, nts, legacy):
    import torch
    from sglm_hip import _lib
    E = engine
    act, L, sc, aa_rm, prev_rel, fresh, n_iter, max_iter, _ = C.decide_case(na, nts)
    ts = C.decide_ts(nts)
    dev = [_t(torch, a) for a in (act, L, sc, ts, aa_rm, prev_rel, fresh, n_iter, max_iter)]
    act_d, L_d, sc_d, ts_d, rm_d, pr_d, fr_d, ni_d, mi_d = dev
    for with_rm in (False, True):
        o = C.decide_oracle(act, L, sc, nts, ts, C.SD_SIGMA, C.SD_TOL, C.SD_SFLOOR, legacy,
                            aa_rm if with_rm else None, prev_rel, fresh, n_iter, max_iter)
        f64 = torch.full((3, na + 2), float("nan"), dtype=torch.float64, device="cuda")
        f32 = torch.full((na + 2,), float("nan"), dtype=torch.float32, device="cuda")
        i32 = torch.full((5, na + 2), POISON_I32, dtype=torch.int32, device="cuda")
        _lib.call("sglm_step_decide", na, E._p(act_d), E._p(L_d), E._p(sc_d), nts, E._p(ts_d),
                  C.SD_SIGMA, C.SD_TOL, C.SD_SFLOOR, legacy, E._p(rm_d) if with_rm else None,
                  E._p(pr_d), E._p(fr_d), E._p(ni_d), E._p(mi_d), E._p(f64[0]), E._p(f32),
                  E._p(f64[1]), E._p(f64[2]), E._p(i32[0]), E._p(i32[1]), E._p(i32[2]),
                  E._p(i32[3]), E._p(i32[4]), None)
        torch.cuda.synchronize()
        f64, f32, i32 = f64.cpu().numpy(), f32.cpu().numpy(), i32.cpu().numpy()
        tag = (na, nts, legacy, with_rm)
        assert np.isnan(f64[:, na:]).all() and np.isnan(f32[na:]).all(), tag
        assert (i32[:3, na:] == POISON_I32).all(), tag
        cnt = int(i32[4, 0])
        assert cnt == o["cnt"] and (i32[4, 1:] == POISON_I32).all(), tag
        assert (i32[3, cnt:] == POISON_I32).all(), tag              # nxt past cnt
        assert np.array_equal(i32[0, :na], o["flags"]), tag
        assert np.array_equal(i32[1, :na], o["tix"]), tag
        assert np.array_equal(i32[2, :na], o["rpos"]), tag
        assert np.array_equal(i32[3, :cnt], o["nxt"]), tag
        assert f64[0, :na].tobytes() == o["step64"].tobytes(), tag
        assert f32[:na].tobytes() == o["step32"].tobytes(), tag
        assert f64[1, :na].tobytes() == o["relv"].tobytes(), tag
        assert f64[2, :na].tobytes() == o["prop"].tobytes(), tag


def _poisson_grid(E, monkeypatch, name):
    """a 3-split x 4-lambda Poisson grid; returns (results, calls of `name`, calls in all,
    fit-iterations that ran the secant correction)"""
    import pandas as pd
    from sglm_hip import _lib, folds, grid, synth
    from sglm_hip.estimators import Objective
    s = synth.make(N=20_000, m=10, L=5, family="poisson", rho=0.03)
    codes = folds.trial_keys_codes(pd.DataFrame({"nTrial": s.trial}), ["nTrial"]).values
    np.random.seed(3)
    cv_idx = folds.cv_idx_from_bucket_ids(codes, num_folds=3)
    d = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    objs = [Objective("irls", E.FAM_TWEEDIE_LOG, 1.0, a, "n", True, 100)
            for a in (1e-3, 1e-2, 1e-1, 1.0)]
    count = {"name": 0, "all": 0}
    real = _lib.call

    def shim(fn, *args):
        count["all"] += 1
        count["name"] += fn == name
        return real(fn, *args)
    with monkeypatch.context() as m:
        m.setattr(_lib, "call", shim)
        st = E.IrlsStats()
        res = grid.run(d, s.y, cv_idx, objs, [0] * len(objs), stats=st)
    return res, count["name"], count["all"], int(st.aa_fit_iters)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def _same_fits(on, off, tag):
    for j, (a, b) in enumerate(zip(on, off)):
        print(f"\n[{tag}] objective {j}: n_iter on {list(np.ravel(a['n_iter']))} "
              f"off {list(np.ravel(b['n_iter']))}")
    worst = max(_rel(a[k], b[k]) for a, b in zip(on, off)
                for k in ("cv_coefs", "cv_intercepts", "refit_coef"))
    print(f"[{tag}] worst relative difference on / off = {worst:.3e} (bar 1e-6)")
    for j, (a, b) in enumerate(zip(on, off)):
        assert np.all(a["converged"]) and np.all(b["converged"]), j
        assert _rel(a["cv_coefs"], b["cv_coefs"]) < 1e-6, j
        assert _rel(a["cv_intercepts"], b["cv_intercepts"]) < 1e-6, j
        assert _rel(a["refit_coef"], b["refit_coef"]) < 1e-6, j


def test_aa_kernel_on_off(engine, monkeypatch):
    """AA_KERNEL (the default) against the torch expressions it replaced: the same fits (1e-6,
    the bar test_gpu_api.py holds GRAD_DEDUP on / off to), every fit converged."""
    E = engine
    assert E.ANDERSON
    monkeypatch.setattr(E, "AA_KERNEL", True)               # the default
    on, n_on, n_all, aa_on = _poisson_grid(E, monkeypatch, "sglm_aa_step")
    assert n_on >= 1 and n_all > n_on
    monkeypatch.setattr(E, "AA_KERNEL", False)
    off, n_off, _, aa_off = _poisson_grid(E, monkeypatch, "sglm_aa_step")
    assert n_off == 0
    print(f"\n[AA_KERNEL] sglm_aa_step calls {n_on}, selected fit-iterations on {aa_on} "
          f"off {aa_off}")
    assert aa_on > 0 and aa_off > 0                         # the correction itself ran in both
    _same_fits(on, off, "AA_KERNEL")


def test_dev_decide_on_off(engine, monkeypatch):
    """DEV_DECIDE (off by default; shipped and documented) against the host's decisions."""
    E = engine
    monkeypatch.setattr(E, "DEV_DECIDE", False)             # the default
    off, n_off, n_all, _ = _poisson_grid(E, monkeypatch, "sglm_step_decide")
    assert n_off == 0 and n_all > 0
    monkeypatch.setattr(E, "DEV_DECIDE", True)
    on, n_on, _, _ = _poisson_grid(E, monkeypatch, "sglm_step_decide")
    assert n_on >= 1
    print(f"\n[DEV_DECIDE] sglm_step_decide calls {n_on}")
    _same_fits(on, off, "DEV_DECIDE")
