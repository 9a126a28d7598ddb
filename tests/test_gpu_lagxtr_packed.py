"""sglm_lag_xtr_packed_bp: the gradient of a time-shifted event design walked over the
occurrences, from the packed R rows, against a float64 numpy X^T R (X built from the definition
on the host) and against the dense bit-plane kernel on the same packed rows.

Mixed-magnitude bound: a lane adds the (exact) f32 values of one event's occurrences inside one
row range one after the other, and the range partials are summed in float64, so
|g - g64| <= (L + 2) 2^-24 sum_t |R_t| X[t, c] with L the largest number of occurrences of one
event inside one row range (L - 1 roundings of the f32 sum, the rest for the float64 sums).
Worst err / bound measured on the MI355X over all cases below: 0.172."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (1, 16, 17, 33, 45)


def shift_list(K, kind):
    """K contiguous shifts: around zero in the order of sglm_ez.timeshift_cols ([0], the
    negative ones, the positive ones), or all positive."""
    if kind == "pos":
        return list(range(2, 2 + K))
    if K == 1:
        return [-1]
    neg = K // 2
    return [0] + list(range(-neg, 0)) + list(range(1, K - neg))


def make_events(n, m, K, shifts, U, H, edges):
    """0/1 events (N_raw x m): random occurrences plus the edge patterns -- event 1 has none;
    windows partly before row 0 and partly past n - 1; first-lag rows on both sides of every
    tile edge and range edge in `edges`; a run of consecutive occurrences (overlapping windows)."""
    smin, smax = min(shifts), max(shifts)
    row0 = max(smax, 0)
    n_raw = n + row0 - smin + 2
    rng = np.random.default_rng(1000 * n + 10 * m + K)
    E = (rng.random((n_raw, m)) < 0.03).astype(np.float32)
    to_u = row0 - smin                                 # u of a first-lag design row v
    marks = [-(K - 1), -(K // 2), 0, n - K, n - K + 1, n - 2, n - 1, n, n + 1]
    for e in edges:
        marks += [e - K, e - 2, e - 1, e, e + 1, e + U - 1]
    a0 = 0
    for v in marks:
        u = v + to_u
        if 0 <= u < n_raw:
            E[u, a0] = 1.0
    run0 = min(max(n // 2, 0), n_raw - 12)
    E[run0:run0 + 12, m - 1] = 1.0
    if m >= 3:
        E[:, 1] = 0.0
    return E, row0, n_raw


def dense_x(E, shifts, row0, n, event_major):
    """X[t, col(b, a)] = E[t + row0 - shifts[b], a] (zero outside E), then the ones column."""
    n_raw, m = E.shape
    K = len(shifts)
    X = np.zeros((n, m * K + 1))
    t = np.arange(n)
    for b, s in enumerate(shifts):
        u = t + row0 - s
        ok = (u >= 0) & (u < n_raw)
        for a in range(m):
            X[ok, a * K + b if event_major else b * m + a] = E[u[ok], a]
    X[:, m * K] = 1.0
    return X


def split3(R):
    import torch
    hi = R.to(torch.bfloat16)
    mid = (R - hi.float()).to(torch.bfloat16)
    lo = (R - hi.float() - mid.float()).to(torch.bfloat16)
    assert torch.equal((hi.float() + mid.float()) + lo.float(), R)
    return hi, mid, lo


class Case:
    """One design with its reference X; R rows and their float64 products made once."""

    def __init__(self, n, m, K, event_major, kind):
        import torch
        from sglm_hip import engine as E_
        self.n, self.m, self.K, self.event_major = n, m, K, event_major
        self.shifts = shift_list(K, kind)
        pl = E_.lag_xtr_plan(n, 45, K, 256)
        self.U, self.H = pl["U"], pl["H"]
        edges = set()
        for c in COUNTS:
            q = E_.lag_xtr_plan(n, c, K, 256)
            edges |= {i * self.U - self.H for i in range(1, q["ntiles"])}      # tile edges
            edges |= {r * q["tiles_per"] * self.U - self.H for r in range(1, q["nranges"])}
        Ev, self.row0, self.n_raw = make_events(n, m, K, self.shifts, self.U, self.H,
                                                sorted(edges))
        self.Ev = Ev
        self.d = E_.Design.from_events(torch.from_numpy(Ev), self.shifts, self.row0, n,
                                       event_major=event_major)
        assert self.d.lag is not None and self.d.lag.px is not None
        self.X = dense_x(Ev, self.shifts, self.row0, n, event_major)
        rng = np.random.default_rng(7)
        B = max(COUNTS)
        self.R_int = rng.integers(-8, 9, size=(B, n)).astype(np.float32)
        mag = np.exp2(rng.uniform(-20, 10, size=(B, n))) * rng.choice([-1.0, 1.0], size=(B, n))
        self.R_mix = mag.astype(np.float32)
        self.ref = {id(R): (R.astype(np.float64) @ self.X, np.abs(R).astype(np.float64) @ self.X)
                    for R in (self.R_int, self.R_mix)}

    def longest_run(self, count):
        """L: the most occurrences of one event that one row range owns."""
        from sglm_hip import engine as E_
        q = E_.lag_xtr_plan(self.n, count, self.K, 256)
        toff = self.d.lag.px[0].cpu().numpy().reshape(q["ntiles"] + 1, self.m)
        best = 0
        for r in range(q["nranges"]):
            i0, i1 = r * q["tiles_per"], min((r + 1) * q["tiles_per"], q["ntiles"])
            best = max(best, int((toff[i1] - toff[i0]).max()))
        return best

    def run(self, R, count, dense=False):
        """G (rows NaN where unlisted) of the first `count` rows of R: permuted slots with gaps,
        a plane stride larger than pad32(count), garbage in the unused rows and past n."""
        import torch
        from sglm_hip import _lib, engine as E_
        d, lg = self.d, self.d.lag
        Bp = (count + 31) // 32 * 32 + 32
        Rd = torch.full((count, d.ld), 3.0, dtype=torch.float32, device="cuda")
        Rd[:, :self.n] = torch.from_numpy(R[:count]).cuda()
        rp = torch.full((3, Bp, d.ld), 7.0, dtype=torch.bfloat16, device="cuda")
        rp[0, :count], rp[1, :count], rp[2, :count] = split3(Rd)
        slots_h = (np.random.default_rng(count).permutation(count) * 2 + 1).astype(np.int32)
        slots = torch.from_numpy(slots_h).cuda()
        G = torch.full((2 * count + 2, d.P), float("nan"), dtype=torch.float64, device="cuda")
        if dense:
            w = torch.empty(_lib.query("sglm_xtr_bits_packed_work_bytes", d.P, count, d.ld),
                            dtype=torch.uint8, device="cuda")
            _lib.call("sglm_xtr_bits_packed_bp", d.cbits_full().data_ptr(), d.ld, d.P, d.n,
                      rp.data_ptr(), count, Bp, slots.data_ptr(), G.data_ptr(), w.data_ptr(), 0)
        else:
            w = torch.empty(E_.lag_xtr_plan(self.n, count, self.K, d.P)["work_bytes"],
                            dtype=torch.uint8, device="cuda")
            _lib.call("sglm_lag_xtr_packed_bp", lg.occ.data_ptr(), int(lg.occ.numel()),
                      lg.px[0].data_ptr(), lg.px[1].data_ptr(), lg.m, lg.K, lg.smin, lg.smax,
                      lg.layout, lg.row0, d.n, d.ld, d.P, rp.data_ptr(), count, Bp,
                      slots.data_ptr(), G.data_ptr(), w.data_ptr(), 2, 0)
        torch.cuda.synchronize()
        return G.cpu().numpy(), slots_h


# every m with every K; n, the layout and the shift range alternate so that each value of each
# meets both values of the others
CASES = [(n, m, K, bool((i + j) % 2), "zero" if (i + j // 2) % 2 else "pos")
         for i, m in enumerate((1, 3, 5, 17)) for j, K in enumerate((1, 4, 7, 40))
         for n in ((700, 5000)[(i + j) % 2],)] + [(5000, 3, 40, False, "zero"),
                                                  (700, 17, 7, True, "pos"),
                                                  (5000, 17, 4, False, "pos"),
                                                  (700, 5, 1, True, "zero")]
_cases = {}


def get_case(key):
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


@pytest.mark.parametrize("n,m,K,event_major,kind", CASES)
def test_packed_walk_vs_float64_and_dense(engine, n, m, K, event_major, kind):
    c = get_case((n, m, K, event_major, kind))
    p1 = m * K + 1
    worst = 0.0
    rows45 = None
    for count in COUNTS:
        # small integers: every sum is exact
        G, slots = c.run(c.R_int, count)
        ref, _ = c.ref[id(c.R_int)]
        assert np.array_equal(G[slots, :p1], ref[:count]), ("exact", count)
        assert np.all(G[slots, p1:] == 0.0)                          # padding columns
        unlisted = np.setdiff1d(np.arange(G.shape[0]), slots)
        assert np.all(np.isnan(G[unlisted]))                         # untouched
        Gd, _ = c.run(c.R_int, count, dense=True)
        assert np.array_equal(G[slots], Gd[slots]), ("dense", count)
        # mixed magnitudes
        G, slots = c.run(c.R_mix, count)
        ref, scale = c.ref[id(c.R_mix)]
        L = c.longest_run(count)
        err = np.abs(G[slots, :p1 - 1] - ref[:count, :p1 - 1])
        bound = (L + 2) * 2.0 ** -24 * scale[:count, :p1 - 1]
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        print(f"[lagxtr] n={n} m={m} K={K} count={count} L={L}: worst err/bound {ratio:.3g}")
        assert np.all(err <= bound), (count, ratio)
        assert np.all(G[slots, p1:] == 0.0)
        assert np.all(np.abs(G[slots, p1 - 1] - ref[:count, p1 - 1])
                      <= n * 2.0 ** -53 * scale[:count, p1 - 1])     # the intercept column
        G2, _ = c.run(c.R_mix, count)
        assert np.array_equal(G[slots].view(np.int64), G2[slots].view(np.int64))   # two runs
        if count == 33:
            rows33 = G[slots]
        if count == 45:
            rows45 = G[slots]
    # one 32-fit group count, one set of row ranges: a fit's row does not depend on the count
    assert np.array_equal(rows33.view(np.int64), rows45[:33].view(np.int64))
    print(f"[lagxtr] n={n} m={m} K={K}: worst err/bound over the counts {worst:.3g}")


def test_uncovered_shape_is_refused_and_engine_keeps_dense(engine, monkeypatch):
    import torch
    from sglm_hip import _lib, synth
    from sglm_hip.estimators import Objective
    from sglm_hip import grid
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.HipEngineError, match="status %d" % 1):
        _lib.call("sglm_lag_xtr_packed_bp", z.data_ptr(), 0, z.data_ptr(), z.data_ptr(), 3, 41,
                  -20, 20, 0, 20, 1000, 1024, 256, z.data_ptr(), 1, 32, z.data_ptr(),
                  z.data_ptr(), z.data_ptr(), 2, 0)
    # shifts with a gap: no table, and the solve takes the dense kernel
    s = synth.make(N=4000, m=4, L=2, family="poisson", rho=0.05, seed=2)
    shifts = [0, -3, -1, 1]
    d = engine.Design.from_events(s.E, shifts, 1, 3990)
    assert d.lag is not None and d.lag.px is None
    monkeypatch.setattr(engine, "XTR_EVENTS", "1")
    st = engine.IrlsStats()
    y = s.y[:3990]
    out = grid.run(d, y, [(np.arange(0, 3000), np.arange(3000, 3990))],
                   [Objective("irls", engine.FAM_TWEEDIE_LOG, 1.0, 0.01, "n", True, 100)], [0],
                   stats=st)
    assert st.grad_events == 0 and out[0]["converged"]


def test_small_grid_events_vs_dense(engine, monkeypatch):
    """n = 20,000, 5 events x 8 lags, 3 splits x 4 penalties and their refits, with the gradient
    from the dense kernel and from the occurrences."""
    import pandas as pd
    from oracle import glm_ref
    from sglm_hip import folds, grid, synth
    from sglm_hip.estimators import Objective
    s = synth.make(N=20000, m=5, L=4, family="poisson", rho=0.03, seed=5)
    d = engine.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    assert len(s.shifts) == 8 and d.lag.px is not None
    codes = folds.trial_keys_codes(pd.DataFrame({"nTrial": s.trial}), ["nTrial"]).values
    np.random.seed(3)
    cv_idx = folds.cv_idx_from_bucket_ids(codes, num_folds=3)
    lams = (1e-3, 1e-2, 1e-1, 1.0)
    objs = [Objective("irls", engine.FAM_TWEEDIE_LOG, 1.0, a, "n", True, 100) for a in lams]
    res, stats = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setattr(engine, "XTR_EVENTS", mode)
        stats[mode] = engine.IrlsStats()
        res[mode] = grid.run(d, s.y, cv_idx, objs, [0] * len(objs), stats=stats[mode])
    assert stats["0"].grad_events == 0
    assert stats["1"].grad_events == stats["1"].newton_iters > 0
    assert stats["0"].newton_iters == stats["1"].newton_iters
    assert stats["0"].gram_fits == stats["1"].gram_fits
    assert stats["0"].fit_iters == stats["1"].fit_iters
    top = 0.0
    for a, b in zip(res["0"], res["1"]):
        for key in ("cv_coefs", "refit_coef", "cv_intercepts", "refit_intercept"):
            x, y = np.asarray(a[key], float), np.asarray(b[key], float)
            scale = max(np.max(np.abs(np.asarray(a["refit_coef"]))), 1e-30)
            top = max(top, float(np.max(np.abs(x - y)) / scale))
            assert np.max(np.abs(x - y)) <= 1e-6 * scale, key
        assert a["n_iter"] == b["n_iter"] and a["converged"] and b["converged"]
    print(f"[lagxtr] small grid: largest coefficient difference / max|coef| {top:.3g}")
    X = s.dense_X()
    tr = cv_idx[1][0]
    for mode in ("0", "1"):
        c, b = glm_ref.fit_tweedie_newton(X, s.y, lams[1], 1.0)
        got = np.asarray(res[mode][1]["refit_coef"], float)
        assert np.max(np.abs(got - c)) / np.max(np.abs(c)) < 1e-4
        assert abs(res[mode][1]["refit_intercept"] - b) < 1e-4 * max(1.0, abs(b))
        c, b = glm_ref.fit_tweedie_newton(X[tr], s.y[tr], lams[2], 1.0)
        got = np.asarray(res[mode][2]["cv_coefs"], float)[:, 1]
        assert np.max(np.abs(got - c)) / np.max(np.abs(c)) < 1e-4
