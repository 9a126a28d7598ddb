"""The tiling of the packed-R occurrence walk (sglm_lag_xtr_packed_bp) without a GPU: the plan
(sglm_lag_xtr_plan, host only) and the (tile, event) offset table built from it
(engine.lag_xtr_offsets) on random occurrence lists."""
import numpy as np
import pytest


def _occurrences(rng, m, n_raw, rate):
    ev, rows = [], []
    for a in range(m):
        if a == 1:
            continue                                   # an event with no occurrence
        u = np.flatnonzero(rng.random(n_raw) < rate)
        if a == 0:                                     # the first and the last raw rows, a run
            u = np.union1d(u, np.r_[0:5, n_raw - 3:n_raw, n_raw // 2:n_raw // 2 + 9])
        ev.append(np.full(u.size, a))
        rows.append(u)
    return np.concatenate(ev).astype(np.int64), np.concatenate(rows).astype(np.int64)


@pytest.mark.parametrize("n,m,K,smin,count", [(700, 3, 4, -2, 1), (5000, 5, 7, 1, 17),
                                              (5000, 17, 40, -20, 45), (40_000, 6, 40, -7, 120),
                                              (1024, 2, 1, 0, 33), (1025, 4, 8, -8, 16)])
def test_every_window_owned_once_and_staged(n, m, K, smin, count):
    import torch
    from sglm_hip import engine as E
    P = 256 * ((m * K + 1 + 255) // 256)
    pl = E.lag_xtr_plan(n, count, K, P)
    U, H, ntiles = pl["U"], pl["H"], pl["ntiles"]
    assert H >= K and H % 8 == 0 and U % 8 == 0
    smax = smin + K - 1
    row0 = max(smax, 0) + 3                            # raw rows 0..2 lie wholly before row 0
    n_raw = n + row0 - min(smin, 0) + 5                # raw rows before and after the design's
    rng = np.random.default_rng(n + K)
    ev, rows = _occurrences(rng, m, n_raw, 0.03)
    toff = E.lag_xtr_offsets(torch.from_numpy(ev), torch.from_numpy(rows), m, row0, smin, U, H,
                             ntiles).numpy().reshape(ntiles + 1, m)
    assert np.all(np.diff(toff, axis=0) >= 0)
    owner = np.full(ev.size, -1)
    times = np.zeros(ev.size, dtype=np.int64)
    for i in range(ntiles):
        for a in range(m):
            owner[toff[i, a]:toff[i + 1, a]] = i
            times[toff[i, a]:toff[i + 1, a]] += 1
            assert np.all(ev[toff[i, a]:toff[i + 1, a]] == a)
    v = rows - row0 + smin                             # design row of the first lag
    touches = (v + K - 1 >= 0) & (v < n)               # some (occurrence, lag) row in [0, n)
    assert touches.any() and (~touches).any()
    assert np.all(times[touches] == 1)                 # owned by exactly one tile
    assert np.all(times <= 1)
    own = owner >= 0
    lo = owner[own] * U - H                            # the owner's staged rows [lo, lo + U + H)
    assert np.all(v[own] >= lo) and np.all(v[own] < lo + U)
    assert np.all(v[own] + K - 1 < lo + U + H)         # no window leaves them
    assert np.all(v[own] + 4 * ((K + 3) // 4) - 1 < lo + U + H)   # nor the lanes' padded reads
    # the ranges tile [0, ntiles)
    tp, nr = pl["tiles_per"], pl["nranges"]
    edges = [(r * tp, min((r + 1) * tp, ntiles)) for r in range(nr)]
    assert edges[0][0] == 0 and edges[-1][1] == ntiles
    assert all(a < b for a, b in edges)
    assert all(edges[r][1] == edges[r + 1][0] for r in range(nr - 1))
    assert ntiles * U - H >= n                         # the tiles' own rows cover the design
    # the work bytes cover the partials of every call with at most `count` fits: per row range
    # and 16-fit group an f32 for every (fit, event <= 64, lag) and a float64 intercept per fit
    assert pl["group_bytes"] >= 16 * (64 * K * 4 + 8)
    for b in range(1, count + 1):
        q = E.lag_xtr_plan(n, b, K, P)
        assert q["nranges"] * -(-b // 16) * q["group_bytes"] <= pl["work_bytes"]


def test_ranges_depend_on_the_32_fit_group_count_only():
    from sglm_hip import engine as E
    for n in (5000, 1_000_000):
        a, b = E.lag_xtr_plan(n, 33, 40, 2048), E.lag_xtr_plan(n, 64, 40, 2048)
        assert all(a[k] == b[k] for k in ("U", "H", "ntiles", "nranges", "tiles_per"))
    big = E.lag_xtr_plan(1_000_000, 120, 40, 2048)
    assert big["nranges"] > 1 and big["ntiles"] == -(-(1_000_000 + big["H"]) // big["U"])


def test_uncovered_shapes():
    from sglm_hip import _lib
    assert _lib.query("sglm_lag_xtr_packed_ok", 50, 40, -20, 19) == 1
    assert _lib.query("sglm_lag_xtr_packed_ok", 65, 40, -20, 19) == 0     # events
    assert _lib.query("sglm_lag_xtr_packed_ok", 50, 41, -20, 20) == 0     # lags
    assert _lib.query("sglm_lag_xtr_packed_ok", 50, 40, -20, 21) == 0     # a gap in the shifts
    out = np.zeros(7, dtype=np.int64)
    with pytest.raises(_lib.HipEngineError):
        _lib.call("sglm_lag_xtr_plan", 1000, 4, 41, 2048, out.ctypes.data)
