"""The event-structured weighted Gram (sglm_lag_gram_w, csrc/lagw.hip) and the dense bit-plane
Gram (sglm_syrk_cbits) against a float64 Gram built without any project kernel.

Reference: X is filled in numpy by plain indexing, X[t, (b, a)] = E[t + row0 - shifts[b], a] (0
outside E), the ones column at d.p, in the column order of Design.from_events; the weights are
rounded to bf16 and H64 = X^T diag(wb) X, C = X^T diag(wb != 0) X are float64 matmuls (C[i, j] =
the number of non-zero terms of H64[i, j]).

Bound, per entry of the upper triangle i <= j <= d.p: the kernels sum the exact products
bf16(w) * {0, 1} in f32; every term is >= 0, so any summation order of k = C[i, j] terms is within
(k - 1) 2^-24 H64[i, j] with round-to-nearest adds, one more add for a split piece's second half:
|H - H64| <= 2 (C + 2) 2^-24 H64 (the factor 2: one ulp per MFMA accumulation step instead of
half).  C == 0: exactly 0.  Columns j > d.p of the upper triangle: exactly 0.  H[p][p] (the
tree-summed weights): the same bound, k = the non-zero weights.  Integer weights 0..3 (sums below
2^24): H == H64 exactly.  H is NaN-filled and the fit slots are non-contiguous: unlisted slots
stay NaN.  The strictly lower triangle of a listed slot is workspace.

Worst err / bound measured on the MI355X over all cases (each test prints its own):
sglm_lag_gram_w 0.295 (case k, 5 fits), sglm_syrk_cbits 0.250 (case h).
"""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_laggram_w import _dense

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
WORST = {"lag": 0.0, "dense": 0.0}


@pytest.fixture(scope="module")
def torch_mod(engine):
    import torch
    return torch


def _events(rng, N, m, rho=0.03):
    """0/1 events at density rho; the first and the last event also occur on the first and the
    last raw row."""
    E = (rng.random((N, m)) < rho).astype(np.float32)
    for a in (0, m - 1):
        E[[0, N - 1], a] = 1
    return E


def _window(N, shifts):
    """(row0, n): the largest design whose every source row lies in E, so that the first and the
    last raw row are read."""
    row0 = max(0, max(shifts))
    return row0, N - row0 + min(0, min(shifts))


def _ref_X(E, shifts, row0, n, event_major, kx=0, rows=None):
    """float64 [n][K m + kx + 1]: the lag columns by plain indexing, kx zero columns in the
    place of a mixed design's continuous ones (the structured call leaves them 0), the ones
    column last; ``rows`` = (a, b): that row slab."""
    N, m = E.shape
    K = len(shifts)
    X = np.zeros((n, K * m + kx + 1))
    t = np.arange(n)
    for b, s in enumerate(shifts):
        src = t + row0 - s
        ok = np.flatnonzero((src >= 0) & (src < N))
        cols = np.arange(m) * K + b if event_major else b * m + np.arange(m)
        X[np.ix_(ok, cols)] = E[src[ok]]
    X[:, K * m + kx] = 1.0
    return X if rows is None else X[rows[0]:rows[1]]


def _float_weights(rng, n):
    """Zero on ~30 % of the rows, else exp(U), U uniform on [ln 1e-6, ln 1e4]."""
    w = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), n))
    return (w * (rng.random(n) >= 0.3)).astype(np.float32)


def _int_weights(rng, n):
    return rng.integers(0, 4, n).astype(np.float32)


def _reference(torch, Xd, W, fits, n):
    """{slot: (H64, C)} on the device."""
    out = {}
    for k in fits:
        wb = W[k, :n].to(torch.bfloat16).double()
        out[k] = (Xd.T @ (Xd * wb[:, None]), Xd.T @ (Xd * (wb != 0).double()[:, None]))
    return out


def _check(torch, tag, H, ref, fits, p, exact):
    """The per-entry assertions on H [slots][P][P] (f32, device) for the listed slots; returns
    the worst err / bound."""
    P = H.shape[1]
    up = torch.triu(torch.ones((p + 1, p + 1), dtype=torch.bool, device=H.device))
    pad = torch.triu(torch.ones((P, P), dtype=torch.bool, device=H.device))[:, p + 1:]
    worst = 0.0
    for k in fits:
        H64, C = ref[k]
        h = H[k, :p + 1, :p + 1].double()[up]
        r, c = H64[up], C[up]
        assert bool(torch.isfinite(h).all()), (tag, k, "non-finite entry in the upper triangle")
        assert bool((H[k][:, p + 1:][pad] == 0).all()), (tag, k, "padding columns not zero")
        if exact:
            bad = torch.nonzero(h != r)[:5].flatten().tolist()
            assert not bad, (tag, k, "integer weights not exact", bad, h[bad].tolist(),
                             r[bad].tolist())
            continue
        zero = c == 0
        assert bool((h[zero] == 0).all()), (tag, k, "entry without a term is not exactly 0")
        ratio = torch.where(zero, torch.zeros_like(r),
                            (h - r).abs() / (2.0 * (c + 2.0) * U24 * r).clamp_min(1e-300))
        q = int(torch.argmax(ratio))
        worst = max(worst, float(ratio[q]))
        assert float(ratio[q]) <= 1.0, (tag, k, "err / bound", float(ratio[q]), "H", float(h[q]),
                                        "H64", float(r[q]), "terms", float(c[q]))
    return worst


def _run(engine, torch, tag, E, shifts, nf, seed, row0=None, n=None, event_major=False,
         slab=None, extra=None, wf_rows=None, dense=False, launch=None):
    """One design: integer and float weights through engine._lag_gram_w (and the dense Gram when
    ``dense``) against the float64 reference.  ``wf_rows``: the float weight rows instead of the
    default; ``launch``: a list of callables, each run before one more launch of the same
    weights (environment settings read per launch).  Returns (design, structure)."""
    rng = np.random.default_rng(seed)
    if row0 is None:
        row0, n = _window(E.shape[0], shifts)
    d = engine.Design.from_events(E, shifts, row0, n, event_major=event_major, slab=slab,
                                  extra=extra)
    lg = engine._lagw(d)
    assert lg is not None, tag
    kx = 0 if extra is None else int(extra.shape[0])
    assert d.p == len(shifts) * E.shape[1] + kx
    Xd = torch.from_numpy(_ref_X(E, shifts, row0, n, event_major, kx, slab)).cuda()
    assert Xd.shape == (d.n, d.p + 1)
    fits = [2 * k + 1 for k in range(nf)]                 # non-contiguous slots
    nslot = 2 * nf + 1
    fits_h = np.asarray(fits, dtype=np.int32)
    for exact in (True, False):
        W = torch.zeros((nslot, d.ld), dtype=torch.float32, device="cuda")
        for q, k in enumerate(fits):
            row = (_int_weights(rng, d.n) if exact else
                   wf_rows[q] if wf_rows is not None else _float_weights(rng, d.n))
            W[k, :d.n] = torch.from_numpy(np.asarray(row, dtype=np.float32))
        ref = _reference(torch, Xd, W, fits, d.n)
        for pre in (launch or [lambda: None]):
            pre()
            bf = SimpleNamespace(W=W, H=torch.full((nslot, d.P, d.P), float("nan"),
                                                   dtype=torch.float32, device="cuda"))
            engine._lag_gram_w(d, lg, bf, fits_h, 0)
            torch.cuda.synchronize()
            for k in range(0, nslot, 2):
                assert bool(torch.isnan(bf.H[k]).all()), (tag, k, "unlisted slot written")
            w = _check(torch, tag, bf.H, ref, fits, d.p, exact)
            if not exact:
                WORST["lag"] = max(WORST["lag"], w)
                print(f"\n[hessian_f64] {tag}: sglm_lag_gram_w worst err/bound {w:.3f}")
        if dense:
            w = _check(torch, tag + " dense", _dense(engine, torch, d, W, fits), ref, fits, d.p,
                       exact)
            if not exact:
                WORST["dense"] = max(WORST["dense"], w)
                print(f"[hessian_f64] {tag}: sglm_syrk_cbits worst err/bound {w:.3f}")
    return d, lg


@pytest.mark.parametrize("tag,m,shifts,nf,dense", [
    ("a", 31, list(range(-3, 3)), 3, True),       # m + 1 == 32: one event half, full
    ("b", 32, list(range(-3, 3)), 3, False),      # the ones bit alone in the second half
    ("c", 63, list(range(0, 4)), 2, False),       # the ABI's maximum m
    ("d", 1, [0], 1, False),                      # K = 1, the smallest P
    ("e", 5, [0], 7, False),                      # K = 1, several fits
    ("f1", 6, list(range(-8, 8)), 4, False),      # nf K = 64: the last launch with NT = 2
    ("f2", 6, list(range(-6, 7)), 5, False),      # nf K = 65: the first with NT = 4
])
def test_shapes(engine, torch_mod, tag, m, shifts, nf, dense):
    rng = np.random.default_rng(100 + m + nf)
    E = _events(rng, 4000, m, 0.05 if m == 1 else 0.03)
    _run(engine, torch_mod, tag, E, shifts, nf, seed=200 + m, dense=dense)
    if tag in ("f1", "f2"):
        assert nf * len(shifts) == (64 if tag == "f1" else 65)


def test_natural_order_launch(engine, torch_mod):
    """Case g: more than 128 piece types (Gm Gy = 6 x 22 = 132), so lagw_plan builds no job list
    and the blocks run the piece types in natural order."""
    m, shifts, nf = 2, list(range(-48, 48)), 29
    K, NH, MB = len(shifts), 1 if m + 1 <= 32 else 2, 16      # 8 waves x 2 M tiles
    NN = 64 if nf * K <= 64 else 128
    Gm, Gy = -(-K * NH // MB), -(-nf * K // NN)
    assert (Gm, Gy) == (6, 22) and Gm * Gy > 128
    rng = np.random.default_rng(7)
    d, _ = _run(engine, torch_mod, "g", _events(rng, 3000, m), shifts, nf, seed=8)
    assert d.P == 256


H_COUNTS = [0, 1, 2, 127, 128, 129, 255, 256, 257]


def _events_h(rng, N):
    """Case h: per event 0 / 1 / 2 / 127 / 128 / 129 / 255 / 256 / 257 occurrences (the edges of
    the 128-occurrence stages and of the pair-interleaved words), one event on every raw row, two
    random events at 3 %."""
    E = np.zeros((N, 12), dtype=np.float32)
    for a, c in enumerate(H_COUNTS):
        rows = rng.choice(np.arange(1, N - 1), max(0, c - 2), replace=False) if c > 2 else []
        E[rows, a] = 1
        E[[0, N - 1][:min(c, 2)], a] = 1
    E[:, 9] = 1
    E[:, 10:] = rng.random((N, 2)) < 0.03
    return E


@pytest.mark.parametrize("event_major", [False, True])
def test_stage_and_pair_edges(engine, torch_mod, event_major):
    rng = np.random.default_rng(31)
    N = 4000
    E = _events_h(rng, N)
    assert E.mean() <= engine.LAG_GRAM_W_MAX_RHO
    shifts = list(range(5, -7, -1)) if event_major else list(range(-6, 6))
    d, lg = _run(engine, torch_mod, "h" + ("-em" if event_major else ""), E, shifts, 5,
                 seed=32, event_major=event_major, dense=not event_major)
    cnt = np.diff(lg.w_ev_off.cpu().numpy())
    assert list(cnt[:9]) == H_COUNTS and cnt[9] == N          # every occurrence is iterated


@pytest.mark.parametrize("slab", [None, (1000, 2500)])
def test_window_edges(engine, torch_mod, slab):
    """Case i: raw rows on both sides of the design rows (the w_occ filter of engine._lagw), one
    event on the first and last raw rows and on the K raw rows either side of both ends of the
    window of raw rows the design reads -- the whole design's and the slab's."""
    rng = np.random.default_rng(41)
    N, m, shifts, row0, n = 4000, 7, list(range(-5, 4)), 40, 3800
    K, smin, smax = len(shifts), min(shifts), max(shifts)
    assert row0 > smax and n < N - row0 - smax
    E = _events(rng, N, m)
    E[:, 0] = 0
    E[[0, 1, N - 2, N - 1], 0] = 1
    for a, b in ((0, n), (1000, 2500)):
        for end in (row0 + a - smax, row0 + b - 1 - smin):    # first / last raw row read
            E[end - K:end + K + 1, 0] = 1
    d, lg = _run(engine, torch_mod, "i" + ("-slab" if slab else ""), E, shifts, 3, seed=42,
                 row0=row0, n=n, slab=slab, dense=True)
    assert d.n == (n if slab is None else 1500)
    assert int(lg.w_occ.numel()) < int(lg.occ.numel())


def test_weights(engine, torch_mod):
    """Case j: weights over ten decades with ~30 % zeros, a fit with every weight zero and a
    fit whose only non-zero weights sit on the first and the last design row."""
    rng = np.random.default_rng(51)
    N, m, shifts = 4000, 10, list(range(-4, 4))
    _, n = _window(N, shifts)
    ends = np.zeros(n, dtype=np.float32)
    ends[0], ends[-1] = 3.14159, 1e-3
    rows = [_float_weights(rng, n), _float_weights(rng, n), np.zeros(n, np.float32), ends]
    _run(engine, torch_mod, "j", _events(rng, N, m), shifts, 4, seed=52, wf_rows=rows)


@pytest.mark.parametrize("nf", [1, 5])
def test_c4_layout_split_and_window(engine, torch_mod, monkeypatch, nf):
    """Case k: the C4 layout (m = 50, 40 shifts: two event halves, 2000 columns) with and without
    the load-balancing split (second halves added by the symmetrize pass: events of up to six
    stages, so the second halves hold terms) and with every piece's column window at its block's
    first column (SGLM_LAGW_WSHIFT=0)."""
    rng = np.random.default_rng(61)
    N, m, shifts = 6000, 50, list(range(-20, 20))
    E = (rng.random((N, m)) < np.linspace(0.005, 0.12, m)[None, :]).astype(np.float32)
    E[[0, N - 1], 0] = 1
    assert E.sum(0).max() > 4 * 128

    def env(split, wshift):
        def pre():
            monkeypatch.setenv("SGLM_LAGW_SPLIT", split)
            monkeypatch.setenv("SGLM_LAGW_WSHIFT", wshift)
        return pre
    _run(engine, torch_mod, f"k-{nf}", E, shifts, nf, seed=62,
         launch=[env("1", "1"), env("0", "1"), env("1", "0")])


def test_mixed_design_lag_block(engine, torch_mod):
    """Case l: case h with two continuous columns (pones > K m).  After the structured call
    alone the lag and ones block holds the bound and every upper-triangle entry of a continuous
    row or column is exactly 0 (the reference's columns there are zero: no term)."""
    rng = np.random.default_rng(71)
    N, shifts = 4000, list(range(-6, 6))
    E = _events_h(rng, N)
    _, n = _window(N, shifts)
    d, lg = _run(engine, torch_mod, "l", E, shifts, 5, seed=72, extra=rng.normal(0, 1, (2, n)))
    assert d.cont is not None and d.p == lg.K * lg.m + 2


def test_report_worst_ratio():
    """The worst err / bound of the cases above (printed; below 1 by their assertions)."""
    print(f"\n[hessian_f64] worst err/bound: sglm_lag_gram_w {WORST['lag']:.3f}, "
          f"sglm_syrk_cbits {WORST['dense']:.3f}")
    assert WORST["lag"] <= 1.0 and WORST["dense"] <= 1.0
