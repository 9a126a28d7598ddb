"""Seeded inputs, np.longdouble references and derived bounds for the mixed-block kernels of
csrc/mixed.hip (CPU only: numpy).  Shared by tests/test_gpu_mixed_kernels.py (the kernels on the
MI355X) and tests/test_mixed_cases_cpu.py (the sanity checks of the inputs and bounds).

Bounds (derived, not measured).  A float64 sum of m products formed with FMAs, in any order,
errs by at most gamma_m sum|term| ~ m 2^-53 sum|term|; the Gram kernel rounds w * a once more
before the FMA and the packed pieces are added exactly (three bf16 values within 2^53 of each
other), which the + 8 covers:

    |got - ref| <= (m + 8) 2^-53 sum|term|                      (sum_bound)

The predictor adds K = k + 1 terms (the stored f32 eta and k products) in float64 and rounds
the sum to f32 once:

    |got - ref| <= 2^-24 |ref| + (K + 8) 2^-53 sum|term|        (eta_bound)

The references are np.longdouble sums (64-bit significand on x86-64) of the exact input values.
"""
from functools import lru_cache

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
SENT = -7.25                      # finite sentinel of the "not written elsewhere" checks
GUARD = 4096                      # bytes of sentinel behind the work buffer
P = 256
CPOS9 = (200, 3, 77, 4, 130, 255, 0, 19, 64)       # unsorted design positions, k <= 9


def have_longdouble():
    """np.longdouble carries at least 11 bits more than float64 (x87 extended or wider)."""
    return np.finfo(LD).nmant >= 63


def cpos_for(k, P=P):
    """k distinct, unsorted design positions < P (the fixed list first)."""
    if k <= len(CPOS9):
        return np.array(CPOS9[:k], dtype=np.int32)
    rest = np.setdiff1d(np.arange(P), CPOS9)
    rest = np.random.default_rng(1000 + k).permutation(rest)
    return np.concatenate([CPOS9, rest[:k - len(CPOS9)]]).astype(np.int32)


def signed_mags(rng, shape, span=10.0):
    """Mixed signs, magnitudes log-uniform over 2^-span .. 2^span (float64)."""
    return rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-span, span, size=shape))


# ------------------------------------------------------------------------------ bf16
def f32_to_bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of finite float32 values."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))
    return (r >> np.uint32(16)).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split3(R):
    """uint16 [3][...]: hi = bf16(R), mid = bf16(R - hi), lo = bf16(R - hi - mid) (f32
    subtractions, exact): hi + mid + lo == R for normal f32 R."""
    R = np.asarray(R, dtype=np.float32)
    hi = f32_to_bf16_bits(R)
    r1 = R - bf16_bits_to_f32(hi)
    mid = f32_to_bf16_bits(r1)
    r2 = r1 - bf16_bits_to_f32(mid)
    lo = f32_to_bf16_bits(r2)
    return np.stack([hi, mid, lo])


# ------------------------------------------------------------------------------ references
def sum_bound(m, sabs):
    return (m + 8) * U53 * np.asarray(sabs, dtype=np.float64)


def eta_bound(K, ref, sabs):
    ref, sabs = np.asarray(ref, dtype=np.float64), np.asarray(sabs, dtype=np.float64)
    return 2.0 ** -24 * np.abs(ref) + (K + 8) * U53 * sabs


def ratio(got, ref, bound):
    """max |got - ref| / bound with the difference taken in np.longdouble."""
    err = np.abs(np.asarray(got).astype(LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    return float(np.max(err / np.asarray(bound, dtype=np.float64)))


# ------------------------------------------------------------------------------ sglm_mixed_gram
GRAM_NS, GRAM_WSEL, GRAM_WROWS = 3, (4, 0, 2), 5
GRAM_CASES = [(n, k, wmode) for n in (5, 16389) for k in (1, 5, 9) for wmode in (0, 1)]


def pairs_gram(k):
    """The (c, c') lists of the upper triangle as Design._set_cont builds its ``pg``."""
    iu = np.triu_indices(k)
    return np.concatenate([iu[0], iu[1]]).astype(np.int32)


@lru_cache(maxsize=None)
def gram_case(n, k, wmode):
    """Inputs of one sglm_mixed_gram call and its reference: ref / bound [ns][npairs]."""
    rng = np.random.default_rng([11, n, k, wmode])
    ldc, ldw = n + 7, n + 13                          # ldw != ldc, both > n; junk past n
    C = signed_mags(rng, (k, ldc))
    if wmode == 0:
        W = signed_mags(rng, (GRAM_WROWS, ldw)).astype(np.float32)
    else:
        W = rng.integers(0, 4, (GRAM_WROWS, ldw)).astype(np.uint8)
    pg = pairs_gram(k)
    npairs = k * (k + 1) // 2
    ref = np.zeros((GRAM_NS, npairs), LD)
    sabs = np.zeros((GRAM_NS, npairs), LD)
    for s, row in enumerate(GRAM_WSEL):
        w = W[row, :n].astype(np.float64)
        for c in range(k):
            q = np.flatnonzero(pg[:npairs] == c)
            T = (w.astype(LD) * C[c, :n].astype(LD))[None, :] * C[pg[npairs + q], :n].astype(LD)
            ref[s, q], sabs[s, q] = T.sum(axis=1), np.abs(T).sum(axis=1)
    return dict(n=n, k=k, wmode=wmode, ldc=ldc, ldw=ldw, C=C, W=W, pg=pg, npairs=npairs,
                cpos=cpos_for(k), ref=ref, bound=sum_bound(n, sabs))


def gram_float64(case):
    """The same sums by plain float64 np.dot (the CPU sanity check of the bound)."""
    n, k, npairs, pg = case["n"], case["k"], case["npairs"], case["pg"]
    out = np.zeros((GRAM_NS, npairs))
    for s, row in enumerate(GRAM_WSEL):
        w = case["W"][row, :n].astype(np.float64)
        for q in range(npairs):
            out[s, q] = np.dot(w * case["C"][pg[q], :n], case["C"][pg[npairs + q], :n])
    return out


# ------------------------------------------------------------------------------ sglm_mixed_xtr
XTR_RROWS, XTR_GROWS, XTR_BP = 16, 20, 16
XTR_RSEL = (13, 2, 7, 0, 15, 9, 4, 11, 6, 1, 14)      # a permutation with gaps into 16 rows of R
XTR_GSLOTS = (17, 3, 8, 0, 19, 5, 12, 1, 14, 10, 6)   # into 20 rows of g
XTR_CASES = [(mode, n, k, nq, False) for mode in (0, 2, 3) for n in (3, 33795) for k in (1, 5)
             for nq in (1, 11)] + [(2, 33795, 5, 11, True)]


def pairs_xtr(k):
    """Design._set_cont's ``px``: {0 .. k-1, k .. k}."""
    return np.concatenate([np.arange(k), np.full(k, k)]).astype(np.int32)


@lru_cache(maxsize=None)
def xtr_case(mode, n, k, nq, indep=False):
    """Inputs of one sglm_mixed_xtr call.  R: f32 [16][ldr] (mode 0), uint16 bf16 bits
    [3][16][ldr] (mode 2: successive roundings of an f32 R, or with ``indep`` three independent
    bf16 planes), uint16 [16][ldr] (mode 3).  Rows n .. ldr of R hold finite non-zero junk, rows
    n .. ldc of C zeros (the engine's layout).  ref / bound [nq][k]."""
    rng = np.random.default_rng([12, mode, n, k, nq, int(indep)])
    n4 = (n + 3) // 4 * 4
    ldr, ldc = n4 + 4, n4 + 8
    C = np.zeros((k, ldc))
    C[:, :n] = signed_mags(rng, (k, n))
    Rf = signed_mags(rng, (XTR_RROWS, ldr)).astype(np.float32)        # junk past n included
    if mode == 0:
        R, val = Rf, Rf.astype(LD)
    elif mode == 3:
        R = f32_to_bf16_bits(Rf)
        val = bf16_bits_to_f32(R).astype(LD)
    else:
        R = split3(Rf)
        if indep:
            R[1] = f32_to_bf16_bits(signed_mags(rng, Rf.shape).astype(np.float32))
            R[2] = f32_to_bf16_bits(signed_mags(rng, Rf.shape).astype(np.float32))
        pl = bf16_bits_to_f32(R).astype(LD)
        val = (pl[0] + pl[1]) + pl[2]                  # the contract: hi + mid + lo
    rsel = np.array(XTR_RSEL[:nq], dtype=np.int32)
    ref = np.zeros((nq, k), LD)
    sabs = np.zeros((nq, k), LD)
    Cl = C[:, :n].astype(LD)
    for q in range(nq):
        T = Cl * val[rsel[q], :n][None, :]
        ref[q], sabs[q] = T.sum(axis=1), np.abs(T).sum(axis=1)
    return dict(mode=mode, n=n, k=k, nq=nq, ldr=ldr, ldc=ldc, C=C, R=R, Rf=Rf, val=val, rsel=rsel,
                gslots=np.array(XTR_GSLOTS[:nq], dtype=np.int32), cpos=cpos_for(k),
                px=pairs_xtr(k), ref=ref, bound=sum_bound(n, sabs))


def xtr_float64(case):
    n = case["n"]
    v = case["val"][case["rsel"], :n].astype(np.float64)     # exact: <= 24 (or 3 x 8) bits
    return v @ case["C"][:, :n].T


# ------------------------------------------------------------------------------ sglm_mixed_eta
ETA_N, ETA_LDC = 16389, 16392
# (name, k, nb, eta rows, ld): (a) the grouped kernel (k <= 64, strides % 4 == 0), with a capped
# grid at nb = 1024; (b) the fallback by k; (c) the fallback by stride
ETA_CASES = [("eta4-k1", 1, 11, 16, 16392), ("eta4-k5", 5, 11, 16, 16392),
             ("eta4-k64", 64, 11, 16, 16392), ("eta4-gridstride", 5, 1024, 1024, 16392),
             ("fallback-k65", 65, 3, 16, 16392), ("fallback-ld", 5, 11, 16, 16391)]


@lru_cache(maxsize=None)
def eta_case(name):
    """Inputs of one sglm_mixed_eta call: C [k][ldc] (junk past n), beta f32 [rows][P] (junk
    outside cpos), eta0 f32 [rows][ld] (random, junk past n), slots (a permutation prefix)."""
    _, k, nb, rows, ld = next(c for c in ETA_CASES if c[0] == name)
    rng = np.random.default_rng([13, k, nb, ld])
    C = signed_mags(rng, (k, ETA_LDC))
    beta = signed_mags(rng, (rows, P)).astype(np.float32)
    eta0 = signed_mags(rng, (rows, ld)).astype(np.float32)
    slots = rng.permutation(rows)[:nb].astype(np.int32)
    return dict(name=name, k=k, nb=nb, rows=rows, ld=ld, ldc=ETA_LDC, n=ETA_N, C=C, beta=beta,
                eta0=eta0, slots=slots, cpos=cpos_for(k))


def eta_ratio(case, got):
    """Worst error / bound of got [rows][ld] (f32) over the listed slots' rows < n, against the
    np.longdouble sum eta0 + sum_c C[c] beta[cpos[c]] (slots in chunks: the reference of 1024
    slots is not held at once).  sum|term| is a float64 sum: it only scales the bound."""
    n, k = case["n"], case["k"]
    Cl = case["C"][:, :n].astype(LD)
    Ca = np.abs(case["C"][:, :n])
    worst = 0.0
    for s0 in range(0, case["nb"], 64):
        sl = case["slots"][s0:s0 + 64]
        b = case["beta"][sl][:, case["cpos"]].astype(np.float64)          # [chunk][k]
        e0 = case["eta0"][sl, :n]
        ref = e0.astype(LD)
        for c in range(k):
            ref += b[:, c].astype(LD)[:, None] * Cl[c][None, :]
        sabs = np.abs(e0).astype(np.float64) + np.abs(b) @ Ca
        worst = max(worst, ratio(got[sl, :n], ref, eta_bound(k + 1, ref, sabs)))
    return worst


def eta_float64(case):
    """eta0 + beta C by float64 np.dot, rounded to f32 once (listed slots; others unchanged)."""
    n = case["n"]
    out = case["eta0"].copy()
    sl = case["slots"]
    b = case["beta"][sl][:, case["cpos"]].astype(np.float64)
    e64 = case["eta0"][sl, :n].astype(np.float64) + b @ case["C"][:, :n]
    out[sl, :n] = e64.astype(np.float32)
    return out


# ------------------------------------------------------------------------------ through Design
DESIGN_N, DESIGN_NBIN = 9003, 12


@lru_cache(maxsize=None)
def design_case(k):
    """Host design of DESIGN_N rows: 12 random 0/1 columns and k well-conditioned continuous
    columns (z-scored smooth signals of distinct frequencies plus noise, stored f32-exact)
    interleaved at scattered positions.  Responses for a Gaussian and a Poisson fit."""
    rng = np.random.default_rng([14, k])
    n, p = DESIGN_N, DESIGN_NBIN + k
    pos = rng.permutation(p)[:k]                       # unsorted; the design reports them sorted
    t = np.arange(n) / n
    X = (rng.random((n, p)) < 0.3).astype(np.float64)
    for j, c in enumerate(pos):
        s = np.sin(2 * np.pi * (1.5 + 0.75 * j) * t + rng.uniform(0, 2 * np.pi))
        s = s + 0.5 * rng.normal(size=n)
        X[:, c] = ((s - s.mean()) / s.std()).astype(np.float32)
    w = rng.normal(0, 0.3, p)
    y = X @ w + 0.7 + rng.normal(0, 0.5, n)
    yp = rng.poisson(np.exp(0.3 * (X @ w) - 0.2)).astype(np.float64)
    return dict(k=k, n=n, p=p, X=X, cpos=np.sort(pos), y=y, ypois=yp)
