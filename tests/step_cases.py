"""Inputs and oracles for the mask-sum and step-control kernels of csrc/api.hip:
sglm_mask_stats, sglm_eta_axpy_max, sglm_aa_step and sglm_step_decide.  numpy only (float64 /
longdouble), nothing from sglm_hip.

`decide_oracle` is a transcription of the host rule of engine.irls (the stage-1 Armijo block, the
scale / prop / relv block and the stop rules) in the host's operand order, written here and not
imported; for a fit whose stage-1 search fails it returns what the header documents for the
kernel (step 0, relv = prop = 0, flags 256 | 512, a packed-R row reserved): the host's stage 2
decides those."""
import functools

import numpy as np

LD = np.longdouble
U32 = 2.0 ** -24


def pad256(n):
    return (n + 255) // 256 * 256


# ---- sglm_mask_stats ------------------------------------------------------------------------
MS_N = (1, 255, 8191, 8192, 8193, 3 * 8192 + 5)            # the row chunk is 8192
MS_POWERS = (-1.0, 0.0, 1.0, 1.5, 2.0, 3.0)
MS_BAR = 1e-12         # test_gpu_nb2ml_kernels.py's bar for the same two-level fixed-order sums


@functools.lru_cache(maxsize=None)
def mask_stats_case(n, positive):
    """M uint8 [4][ldm] (random 0/1; multiplicities in {0, 2, 3}; all zero; only the last row;
    the padding rows [n, ldm) are 1 and must not be read), Y [2][n] (1e6 + N(0,1) with K = its
    mean; counts with exact zeros and K = 0 -- shifted up by 0.5 when `positive`), K."""
    rng = np.random.default_rng(40 + n)
    ldm = pad256(n)
    M = np.ones((4, ldm), dtype=np.uint8)
    M[0, :n] = rng.integers(0, 2, n)
    M[1, :n] = rng.choice(np.array([0, 2, 3], dtype=np.uint8), n)
    M[2, :n] = 0
    M[3, :n] = 0
    M[3, n - 1] = 1
    Y = np.zeros((2, n))
    Y[0] = 1e6 + rng.normal(size=n)
    Y[1] = rng.poisson(1.2, n).astype(np.float64) * rng.choice([1.0, 0.5, 2.25], n)
    if positive:
        Y[1] += 0.5
    elif n > 1:
        assert (Y[1] == 0).any()
    K = np.array([Y[0].mean(), 0.0])
    for a in (M, Y, K):
        a.setflags(write=False)
    return M, Y, K


def tweedie_const(power, y):
    """half-Tweedie loss constant (sklearn constant_to_optimal_zero), longdouble"""
    y = y.astype(LD)
    if power == 0:
        return -y * y / 2
    if power == 1:
        out = -y.copy()
        pos = y > 0
        out[pos] += y[pos] * np.log(y[pos])
        return out
    if power == 2:
        return -np.log(y) - 1
    pw = LD(power)
    return np.power(np.maximum(y, 0), 2 - pw) / (1 - pw) / (2 - pw)


def mask_stats_oracle(M, Y, K, n, power):
    """(ref [R][F][5], mag [R][F][3]): count, sum m (y - K), sum m (y - K)^2, sum m c(y) (0 for
    power < 0), min over m > 0 of y (+inf for an empty mask), summed in longdouble row by row;
    mag = sum m |term| of the three real sums."""
    R, F = Y.shape[0], M.shape[0]
    ref = np.zeros((R, F, 5), dtype=LD)
    mag = np.zeros((R, F, 3), dtype=LD)
    for r in range(R):
        y = Y[r].astype(LD)
        d = y - LD(K[r])
        c = tweedie_const(power, Y[r]) if power >= 0 else np.zeros(n, dtype=LD)
        for f in range(F):
            on = np.flatnonzero(M[f, :n])
            m = M[f, on].astype(LD)
            terms = (m * d[on], m * d[on] * d[on], m * c[on])
            ref[r, f, 0] = m.sum()
            for k in range(3):
                ref[r, f, 1 + k] = terms[k].sum()
                mag[r, f, k] = np.abs(terms[k]).sum()
            ref[r, f, 4] = y[on].min() if on.size else LD(np.inf)
    return ref, mag


# ---- sglm_eta_axpy_max ------------------------------------------------------------------------
EA_N = (1, 255, 262144 + 77)            # the last: more than 1024 blocks of 256 rows (stride loop)
EA_STEP = np.array([0.5, 0.0, -1.0], dtype=np.float32)
EA_FIT_MASK = np.array([1, 0, 1], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def eta_axpy_case(n):
    """ld, eta [4][ld] f32 (row 3 and the rows [n, ld) of every fit are sentinels that no call
    may change), deta [3][ld] (NaN past n), M uint8 [2][ld] with multiplicities 0..2 (1 past
    n).  The largest |deta| of each fit sits on a row its mask leaves out."""
    rng = np.random.default_rng(60 + n)
    ld = pad256(n) + 256
    eta = rng.normal(0, 3, (4, ld)).astype(np.float32)
    deta = np.full((3, ld), np.nan, dtype=np.float32)
    deta[:, :n] = rng.normal(0, 1, (3, n)).astype(np.float32)
    M = np.ones((2, ld), dtype=np.uint8)
    M[:, :n] = rng.integers(0, 3, (2, n))
    if n > 1:
        for k in range(3):
            i = int(rng.integers(0, n))
            deta[k, i] = 50.0
            M[EA_FIT_MASK[k], i] = 0
        M[:, n - 1] = 2                                     # the last row counts
    for a in (eta, deta, M):
        a.setflags(write=False)
    return ld, eta, deta, M


def eta_axpy_oracle(n, eta, deta, M):
    """(eta64 [3][n], bound, dmax f32 [3]): eta + t deta in float64 with 2^-23 (|eta| + |t deta|)
    (the add may contract into an fma), dmax = max over mask rows of |fl32(t * deta)| exactly."""
    e64 = np.zeros((3, n))
    bound = np.zeros((3, n))
    dmax = np.zeros(3, dtype=np.float32)
    for k in range(3):
        t = EA_STEP[k]
        dv = (t * deta[k, :n]).astype(np.float32)           # one f32 product
        e64[k] = eta[k, :n].astype(np.float64) + np.float64(t) * deta[k, :n].astype(np.float64)
        bound[k] = 2.0 ** -23 * (np.abs(eta[k, :n]).astype(np.float64)
                                 + np.abs(np.float64(t) * deta[k, :n].astype(np.float64)))
        rows = M[EA_FIT_MASK[k], :n] > 0
        if t != 0 and rows.any():
            dmax[k] = np.abs(dv[rows]).max()
    return e64, bound, dmax


# ---- sglm_aa_step ---------------------------------------------------------------------------
AA_SHAPES = ((64, 1), (256, 255), (512, 300))
AA_NSLOT = 9
AA_SLOTS = np.array([7, 0, 3, 8, 5, 2], dtype=np.int32)
AA_KINDS = ("accepted", "gamma>0.5", "gamma<-2", "raw_prev==f", "g.d>=0", "sel=0")
AA_SEL = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)
AA_TPREV = np.array([1.0, 0.5, 0.25, 1.0, 1.0, 0.5], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def aa_case(P, p):
    """delta, raw_prev, used_prev f32 [9][P], gtot f64 [9][P], rm f32 [9][2]; rows of the slots
    1, 4, 6 no fit names are NaN.  Fit q (slot AA_SLOTS[q]) is of AA_KINDS[q]: df = s (f + r)
    with |r| = |f| gives gamma = df.f / df.df = 1 / (2 s): s = -2, 0.5, -0.1 for gamma = -0.25
    (accepted), 1 and -5; gtot = -(the corrected direction) + noise makes g.d < 0 clearly."""
    rng = np.random.default_rng(80 + P + p)
    f32 = np.float32
    delta = np.full((AA_NSLOT, P), np.nan, dtype=f32)
    raw = np.full((AA_NSLOT, P), np.nan, dtype=f32)
    used = np.full((AA_NSLOT, P), np.nan, dtype=f32)
    gtot = np.full((AA_NSLOT, P), np.nan)
    rm = np.full((AA_NSLOT, 2), np.nan, dtype=f32)
    acc = None
    for q, kind in enumerate(AA_KINDS):
        k = AA_SLOTS[q]
        if kind == "g.d>=0":                                # the accepted fit, gtot negated
            delta[k], raw[k], used[k], gtot[k] = delta[acc], raw[acc], used[acc], -gtot[acc]
            continue
        f = rng.normal(0, 1, P)
        r = rng.normal(0, 1, P)
        r *= np.linalg.norm(f) / np.linalg.norm(r)
        s = {"accepted": -2.0, "gamma>0.5": 0.5, "gamma<-2": -0.1}.get(kind, -2.0)
        delta[k] = f.astype(f32)
        raw[k] = (f - s * (f + r)).astype(f32)
        if kind == "raw_prev==f":
            raw[k] = delta[k]
        used[k] = rng.normal(0, 1, P).astype(f32)
        fk = delta[k].astype(np.float64)
        df = fk - raw[k].astype(np.float64)
        db = used[k].astype(np.float64) * float(AA_TPREV[q])
        den = df @ df
        gam = (df @ fk) / max(den, 1e-30)
        dn = fk - gam * (db + df)
        gtot[k] = -dn + 0.3 * rng.normal(0, 1, P)
        if kind == "accepted":
            acc = k
    for a in (delta, raw, used, gtot, rm):
        a.setflags(write=False)
    return delta, raw, used, gtot, rm


def aa_oracle(P, p, delta, raw, used, gtot):
    """The header's definition in float64, per fit q: dict with f, dnew, good, gamma, den, ff,
    gd, the absolute sums of the three dots, and the bound on |d - dnew| of an accepted fit:
    each f32 dot is within k 2^-24 of its absolute sum, k = ceil(P / 256) + 10 (the per-thread
    fma chain, six shuffle adds, three LDS adds and the rounding of df), so
      |dgamma| <= k 2^-24 (sum|df f| + |gamma| df.df) / df.df,
      |d - dnew| <= |dgamma| |db + df| + 3 * 2^-24 (|f| + |gamma| |db + df|)
    (df, db, their sum and product, and the final subtraction: one rounding each)."""
    out = []
    kk = -(-P // 256) + 10
    for q in range(len(AA_SLOTS)):
        k = AA_SLOTS[q]
        f = delta[k].astype(np.float64)
        df = f - raw[k].astype(np.float64)
        db = used[k].astype(np.float64) * np.float64(AA_TPREV[q])
        den, num, ff = df @ df, df @ f, f @ f
        gam = num / max(den, 1e-30)
        dn = f - gam * (db + df)
        gd = gtot[k] @ dn
        good = bool(AA_SEL[q]) and den > 1e-12 * ff and -2.0 <= gam <= 0.5 and gd < 0
        dgam = kk * U32 * (np.abs(df * f).sum() + abs(gam) * den) / max(den, 1e-30)
        bound = dgam * np.abs(db + df) + 3 * U32 * (np.abs(f) + abs(gam) * np.abs(db + df))
        out.append(dict(f=f, dnew=dn, good=good, gamma=gam, den=den, ff=ff, gd=gd,
                        gd_abs=np.abs(gtot[k] * dn).sum(), bound=bound,
                        rm=(np.abs(delta[k][:p]).max() if p else np.float32(0),
                            np.abs(delta[k][p])) if AA_SEL[q] else (0.0, 0.0)))
    return out


# ---- sglm_step_decide -----------------------------------------------------------------------
SD_NA = (1, 5, 1024, 1025, 2050)
SD_NSLOT = 2100
SD_SIGMA, SD_TOL, SD_SFLOOR = 2.0 ** -11, 3e-6, 0.1
TS1 = np.array([0.0, 1.0, 0.5, 0.25, 0.125])
TV2 = np.array([0.0625, 0.03125, 0.015625, 0.0078125, 2.0 ** -10, 2.0 ** -14, 2.0 ** -20])
SD_KINDS = ("tix1 continue", "tix2 tol", "tix3 stagnation", "tix4 out of iterations", "no hit",
            "flat", "tix1 tol unless raw step", "tix2 stale no stagnation")


def decide_ts(nts):
    return TS1.copy() if nts == 5 else np.concatenate([TS1, TV2])


@functools.lru_cache(maxsize=None)
def decide_case(na, nts):
    """act (an injection into 2100 slots, not sorted), L [na][5], sc [na][6 + nts], aa_rm f32
    [2100][2], prev_rel, fresh, n_iter, max_iter.  Fit q is of SD_KINDS[kind[q]]."""
    rng = np.random.default_rng(90 + na + nts)
    ts = decide_ts(nts)
    act = rng.permutation(SD_NSLOT)[:na].astype(np.int32)
    kind = ((np.arange(na) * 5 + 2) % len(SD_KINDS)) if na > 1 else np.array([6])
    kind[-1] = 0 if na > 1 else 6          # the last fit takes a row (past 1024: the scan's carry)
    L = np.zeros((na, 5))
    sc = np.zeros((na, 6 + nts))
    aa_rm = rng.uniform(0, 1, (SD_NSLOT, 2)).astype(np.float32)    # rows of no fit: large
    prev_rel = np.zeros(na)
    fresh = np.zeros(na, dtype=np.uint8)
    n_iter = rng.integers(0, 20, na).astype(np.int32)
    max_iter = np.full(na, 100, dtype=np.int32)
    for q in range(na):
        kd = SD_KINDS[kind[q]]
        gdir = -rng.uniform(0.5, 5.0)
        A, B, C = rng.uniform(0, 3), rng.normal(0, 1), rng.uniform(0, 2)
        L0 = rng.uniform(100.0, 3000.0)
        tix = {"tix1": 1, "tix2": 2, "tix3": 3, "tix4": 4}.get(kd[:4], 0)
        if kd == "flat":
            A = B = C = 0.0
            L[q] = L0 * (1 + 2.0 ** -50)                    # above obj(0) by less than 1e-13
            L[q, 0] = L0
            tix = 1
        else:
            quad = A + 2 * ts[:5] * B + ts[:5] ** 2 * C
            dlt = -gdir * rng.uniform(0.1, 1.0, 5)          # positive: no Armijo, not flat
            if tix:
                dlt[tix] = 0.5 * ts[tix] * gdir             # half the slope: Armijo holds
                dlt[tix + 1:] = rng.normal(0, 1, 4 - tix)   # whatever comes later is not read
            dlt[0] = 0.0
            L[q] = L0 + dlt - 0.5 * (quad - quad[0])
        maxb = rng.uniform(0.03, 2.0, nts)                  # both sides of the floor 0.1
        step = ts[tix]
        want = 10.0 ** rng.uniform(-2.5, -0.5)              # relv of a fit that goes on
        if "tol" in kd:
            want = SD_TOL * rng.uniform(0.05, 0.8)
        if "stagnation" in kd:
            want = 10.0 ** rng.uniform(-5.0, -4.3)
        # relv = step * max(maxd / scale, maxdi): one of the two terms carries it
        per, scale = want / max(step, 0.125), max(maxb[tix], SD_SFLOOR)
        if q % 2:
            maxd, maxdi = 0.3 * per * scale, per            # the intercept's step carries it
        else:
            maxd, maxdi = per * scale, 0.3 * per            # the coefficients' step does
        fresh[q] = rng.integers(0, 2)
        prev_rel[q] = want * rng.uniform(2.5, 10.0)         # halved at least: no stagnation
        if "stagnation" in kd:
            prev_rel[q] = want * rng.uniform(0.8, 1.6)
            fresh[q] = 0 if kd.startswith("tix2 stale") else 1
        if kd == "tix4 out of iterations":
            n_iter[q] = max_iter[q] - 1
        k = act[q]
        aa_rm[k] = (maxd * rng.uniform(0, 0.5), maxdi * rng.uniform(0, 0.5))
        if kd == "tix1 tol unless raw step":
            aa_rm[k] = (rng.uniform(0.01, 0.1), 0.0) if q % 2 else (0.0, rng.uniform(1e-3, 0.1))
        sc[q, 0], sc[q, 1], sc[q, 2], sc[q, 3], sc[q, 4] = gdir, A, B, C, maxd
        sc[q, 5:5 + nts] = maxb
        sc[q, 5 + nts] = maxdi
    out = (act, L, sc, aa_rm, prev_rel, fresh, n_iter, max_iter, kind)
    for a in out:
        a.setflags(write=False)
    return out


def decide_oracle(act, L, sc, nts, ts, sigma, tol, sfloor, legacy, aa_rm, prev_rel, fresh,
                  n_iter, max_iter):
    """engine.irls' host rule, restated (same operand order as the host's numpy expressions)."""
    na = len(act)
    gdir, A_, B_, C_, maxd = sc[:, 0], sc[:, 1], sc[:, 2], sc[:, 3], sc[:, 4]
    maxb = sc[:, 5:5 + nts]
    maxdi = sc[:, 5 + nts]
    t1 = ts[:5]

    def objectives(Lm, tv):
        return Lm + 0.5 * (A_[:, None] + 2 * tv[None, :] * B_[:, None]
                           + tv[None, :] ** 2 * C_[:, None])
    step_a = np.zeros(na)
    tix = np.zeros(na, dtype=np.int64)
    obj = objectives(L, t1)
    armijo = obj[:, 1:] - obj[:, :1] <= sigma * t1[None, 1:] * gdir[:, None]
    flat = np.abs(obj[:, 1:] - obj[:, :1]) <= 1e-13 * np.abs(obj[:, :1])
    ok = armijo | flat
    first = np.argmax(ok, axis=1)
    hit = ok[np.arange(na), first]
    step_a[hit] = t1[1:][first[hit]]
    tix[hit] = 1 + first[hit]
    by_flat = hit & ~armijo[np.arange(na), first]           # taken by the flat branch alone
    if legacy:
        scale = 1.0 + maxb[np.arange(na), tix]
        prop = maxd / scale
    else:
        scale = np.maximum(maxb[np.arange(na), tix], sfloor)
        prop = np.maximum(maxd / scale, maxdi)
    relv = step_a * prop
    if aa_rm is not None:
        rm = aa_rm[act].astype(np.float64)
        rawp = np.maximum(rm[:, 0] / scale, rm[:, 1])
        relv = np.maximum(relv, rawp)
    ls_fail = step_a == 0.0
    stop_tol = ~ls_fail & (relv <= tol)
    stop_stag = (~ls_fail & ~stop_tol & (fresh != 0) & (relv < 1e-4)
                 & (relv >= 0.5 * prev_rel))
    stop = stop_tol | stop_stag
    ooi = ~stop & (n_iter + 1 >= max_iter)
    cont = ~stop & ~ooi
    # what the kernel reports: stage-1 verdicts; a failed search is left to the host's stage 2
    flags = np.where(hit, 1, 256 | 512).astype(np.int32)
    flags[hit & stop_tol] |= 16 | 4 | 2
    flags[hit & stop_stag] |= 32 | 2
    flags[hit & ooi] |= 8
    flags[hit & cont] |= 512
    relv = np.where(hit, relv, 0.0)
    prop = np.where(hit, prop, 0.0)
    row = (flags & 512) != 0
    rpos = np.where(row, np.cumsum(row) - 1, -1).astype(np.int32)
    nxt = act[row].astype(np.int32)
    return dict(step64=step_a, step32=step_a.astype(np.float32), relv=relv, prop=prop,
                flags=flags, tix=tix.astype(np.int32), rpos=rpos, nxt=nxt, cnt=int(row.sum()),
                by_flat=by_flat)
