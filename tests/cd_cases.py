"""Inputs and longdouble oracles for the kernels of csrc/cd.hip: the Gram-space elastic-net
coordinate descent (sglm_enet_cd_grouped in its lane, reg and multi forms, sglm_enet_cd_shared),
sglm_center_gram and sglm_gram_ss.  numpy only, plain loops, nothing from sglm_hip.

The descent is called with tol = 0 and max_sweeps = S: every form then does the same fixed work
(S sweeps, or one for a fit whose solution is all zero) and no answer hangs on a convergence
threshold.  `cd_oracle` records every sweep's max|dw| / max|w| so that the CPU test can show that
no fit stops on a rounding accident: a fit either has max|w| = 0 after its first sweep, or moves
by more than 1e-6 of its scale in every sweep -- except at p = 1, where the case is built so that
all of its arithmetic is exact (integer q, dyadic l1, Q + l2 a power of two) and the second sweep's
move is exactly zero in any precision."""
import functools

import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
BAR_W = 1e-9                     # the bar test_gpu_tweedie_enet.py holds the other CD kernels to

P_REG = (1, 7, 511, 512, 513, 1025, 2047, 2048)     # lane (fpw 8) and reg (fpw 4) forms
P_MULTI = (2049, 2262)                              # only the multi form (fpw 4, fpw 2)
P_SHARED = (7, 513, 4071)
# fits_per_wg by p, SGLM_CD_FPW unset / "4": (2 f + 1) * 8 p <= 160 KiB - 1 KiB past p = 2048
FPW_TABLE = {1: (8, 4), 2048: (8, 4), 2049: (4, 4), 2261: (4, 4), 2262: (2, 2), 4070: (2, 2),
             4071: (1, 1)}
L1_FRAC = (1.5, 0.3125, 0.25, 0.125, 0.0625, 0.03125, 0.0)   # of max|q|; 1.5: the all-zero fit


def dead_column(p):
    return p // 2 if p >= 7 else None


@functools.lru_cache(maxsize=None)
def gram(p, seed, rows=300):
    """(Q, X): Q = X^T X of a sparse 0/1 X; for p >= 7 one column's row and column zeroed."""
    rng = np.random.default_rng(1000 * seed + p)
    X = (rng.random((rows, p)) < 0.12).astype(np.float64)
    X[rng.integers(0, rows, p), np.arange(p)] = 1.0         # no column empty by chance
    Q = X.T @ X
    dc = dead_column(p)
    if dc is not None:
        Q[dc, :] = 0.0
        Q[:, dc] = 0.0
    Q.setflags(write=False)
    return Q, X


@functools.lru_cache(maxsize=None)
def cd_case(p, nfit=19, nq=2):
    """Qs [nq][p][p], and per fit: its Q (fit_q), q [nfit][p], l1, l2.  Fit i of Q 0 are the
    first 7 of 19 (2 of 5), so that the workgroup layouts of `layout` come out as the tests say."""
    rng = np.random.default_rng(77 + p)
    Qs, Xs = zip(*(gram(p, s) for s in range(nq)))
    n0 = 7 if nfit == 19 else max(1, (2 * nfit) // 5)
    fit_q = np.array([0] * n0 + [1] * (nfit - n0), dtype=np.int32)
    q = np.zeros((nfit, p))
    l1, l2 = np.zeros(nfit), np.zeros(nfit)
    dc = dead_column(p)
    for i in range(nfit):
        X = Xs[fit_q[i]]
        y = rng.integers(-3, 4, X.shape[0]).astype(np.float64)
        q[i] = X.T @ y                                      # integers
        if dc is not None:
            q[i, dc] = 0.0
        if not np.abs(q[i]).max() > 0:
            q[i, 0] = 3.0
        frac = L1_FRAC[i % len(L1_FRAC)]
        l1[i] = frac * np.abs(q[i]).max()
        if frac < 1 and p >= 7:
            # at least three coordinates start above the threshold: a fit with one active
            # coordinate is at its solution after one sweep, and its second sweep's move is zero
            # or one ulp depending on the precision
            l1[i] = min(l1[i], 0.75 * np.sort(np.abs(q[i]))[-3])
        if p == 1:
            # exact arithmetic: Q + l2 a power of two above Q, so w = (|q| - l1) / 2^k is exact
            q00 = Qs[fit_q[i]][0, 0]
            l2[i] = 2.0 ** (int(np.ceil(np.log2(q00 + 1))) + i % 3) - q00
        else:
            l2[i] = (0.1, 1.0, 10.0, 37.5)[i % 4]
    for a in (q, l1, l2, fit_q):
        a.setflags(write=False)
    return np.stack(Qs), fit_q, q, l1, l2


def cd_oracle(Q, q, l1, l2, max_sweeps, tol):
    """Cyclic coordinate descent in longdouble in the kernels' order, for the fits of ONE Q:
    hv = -q, w = 0; for j in order, skip if Q_jj <= 0, else
        rho = -(hv_j - Q_jj w_j), w_j' = sign(rho) max(|rho| - l1, 0) / (Q_jj + l2),
        hv += Q_j (w_j' - w_j);
    after each sweep a fit stops when max|w| == 0 or max|dw| <= tol max|w|.
    Returns w [nfit][p] (longdouble), sweeps [nfit], ratios: per fit the list of max|dw| / max|w|
    of its sweeps (inf where max|w| == 0)."""
    nfit, p = q.shape
    hv = -q.astype(LD)
    w = np.zeros((nfit, p), dtype=LD)
    l1, l2 = l1.astype(LD), l2.astype(LD)
    act = np.ones(nfit, dtype=bool)
    sweeps = np.full(nfit, max_sweeps, dtype=np.int32)
    ratios = [[] for _ in range(nfit)]
    tol = LD(tol)
    for sweep in range(max_sweeps):
        if not act.any():
            break
        mdw = np.zeros(nfit, dtype=LD)
        mw = np.zeros(nfit, dtype=LD)
        live = np.flatnonzero(act)
        for j in range(p):
            qjj = LD(Q[j, j])
            if not qjj > 0:
                continue
            wj = w[live, j]
            rho = -(hv[live, j] - qjj * wj)
            mag = np.abs(rho) - l1[live]
            nw = np.where(mag > 0, np.copysign(mag, rho) / (qjj + l2[live]), LD(0))
            d = nw - wj
            w[live, j] = nw
            mdw[live] = np.maximum(mdw[live], np.abs(d))
            mw[live] = np.maximum(mw[live], np.abs(nw))
            mv = d != 0
            if mv.any():
                hv[live[mv]] += d[mv, None] * Q[j].astype(LD)[None, :]
        for i in live:
            ratios[i].append(float(mdw[i] / mw[i]) if mw[i] > 0 else np.inf)
            if mw[i] == 0 or mdw[i] <= tol * mw[i]:
                act[i] = False
                sweeps[i] = sweep + 1
    return w, sweeps, ratios


@functools.lru_cache(maxsize=None)
def cd_reference(p, S, nfit=19):
    """(w_ref float64 [nfit][p], sweeps, ratios) of cd_case(p, nfit) with tol = 0, S sweeps."""
    Qs, fit_q, q, l1, l2 = cd_case(p, nfit)
    w = np.zeros((nfit, p))
    sw = np.zeros(nfit, dtype=np.int32)
    ratios = [None] * nfit
    for m in range(Qs.shape[0]):
        sel = np.flatnonzero(fit_q == m)
        wm, sm, rm = cd_oracle(Qs[m], q[sel], l1[sel], l2[sel], S, 0.0)
        w[sel], sw[sel] = wm.astype(np.float64), sm
        for i, r in zip(sel, rm):
            ratios[i] = r
    w.setflags(write=False)
    sw.setflags(write=False)
    return w, sw, ratios


def chunks_sparse(n):
    """two fits per workgroup, the last two workgroups one each (n = 7: 2,2,2,1; 12: 2 x 5,1,1)"""
    if n < 4:
        return [1] * n
    c = [2] * ((n - 2) // 2) + [1, 1] if n % 2 == 0 else [2] * (n // 2) + [1]
    assert sum(c) == n
    return c


def chunks_dense(n, fpw):
    """full workgroups, the last one padded (a full last one gives up a fit to one more)"""
    c = [fpw] * (n // fpw) + ([n % fpw] if n % fpw else [])
    if n % fpw == 0:
        c = c[:-1] + ([fpw - 1, 1] if fpw > 1 else [1])
    assert sum(c) == n
    return c


def layout(fit_q, fit_ids, fpw, sparse):
    """wg_fits [nwg][fpw] (-1 padded), wg_q [nwg]: the fits of each Q in chunks, the workgroups
    then shuffled so that wg_q is not sorted; fit_ids[i] is fit i's row in q / l1 / l2 / w."""
    wgs = []
    for m in np.unique(fit_q):
        ids = [int(fit_ids[i]) for i in np.flatnonzero(fit_q == m)][::-1]   # not ascending
        sizes = chunks_sparse(len(ids)) if sparse else chunks_dense(len(ids), fpw)
        o = 0
        for s in sizes:
            wgs.append((int(m), ids[o:o + s] + [-1] * (fpw - s)))
            o += s
    order = np.random.default_rng(5).permutation(len(wgs))
    if len(wgs) > 1 and all(wgs[a][0] <= wgs[b][0] for a, b in zip(order[:-1], order[1:])):
        order = order[::-1]
    wg_q = np.array([wgs[i][0] for i in order], dtype=np.int32)
    wg_fits = np.array([wgs[i][1] for i in order], dtype=np.int32).reshape(len(wgs), fpw)
    return wg_fits, wg_q


def fit_rows(nfit):
    """fit i's row in the device buffers: an injection into nfit + 2 rows (two stay unnamed)"""
    rows = np.random.default_rng(9).permutation(nfit + 2)
    return rows[:nfit].astype(np.int32), rows[nfit:].astype(np.int32)


def kkt_violation(Q, q, l1, l2, w):
    """largest violation of the elastic-net optimality conditions, relative to max|q|:
    g = Q w - q + l2 w; w_j != 0: g_j + l1 sign w_j = 0; w_j = 0: |g_j| <= l1."""
    Ql, wl = Q.astype(LD), w.astype(LD)
    g = Ql @ wl - q.astype(LD) + LD(l2) * wl
    nz = wl != 0
    v = np.where(nz, np.abs(g + LD(l1) * np.sign(wl)), np.maximum(np.abs(g) - LD(l1), 0))
    return float(v.max() / np.abs(q).max())


# ---- sglm_center_gram ---------------------------------------------------------------------
CG_P = 256
CG_GRAM_OF = np.array([2, 0, 2], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def center_case(p):
    """H f32 [3][256][256]: slot 2 the augmented Gram of a 0/1 design (ones column at index p),
    slot 0 that of an empty mask (all counts 0, G_pp = 0), slot 1 never named; only the entries
    a <= b <= p hold numbers, everything else (the strictly lower triangle included) is NaN."""
    rng = np.random.default_rng(300 + p)
    n = 5000
    X = np.ones((n, p + 1))
    X[:, :p] = rng.random((n, p)) < rng.uniform(0.02, 0.6, p)[None, :]
    G = X.T @ X
    H = np.full((3, CG_P, CG_P), np.nan, dtype=np.float32)
    iu = np.triu_indices(p + 1)
    H[2][iu] = G[iu].astype(np.float32)
    H[0][iu] = 0.0
    assert np.array_equal(H[2][iu].astype(np.float64), G[iu])       # exact counts
    H.setflags(write=False)
    return H


def center_oracle(H, p, gram_of, center):
    """(Q_ref [nmask][p][p] longdouble, bound): Q = G_ab - G_ap G_bp / n (n = G_pp > 0 and
    center), the product exact, one division, one subtraction:
    bound = 4 * 2^-53 (|G_ab| + |G_ap G_bp| / n)."""
    nm = len(gram_of)
    Qr = np.zeros((nm, p, p), dtype=LD)
    bound = np.zeros((nm, p, p))
    for m in range(nm):
        Gm = H[gram_of[m]]
        n = LD(Gm[p, p])
        U = np.triu(Gm[:p, :p].astype(LD))
        gab = U + np.triu(U, 1).T                           # the lower triangle is never read
        g = Gm[:p, p].astype(LD)
        c = np.outer(g, g) / n if (center and n > 0) else np.zeros((p, p), dtype=LD)
        Qr[m] = gab - c
        bound[m] = 4 * U64 * (np.abs(gab) + np.abs(c)).astype(np.float64)
    return Qr, bound


# ---- sglm_gram_ss ---------------------------------------------------------------------------
GS_P = 128
GS_PA = (1, 31, 32, 33, 65)
GS_GROUPS = (1, 256, 257)
GS_SLOT = np.array([2, 0, 1], dtype=np.int32)
GS_NC = 5


@functools.lru_cache(maxsize=None)
def gram_ss_case(pa):
    """H f32 [3][P][P] (upper triangle of three 0/1 designs' augmented Grams over pa
    coordinates, NaN elsewhere), grp_off, fits (a permutation into a beta buffer of nfit + 6
    rows), beta (NaN past pa and in the unnamed rows), c [5][P], cidx, yy.  Fit 0 of the last
    group has small integer beta and c and yy = 2 beta.c - beta^T G beta - 1: its value is
    exactly -1 in any precision."""
    rng = np.random.default_rng(500 + pa)
    P = GS_P
    nfit = sum(GS_GROUPS)
    H = np.full((3, P, P), np.nan, dtype=np.float32)
    Gs = []
    for s in range(3):
        X = np.ones((400, pa))
        X[:, :pa - 1] = rng.random((400, pa - 1)) < 0.2
        G = X.T @ X
        iu = np.triu_indices(pa)
        H[s][iu] = G[iu].astype(np.float32)
        Gs.append(G)
    grp_off = np.concatenate([[0], np.cumsum(GS_GROUPS)]).astype(np.int32)
    fits = rng.permutation(nfit + 6)[:nfit].astype(np.int32)
    beta = np.full((nfit + 6, P), np.nan)
    beta[fits, :pa] = rng.normal(0, 0.3, (nfit, pa))
    c = np.full((GS_NC, P), np.nan)
    c[:, :pa] = rng.normal(0, 20.0, (GS_NC, pa))
    c[3, :pa] = rng.integers(-9, 10, pa)
    cidx = ((np.arange(nfit) * 7 + 3) % GS_NC).astype(np.int32)
    w1 = int(grp_off[2])                                    # the fit whose value is -1
    cidx[w1] = 3
    beta[fits[w1], :pa] = rng.integers(-3, 4, pa)
    yy = np.zeros(nfit)
    for g in range(3):
        G = Gs[GS_SLOT[g]]
        for w in range(grp_off[g], grp_off[g + 1]):
            b = beta[fits[w], :pa]
            v = -2.0 * (b @ c[cidx[w], :pa]) + b @ G @ b
            yy[w] = -v + abs(v) * rng.uniform(0.05, 1.0) + rng.uniform(0.0, 2.0)
    b = beta[fits[w1], :pa]
    yy[w1] = 2.0 * (b @ c[3, :pa]) - b @ Gs[GS_SLOT[2]] @ b - 1.0       # integers: exact
    return H, grp_off, fits, beta, c, cidx, yy, w1


def gram_ss_oracle(H, pa, grp_off, fits, beta, c, cidx, yy):
    """(raw, bound): raw = yy - 2 beta.c + beta^T G beta in longdouble with G symmetrised from
    the upper triangle (the kernel returns max(raw, 0)); bound = (pa + 64) 2^-53 (|yy| +
    2 sum|beta_a c_a| + sum|beta_a||G_ab||beta_b|) -- the constant counts the additions on the
    longest path (32 columns x ceil(pa/32) steps folded into pa, then the row, block, lane and
    final sums)."""
    nfit = len(yy)
    raw = np.zeros(nfit, dtype=LD)
    bound = np.zeros(nfit)
    for g in range(len(grp_off) - 1):
        U = np.triu(np.nan_to_num(H[GS_SLOT[g]][:pa, :pa].astype(np.float64)))
        G = (U + np.triu(U, 1).T).astype(LD)
        for w in range(grp_off[g], grp_off[g + 1]):
            b = beta[fits[w], :pa].astype(LD)
            cw = c[cidx[w], :pa].astype(LD)
            lin = LD(0)
            for a in range(pa):
                lin += b[a] * cw[a]
            quad = b @ (G @ b)
            raw[w] = LD(yy[w]) - 2 * lin + quad
            mag = (abs(yy[w]) + 2 * float(np.abs(b * cw).sum())
                   + float(np.abs(b) @ (np.abs(G) @ np.abs(b))))
            bound[w] = (pa + 64) * U64 * mag
    return raw, bound
