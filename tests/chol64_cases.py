"""Seeded inputs, np.longdouble references, derived bounds and plain float64 numpy transcriptions
for the float64 chain of csrc/chol64.hip and csrc/chol64_drop.hip (CPU only: numpy, scipy).
Shared by tests/test_gpu_chol64_kernels.py (the kernels on the MI355X) and
tests/test_chol64_cases_cpu.py (the checks of the cases themselves).

Bounds.  u = 2^-53, |.| entrywise, every product of a check taken in np.longdouble.

  factor     |Uk^T Uk - A_KK| <= (P + 2) u |Uk|^T |Uk| on the kept set K (the backward bound of a
             Cholesky factorisation, Higham 10.3 with gamma_{P+1}), and for every dependent d the
             kept representation: |Uk[:, <d]^T U[K<d][d] - A[K<d, d]| <= (P + 2) u |Uk|^T |U[K][d]|
             (column d is the forward substitution of A[K<d, d], the same sums).
  solves     x = U^-1 U^-T g on the kept set: |g_K - Uk^T Uk x_K| <= (2 P + 4) u w with
             w = |Uk|^T (|Uk| |x|) (two substitutions, gamma_P each); sglm_chol64_solve rounds x to
             f32 once more: + 2^-24 w.
  residual   |r - ref| <= (P + 3) u (|c| + |G| |x| + |lam x|) (P + 1 FMA terms and a subtraction).
  minnorm    forward error, conditioning of U_KK enters: 16 max(e_ref, P u max|ref|) with e_ref the
  and drop   error of the float64 numpy transcription against the longdouble reference -- the one
             measured quantity; the kernels' reduction orders differ from numpy's under the same
             gamma-type bounds, which the factor 16 allows for.

ratio() divides entrywise: 0/0 counts as 0, x/0 with x > 0 (or NaN) as failure (inf).
"""
from functools import lru_cache

import numpy as np
import scipy.linalg

LD = np.longdouble
U53 = 2.0 ** -53
SENT = -7.25                      # finite float sentinel of the "not written" checks
ISENT = -77                       # int32 sentinel (nulls, counts, status)
BSENT = 0xEE                      # uint8 sentinel (state)
GUARD = 4096                      # bytes of sentinel behind a work buffer
TOL = 1e-9                        # the dependence threshold the engine uses
KEPT, DEP, EXCL, ZERO = 0, 1, 2, 3


def have_longdouble():
    return bool(np.finfo(LD).eps < 2.0 ** -60)


def ld(a):
    return np.asarray(a, dtype=LD)


def err_ratio(err, bound):
    """max err / bound entrywise; 0/0 = 0, x/0 (x > 0 or NaN) = inf."""
    err = np.asarray(err, dtype=np.float64)
    if err.size == 0:
        return 0.0
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where((err > 0) | np.isnan(err), np.inf, 0.0))
    return float(np.max(r))


def ratio(got, ref, bound):
    """max |got - ref| / bound with the difference taken in np.longdouble."""
    return err_ratio(np.abs(ld(got) - ld(ref)), bound)


def sym_upper(T):
    """Symmetric float64 matrix from the upper triangle (i <= j) of T; the rest is not read."""
    T = np.asarray(T, dtype=np.float64)
    return np.triu(T) + np.triu(T, 1).T


def poison_lower(T, k=-1):
    """NaN strictly below the diagonal (in place)."""
    T[np.tril_indices(T.shape[-1], k)] = np.nan
    return T


def assemble(H, S, cmap):
    """The symmetric float64 Gram the header defines: entry (i <= j) is S[cmap[i]][j] when i is
    continuous, else S[cmap[j]][i] when j is, else H[i][j] -- a continuous-continuous entry comes
    from the row of the smaller index."""
    A = np.array(H, dtype=np.float64)
    if S is not None:
        cont = np.flatnonzero(cmap >= 0)
        for j in cont:
            A[:j, j] = S[cmap[j], :j]
        for i in cont:
            A[i, i:] = S[cmap[i], i:]
    return sym_upper(A)


def ld_spd_solve(A, b):
    """solve(A, b) for a symmetric positive definite A, Cholesky in np.longdouble."""
    A, b = ld(A).copy(), ld(b).copy()
    n = A.shape[0]
    R = np.zeros((n, n), LD)
    for j in range(n):
        R[j, j] = np.sqrt(A[j, j])
        R[j, j + 1:] = A[j, j + 1:] / R[j, j]
        A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    for j in range(n):                                   # R^T z = b
        b[j] = (b[j] - R[:j, j] @ b[:j]) / R[j, j]
    for j in range(n - 1, -1, -1):                       # R x = z
        b[j] = (b[j] - R[j, j + 1:] @ b[j + 1:]) / R[j, j]
    return b


def ld_gauss_solve(A, B):
    """solve(A, B) for a small square A by Gaussian elimination with partial pivoting (LD)."""
    A, B = ld(A).copy(), ld(B).copy()
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]], B[[j, p]] = A[[p, j]], B[[p, j]]
        for i in range(j + 1, n):
            m = A[i, j] / A[j, j]
            A[i, j:] -= m * A[j, j:]
            B[i] -= m * B[j]
    for j in range(n - 1, -1, -1):
        B[j] = (B[j] - A[j, j + 1:] @ B[j + 1:]) / A[j, j]
    return B


# ------------------------------------------------------------------------------ factor
FACTOR_CASES = {                       # name: (P, lamp given, one-hot triple)
    "p64": (64, True, False),
    "p192": (192, True, False),
    "p320": (320, True, True),
    "p192_nolamp": (192, False, True),
}
FACTOR_HSRC, FACTOR_DSRC = (1, 0, 1), (2, 0, 1)
ONEHOT = (15, 90, 170)
RIDGE = 2.5


def _structure(P):
    """(copies (d, src), sums (d, (a, b)), zero columns, the interior exclusions of the two
    unpenalised factors) -- every place where the factor's code branches."""
    if P == 64:
        return [(20, 3), (50, 20)], [(40, (7, 11))], [0], (30, 33)
    copies = [(63, 5), (64, 10), (127, 70), (160, 64)]
    zeros = [128]
    if P == 192:
        copies += [(150, 130)]
    else:
        copies += [(255, 190), (256, 200), (300, 130)]
        zeros += [192]
    return copies, [(140, (20, 100))], zeros, (30, 33)


def _design01(rng, P, onehot):
    p, n = P - 7, 3 * P
    X = (rng.random((n, p)) < 0.2).astype(np.float64)
    if onehot:
        pick = rng.integers(0, 3, n)
        for t, col in enumerate(ONEHOT):
            X[:, col] = pick == t
    copies, sums, zeros, _ = _structure(P)
    X[:, zeros] = 0.0
    for d, s in copies:
        X[:, d] = X[:, s]
    for d, (a, b) in sums:
        X[:, d] = X[:, a] + X[:, b]
    Xa = np.zeros((n, P))
    Xa[:, :p] = X
    Xa[:, p] = 1.0
    return Xa


def null_vectors(P, onehot):
    """{d: integer null vector} of the construction, written in the kept columns."""
    copies, sums, _, _ = _structure(P)
    rep = {}

    def r(j):
        return rep.get(j, {j: 1})

    out = {}
    for d, s in copies:
        rep[d] = dict(r(s))
    for d, (a, b) in sums:
        rep[d] = {**r(a)}
        for j, v in r(b).items():
            rep[d][j] = rep[d].get(j, 0) + v
    if onehot:
        rep[P - 7] = {c: 1 for c in ONEHOT}
    for d, comb in rep.items():
        v = np.zeros(P)
        v[d] = 1.0
        for j, m in comb.items():
            v[j] -= m
        out[d] = v
    return dict(sorted(out.items()))


@lru_cache(maxsize=None)
def factor_case(name):
    """Inputs of one sglm_chol64_factor call (nf = 3 on two Grams and three shift rows) and what
    it must return: A [3] (float64, the header's matrix), state / nulls / counts."""
    P, with_lamp, onehot = FACTOR_CASES[name]
    p = P - 7
    rng = np.random.default_rng([31, P, int(onehot)])
    G = np.stack([_design01(rng, P, onehot) for _ in range(2)])
    G = G.transpose(0, 2, 1) @ G
    H = G.astype(np.float32)
    assert np.array_equal(H.astype(np.float64), G)
    for g in range(2):
        poison_lower(H[g])
    excl = _structure(P)[3]
    shift = np.zeros((3, P))
    shift[0, :p] = RIDGE                                  # row 0: ridge, intercept unpenalised
    dshift = shift.astype(np.float32) if not with_lamp else np.full((3, P), 0.5, np.float32)
    dshift[:, p + 1:] = -1.0
    dshift[2, excl[0]] = dshift[1, excl[1]] = -1.0
    lamp = shift.copy() if with_lamp else None
    nulls_of = null_vectors(P, onehot)
    deps = np.array(sorted(nulls_of), dtype=np.int32)
    A, state, nulls, counts = [], [], [], []
    for f in range(3):
        g, r = FACTOR_HSRC[f], FACTOR_DSRC[f]
        Af = G[g] + np.diag(shift[r])
        ex = dshift[r] < 0
        st = np.where(ex, EXCL, np.where(np.diag(Af) > 0, KEPT, ZERO)).astype(np.uint8)
        if r != 0:
            st[deps] = DEP
        A.append(Af)
        state.append(st)
        nd, nz = int(np.sum(st == DEP)), int(np.sum(st == ZERO))
        nulls.append(np.flatnonzero(st == DEP).astype(np.int32))
        counts.append((nd, nd + nz))
    return dict(P=P, p=p, nf=3, H=H, G=G, dshift=dshift, lamp=lamp, A=np.stack(A),
                hsrc=np.array(FACTOR_HSRC, np.int32), dsrc=np.array(FACTOR_DSRC, np.int32),
                state=np.stack(state), nulls=nulls, counts=np.array(counts, np.int32),
                nullvecs=nulls_of, onehot=onehot, tol=TOL)


def factor_f64(A, excl, tol):
    """Plain float64 transcription of the factorisation: right-looking, one pivot at a time.
    -> U (upper), state, piv (Schur complement / original diagonal per initially kept pivot)."""
    A = np.array(A, dtype=np.float64)
    P = A.shape[0]
    d0 = np.diag(A).copy()
    state = np.where(excl, EXCL, np.where(d0 > 0, KEPT, ZERO)).astype(np.uint8)
    off = state != KEPT
    A[off, :] = 0.0
    A[:, off] = 0.0
    U = np.zeros((P, P))
    piv = np.full(P, np.nan)
    for j in range(P):
        if state[j] != KEPT:
            U[j, j] = 1.0
            continue
        piv[j] = A[j, j] / d0[j]
        if not A[j, j] > tol * d0[j]:
            state[j] = DEP
            U[j, j] = 1.0
            continue
        U[j, j] = np.sqrt(A[j, j])
        U[j, j + 1:] = A[j, j + 1:] / U[j, j]
        A[j + 1:, j + 1:] -= np.outer(U[j, j + 1:], U[j, j + 1:])
    return U, state, piv


def factor_ratio(A, state, U):
    """Worst |residual| / bound of the two backward bounds of the factor (module docstring)."""
    P = A.shape[0]
    Uu = np.triu(U)                                       # only i <= j is defined
    K = np.flatnonzero(state == KEPT)
    Uk = ld(Uu[np.ix_(K, K)])
    aUk = np.abs(Uk)
    r = err_ratio(np.abs(Uk.T @ Uk - ld(A[np.ix_(K, K)])), (P + 2) * U53 * (aUk.T @ aUk))
    for d in np.flatnonzero(state == DEP):
        lo = K < d
        col = ld(Uu[K, d])
        err = np.abs(Uk[:, lo].T @ col - ld(A[K[lo], d]))
        r = max(r, err_ratio(err, (P + 2) * U53 * (aUk[:, lo].T @ np.abs(col))))
    return r


def factor_structure(U, state):
    """The exact properties of a factor: [] or the list of those violated."""
    P = U.shape[0]
    bad = []
    off = np.flatnonzero(state != KEPT)
    if not np.all(U[off, off] == 1.0):
        bad.append("diagonal of a non-kept coordinate is not 1.0")
    if any(np.any(U[j, j + 1:] != 0.0) for j in off):
        bad.append("row of a non-kept coordinate is not zero right of the diagonal")
    if any(np.any(U[:j, j] != 0.0) for j in np.flatnonzero(state >= EXCL)):
        bad.append("column of an excluded / zero coordinate is not zero above the diagonal")
    for b in range(0, P, 64):
        if np.any(np.tril(U[b:b + 64, b:b + 64], -1) != 0.0):
            bad.append(f"strict lower part of diagonal tile {b // 64} is not 0.0")
    if np.any(np.isnan(U)):
        bad.append("NaN in U")
    return bad


TOL_EDGE = ("first", "cross")


def tol_edge_case(which):
    """[[4, 2], [2, 2]] at coordinates (a, b): the Schur complement of b is exactly 1.0 on a
    diagonal of 2.0, so b is dependent at tol = 0.5 and kept just below.  "first": a, b = 0, 1 of
    P = 64, everything else excluded.  "cross": a, b = 63, 64 of P = 128, every coordinate kept on
    a diagonal of 4 / 16 -- the decision follows a panel and a trailing update.  Every
    intermediate is a power of two.  U is the same in both outcomes (U_bb = 1 either way)."""
    if which == "first":
        P, a, b = 64, 0, 1
        H = np.zeros((P, P), np.float32)
        dshift = np.full((1, P), -1.0, np.float32)
        dshift[0, [a, b]] = 0.0
        U = np.eye(P)
    else:
        P, a, b = 128, 63, 64
        d = np.where(np.arange(P) % 2 == 0, 4.0, 16.0)
        H = np.diag(d).astype(np.float32)
        dshift = np.zeros((1, P), np.float32)
        U = np.diag(np.sqrt(d))
    H[a, a], H[a, b], H[b, b] = 4.0, 2.0, 2.0
    U[a, a], U[a, b], U[b, b] = 2.0, 1.0, 1.0
    A = sym_upper(H)
    poison_lower(H)
    return dict(P=P, a=a, b=b, H=H[None], dshift=dshift, lamp=np.zeros((1, P)), A=A, U=U,
                excl=dshift[0] < 0, tols=(0.5, float(np.nextafter(0.5, 0.0))))


MIXED_P, MIXED_CPOS = 192, (70, 0, 130)          # c = 0, 1, 2; three blocks; 130 copies 70


def _last_bit_pairs(S, cpos):
    """Make the copy of every continuous-continuous entry that the rule does not select differ
    in its last bit (S: [k][P], in place)."""
    k = len(cpos)
    for c in range(k):
        for e in range(k):
            if cpos[c] < cpos[e]:                        # read: S[c][cpos[e]]
                S[e, cpos[c]] = np.nextafter(S[c, cpos[e]], np.inf)


@lru_cache(maxsize=None)
def mixed_factor_case():
    """sglm_chol64_factor_mixed: P = 192, nf = 2 on hsrc = [1, 0], k = 3 continuous coordinates
    at 70, 0 and 130 (130 an exact copy of 70; a 0/1 copy 64 <- 10).  A[0][0] is raised to 1024 so
    that row 0 of U is A[0][.] / 32 exactly -- which S copy was read then shows bitwise."""
    P, p, k = MIXED_P, MIXED_P - 7, 3
    cpos = np.array(MIXED_CPOS)
    cmap = np.full(P, -1, np.int32)
    cmap[cpos] = np.arange(k)
    rng = np.random.default_rng(32)
    H = np.zeros((2, P, P), np.float32)
    Sg = np.zeros((2, k, P))
    for g in range(2):
        n = 3 * P
        Xa = np.zeros((n, P))
        Xa[:, :p] = rng.random((n, p)) < 0.2
        Xa[:, p] = 1.0
        Xa[:, 64] = Xa[:, 10]
        Xa[:, 0], Xa[:, 70] = rng.normal(0, 1, n), rng.normal(0, 1, n)
        Xa[:, 130] = Xa[:, 70]
        G = Xa.T @ Xa
        S = G[cpos].copy()
        S[1, 0] = 1024.0
        S[2] = S[0]                                       # rows of 130 = rows of 70, then the
        S[0, 130] = S[2, 130] = S[0, 70]                  # entries the rule reads made equal
        S[1, 130] = S[1, 70]
        _last_bit_pairs(S, cpos)
        Sg[g] = S
        G[cpos, :] = np.nan
        G[:, cpos] = np.nan
        H[g] = poison_lower(G).astype(np.float32)
    hsrc, dsrc = np.array([1, 0], np.int32), np.array([1, 0], np.int32)
    S = Sg[hsrc]                                          # S is indexed by the factor
    lamp = np.zeros((2, P))
    lamp[0, :p] = RIDGE
    dshift = np.full((2, P), 0.5, np.float32)
    dshift[:, p + 1:] = -1.0
    A, state = [], []
    for f in range(2):
        Af = assemble(H[hsrc[f]], S[f], cmap) + np.diag(lamp[dsrc[f]])
        st = np.where(dshift[dsrc[f]] < 0, EXCL, KEPT).astype(np.uint8)
        if dsrc[f] == 1:
            st[[64, 130]] = DEP
        A.append(Af)
        state.append(st)
    counts = np.array([[2, 2], [0, 0]], np.int32)
    return dict(P=P, p=p, k=k, nf=2, H=H, S=S, cmap=cmap, cpos=cpos, hsrc=hsrc, dsrc=dsrc,
                lamp=lamp, dshift=dshift, A=np.stack(A), state=np.stack(state), counts=counts,
                nulls=[np.array([64, 130], np.int32), np.zeros(0, np.int32)], tol=TOL)


# ------------------------------------------------------------------------------ host-built factors
def _spd(rng, P):
    M = rng.normal(0, 1, (P, P))
    return M @ M.T / P + np.diag(rng.uniform(0.5, 2.0, P))


def host_factor(rng, P, dep=(), excl=(), zero=()):
    """An upper factor by np.linalg.cholesky with the listed coordinates marked by the factor's
    own conventions (identity rows; excluded / zero columns zero, dependent columns kept above
    the diagonal), NaN everywhere below the diagonal.  -> U, state, counts."""
    A = _spd(rng, P)
    state = np.zeros(P, np.uint8)
    state[list(dep)], state[list(excl)], state[list(zero)] = DEP, EXCL, ZERO
    off = state != KEPT
    A[off, :] = 0.0
    A[:, off] = 0.0
    A[off, off] = 1.0
    U = np.linalg.cholesky(A).T.copy()
    for d in dep:
        rows = np.flatnonzero(state[:d] == KEPT)
        U[rows, d] = rng.normal(0, 0.3, rows.size)
    poison_lower(U)
    nd, nz = len(dep), len(zero)
    return U, state, np.array([nd, nd + nz], np.int32)


def kept_block(U, state):
    """(K, U[K][:, K] with zeros below the diagonal); the P = 8192 factor, all kept and built
    with zeros there, is returned as it is (no 512 MiB copies)."""
    K = np.flatnonzero(state == KEPT)
    if K.size == U.shape[0] > 4096:
        return K, U
    return K, np.triu(U)[np.ix_(K, K)]


# ------------------------------------------------------------------------------ solves
SOLVE_PS = (64, 192, 320)
SOLVE_ROWS = 7
SOLVE_FITS, SOLVE_FSRC, SOLVE_GSRC = (5, 0, 3, 6, 2), (1, 0, 0, 1, 0), (3, 3, 0, 1, 2)


@lru_cache(maxsize=None)
def solve_case(P):
    rng = np.random.default_rng([33, P])
    U0, s0, _ = host_factor(rng, P, dep=(P // 3, P - 1), excl=(5,), zero=(P // 2,))
    U1, s1, _ = host_factor(rng, P, dep=(63,), excl=(0, P - 2))
    g = rng.normal(0, 1, (SOLVE_ROWS, P))
    x0 = rng.normal(0, 1, (SOLVE_ROWS, P))
    return dict(P=P, U=np.stack([U0, U1]), state=np.stack([s0, s1]), g=g, x0=x0,
                fits=np.array(SOLVE_FITS, np.int32), fsrc=np.array(SOLVE_FSRC, np.int32),
                gsrc=np.array(SOLVE_GSRC, np.int32), nq=5)


def solve_f64(U, state, g):
    """x = U^-1 U^-T g on the kept coordinates, 0 elsewhere (scipy triangular solves)."""
    K, Uk = kept_block(U, state)
    x = np.zeros(U.shape[0])
    z = scipy.linalg.solve_triangular(Uk, g[K], trans="T")
    x[K] = scipy.linalg.solve_triangular(Uk, z)
    return x


def solve_ratio(U, state, x, g, f32=False):
    """|g_K - Uk^T Uk x_K| against (2 P + 4) u w (+ 2^-24 w for the f32 output)."""
    P = U.shape[0]
    K, Uk = kept_block(U, state)
    Uk, xk = ld(Uk), ld(x[K])
    aU = np.abs(Uk)
    w = (aU.T @ (aU @ np.abs(xk))).astype(np.float64)
    err = np.abs(ld(g[K]) - Uk.T @ (Uk @ xk))
    return err_ratio(err, ((2 * P + 4) * U53 + (2.0 ** -24 if f32 else 0.0)) * w)


# ------------------------------------------------------------------------------ residual
RESID_CPOS = (130, 20, 70)


def _ld_matvec(G, x, block=256):
    """(G @ x, |G| @ |x|) in np.longdouble, G float64, in row blocks."""
    xl, ax = ld(x), np.abs(ld(x))
    out, oab = np.zeros(G.shape[0], LD), np.zeros(G.shape[0], LD)
    for i in range(0, G.shape[0], block):
        Gl = ld(G[i:i + block])
        out[i:i + block], oab[i:i + block] = Gl @ xl, np.abs(Gl) @ ax
    return out, oab


@lru_cache(maxsize=2)
def resid_case(P, mixed):
    """sglm_chol64_resid: nq fits over two Grams (hsrc = [1, 0]); lamp, dshift, x and r indexed by
    the fit, c by csrc, every row different.  P = 3328: one fit on one Gram (the first size whose
    dynamic LDS, 20 B per coordinate, passes 64 KiB)."""
    rng = np.random.default_rng([34, P, int(mixed)])
    big = P > 1000
    nG, rows, crows = (1, 2, 1) if big else (2, 6, 3)
    if big:
        fits, fsrc, csrc, hsrc = [1], [0], [0], [0]
    else:
        fits, fsrc, csrc, hsrc = [5, 1, 3, 0], [0, 1, 1, 0], [2, 0, 1, 1], [1, 0]
    H = rng.integers(0, 40, (nG, P, P)).astype(np.float32)
    S = cmap = None
    k = 0
    if mixed:
        k = 3
        cmap = np.full(P, -1, np.int32)
        cmap[list(RESID_CPOS)] = np.arange(k)
        S = rng.normal(0, 10, (nG, k, P))
        for g in range(nG):
            _last_bit_pairs(S[g], RESID_CPOS)
            H[g][list(RESID_CPOS), :] = np.nan
            H[g][:, list(RESID_CPOS)] = np.nan
    for g in range(nG):
        poison_lower(H[g])
    x = rng.normal(0, 1, (rows, P))
    c = rng.normal(0, 50, (crows, P))
    lamp = rng.uniform(0, 3, (rows, P))
    dshift = rng.uniform(0, 1, (rows, P)).astype(np.float32)
    dshift[:, P - 6:] = -1.0
    for r in range(rows):
        dshift[r, 10 + r] = -1.0
    ref = np.zeros((len(fits), P), LD)
    bound = np.zeros((len(fits), P))
    for q, fit in enumerate(fits):
        f = fsrc[q]
        G = assemble(H[hsrc[f]], None if S is None else S[f], cmap)
        ex = dshift[fit] < 0
        xs = np.where(ex, 0.0, x[fit])
        gx, agx = _ld_matvec(G, xs)
        lx = ld(lamp[fit]) * ld(xs)
        r = ld(c[csrc[q]]) - (gx + lx)
        b = (P + 3) * U53 * (np.abs(ld(c[csrc[q]])) + agx + np.abs(lx))
        ref[q], bound[q] = np.where(ex, 0.0, r), np.where(ex, 0.0, b.astype(np.float64))
    ii = lambda a: np.array(a, np.int32)
    return dict(P=P, k=k, H=H, S=S, cmap=cmap, x=x, c=c, lamp=lamp, dshift=dshift, rows=rows,
                fits=ii(fits), fsrc=ii(fsrc), csrc=ii(csrc), hsrc=ii(hsrc), nq=len(fits),
                ref=ref, bound=bound)


def resid_f64(c):
    """Plain float64 numpy: c - (G + diag(lam)) x per fit."""
    out = np.zeros((c["nq"], c["P"]))
    for q, fit in enumerate(c["fits"]):
        f = c["fsrc"][q]
        G = assemble(c["H"][c["hsrc"][f]], None if c["S"] is None else c["S"][f], c["cmap"])
        ex = c["dshift"][fit] < 0
        xs = np.where(ex, 0.0, c["x"][fit])
        out[q] = np.where(ex, 0.0, c["c"][c["csrc"][q]] - (G @ xs + c["lamp"][fit] * xs))
    return out


# ------------------------------------------------------------------------------ minnorm
MINNORM_CASES = ("p192", "p320")
MINNORM_ROWS = 4
MINNORM_FITS, MINNORM_FSRC = (2, 0, 3), (0, 1, 2)


def minnorm_f64(U, state, pw, beta):
    """Float64 transcription: null vectors by triangular solves on the kept block, two-pass
    classical Gram-Schmidt on the first pw coordinates, projection."""
    P = U.shape[0]
    Uu = np.triu(U)
    K = np.flatnonzero(state == KEPT)
    Q = []
    for d in np.flatnonzero(state == DEP):
        Kd = K[K < d]
        v = np.zeros(P)
        v[d] = 1.0
        v[Kd] = -scipy.linalg.solve_triangular(Uu[np.ix_(Kd, Kd)], Uu[Kd, d])
        for _ in range(2):
            if Q:
                Qm = np.array(Q)
                v = v - (Qm[:, :pw] @ v[:pw]) @ Qm
        s = v[:pw] @ v[:pw]
        Q.append(v * (1.0 / np.sqrt(s) if s > 0 else 0.0))
    if not Q:
        return beta.copy()
    Qm = np.array(Q)
    return beta - (Qm[:, :pw] @ beta[:pw]) @ Qm


def minnorm_ref(N, pw, beta):
    """beta - N (N_w^T N_w)^-1 N_w^T beta in np.longdouble, N [nd][P] exact integers."""
    if len(N) == 0:
        return ld(beta).copy()
    N, b = ld(N), ld(beta)
    Nw = N[:, :pw]
    return b - ld_gauss_solve(Nw @ Nw.T, Nw @ b[:pw]) @ N


@lru_cache(maxsize=None)
def minnorm_case(name):
    """Three fits (rows 2, 0, 3 of four) on the three factors of factor_case(name); the middle one
    sits on the ridge factor (nd = 0).  ref [3][P] (LD), e_ref and bound per fit."""
    c = factor_case(name)
    P, p = c["P"], c["p"]
    rng = np.random.default_rng([35, P])
    beta = rng.normal(0, 1, (MINNORM_ROWS, P))
    N = np.array(list(c["nullvecs"].values()))
    ref, e_ref, bound, trans = [], [], [], []
    for fit, f in zip(MINNORM_FITS, MINNORM_FSRC):
        st = c["state"][f]
        Nf = N if np.any(st == DEP) else N[:0]
        r = minnorm_ref(Nf, p, beta[fit])
        U, st64, _ = factor_f64(c["A"][f], st == EXCL, c["tol"])
        t = minnorm_f64(U, st64, p, beta[fit])
        e = float(np.max(np.abs(ld(t) - r)))
        floor = P * U53 * float(np.max(np.abs(r)))
        ref.append(r), e_ref.append(e), trans.append(t), bound.append(16 * max(e, floor))
    return dict(P=P, p=p, beta=beta, fits=np.array(MINNORM_FITS, np.int32),
                fsrc=np.array(MINNORM_FSRC, np.int32), ref=ref, e_ref=e_ref, bound=bound,
                trans=trans, floor=[b / 16 for b in bound])


# ------------------------------------------------------------------------------ drop sets
DROP_P = 192
DROP_CASES = ("k64", "k41", "k1")


@lru_cache(maxsize=None)
def drop_factors():
    """Three host-built factors: 0 all kept, 1 with two excluded coordinates (state 2, counts
    zero), 2 with a dependent coordinate (counts non-zero: every pair on it has status 2)."""
    rng = np.random.default_rng(36)
    P = DROP_P
    fs = [host_factor(rng, P), host_factor(rng, P, excl=(7, 150)), host_factor(rng, P, dep=(100,))]
    return (np.stack([f[0] for f in fs]), np.stack([f[1] for f in fs]),
            np.stack([f[2] for f in fs]))


def drop_f64(U, state, sset, c):
    """Float64 transcription of the W / T formula: x = U^-1 (z - W T^-1 W^T z), z = U^-T c, on the
    kept coordinates; 0 on the set.  Set coordinates the factor does not keep are absent."""
    P = U.shape[0]
    K, Uk = kept_block(U, state)
    pos = {int(j): i for i, j in enumerate(K)}
    cols = [pos[s] for s in sset if s in pos]
    z = scipy.linalg.solve_triangular(Uk, c[K], trans="T")
    if cols:
        E = np.zeros((K.size, len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        W = scipy.linalg.solve_triangular(Uk, E, trans="T")
        R = np.linalg.cholesky(W.T @ W).T
        t = scipy.linalg.solve_triangular(R, W.T @ z, trans="T")
        z = z - W @ scipy.linalg.solve_triangular(R, t)
    x = np.zeros(P)
    x[K] = scipy.linalg.solve_triangular(Uk, z)
    x[[s for s in sset]] = 0.0
    return x


@lru_cache(maxsize=None)
def _drop_ref(f, sset):
    """(keep, solve(A[keep, keep], c[keep]) for the three right-hand sides) in np.longdouble, A =
    Uk^T Uk of the factor as given."""
    U, state, _ = drop_factors()
    K, Uk = kept_block(U[f], state[f])
    sel = np.flatnonzero(~np.isin(K, sset))
    keep = K[sel]
    A = ld(Uk).T @ ld(Uk)
    Ak = A[np.ix_(sel, sel)]
    return keep, [ld_spd_solve(Ak, drop_rhs()[r][keep]) for r in range(3)]


@lru_cache(maxsize=None)
def drop_rhs():
    return np.random.default_rng(37).normal(0, 1, (3, DROP_P))


@lru_cache(maxsize=None)
def drop_case(name):
    """One prep + solve_add configuration.  Per query q: expect[q] = None (status 2: the row of x
    stays bitwise) or (keep, ref, bound, e_ref, zero coordinates)."""
    P = DROP_P
    U, state, counts = drop_factors()
    far = P + 1000
    if name == "k64":
        kmax = 64
        sets = [[], list(range(40, 104)), [131, 140, 191], [5, 7, 100], list(range(64))]
        lens = [0, 64, 3, 3, 65]                          # the last one is longer than kmax
        pf, pg = [0, 1, 0, 1, 0, 2, 0], [1, 3, 0, 2, 4, 2, 3]
        psrc = [0, 1, 2, 3, 4, 5, 6, 0, 3]
        fits, rows = [4, 9, 0, 7, 2, 10, 5, 1, 8], 12
        gsrc = [1, 0, 2, 1, 0, 2, 0, 2, 2]
    elif name == "k41":
        kmax = 41
        sets = [[3, 64, 127, 128, 190], list(range(100, 141))]
        lens = [5, 41]
        pf, pg = [1, 0, 0], [0, 0, 1]
        psrc, fits, rows, gsrc = [2, 0, 1], [3, 0, 2], 4, [0, 2, 1]
    else:
        kmax = 1
        sets, lens = [[77]], [1]
        pf, pg = [0, 1], [0, 0]
        psrc, fits, rows, gsrc = [1, 0], [2, 0], 3, [2, 0]
    tab = np.empty((len(sets), kmax), np.int32)
    tab[:, 0::2], tab[:, 1::2] = -1, far                  # the pad: -1 and an index out of range
    for i, s in enumerate(sets):
        tab[i, :min(len(s), kmax)] = s[:kmax]
    status = [2 if (counts[f][1] != 0 or lens[g] > kmax) else 0 for f, g in zip(pf, pg)]
    rng = np.random.default_rng([38, kmax])
    x0 = rng.normal(0, 1, (rows, P))
    fsrc = [pf[pr] for pr in psrc]
    expect = []
    for q, pr in enumerate(psrc):
        if status[pr]:
            expect.append(None)
            continue
        f, sset = pf[pr], tuple(sets[pg[pr]])
        keep, refs = _drop_ref(f, sset)
        expect.append((f, sset, keep, refs))
    ii = lambda a: np.array(a, np.int32)
    return dict(P=P, kmax=kmax, U=U, state=state, counts=counts, sets=tab, lens=ii(lens),
                pf=ii(pf), pg=ii(pg), npair=len(pf), status=ii(status), psrc=ii(psrc),
                fits=ii(fits), fsrc=ii(fsrc), gsrc=ii(gsrc), nq=len(psrc), rows=rows, x0=x0,
                c=drop_rhs(), expect=expect)


def drop_expected(c, q, rhs):
    """(keep, ref (LD), bound, e_ref, floor, set coordinates) of query q solved for c[rhs]."""
    f, sset, keep, refs = c["expect"][q]
    ref = refs[rhs]
    t = drop_f64(c["U"][f], c["state"][f], sset, c["c"][rhs])
    e = float(np.max(np.abs(ld(t[keep]) - ref)))
    floor = c["P"] * U53 * float(np.max(np.abs(ref)))
    return keep, ref, 16 * max(e, floor), e, floor, np.array(sset, dtype=np.int64)


# ------------------------------------------------------------------------------ P = 8192
BIG_P = 8192
BIG_SET = (4100, 8000)


class RankOneUpper:
    """U = diag(D) + strict upper part of a b^T with a, b, D of <= 11 significant bits, so that
    every entry is exact in float64 and products, sums and substitutions with U run in O(P) in
    np.longdouble (running sums).  Dense, diagonally dominant, well conditioned."""

    def __init__(self, P, seed=39):
        rng = np.random.default_rng([seed, P])
        sg = lambda: rng.choice([-1.0, 1.0], P)
        self.P = P
        self.a = sg() * rng.integers(1024, 2048, P) * 2.0 ** -20
        self.b = sg() * rng.integers(1024, 2048, P) * 2.0 ** -20
        self.D = 1.0 + rng.integers(0, 1024, P) / 1024.0

    def dense(self):
        U = np.triu(np.outer(self.a, self.b), 1)
        U[np.diag_indices(self.P)] = self.D
        return U

    def _parts(self, absolute):
        a, b, D = ld(self.a), ld(self.b), ld(self.D)
        return (np.abs(a), np.abs(b), np.abs(D)) if absolute else (a, b, D)

    def mul(self, x, absolute=False):
        """U x (or |U| x)."""
        a, b, D = self._parts(absolute)
        bx = b * ld(x)
        suf = np.cumsum(bx[::-1])[::-1] - bx                # sum over j > i
        return D * ld(x) + a * suf

    def tmul(self, y, absolute=False):
        """U^T y (or |U|^T y)."""
        a, b, D = self._parts(absolute)
        ay = a * ld(y)
        return D * ld(y) + b * (np.cumsum(ay) - ay)         # sum over i < j

    def solve_t(self, g):
        """U^T z = g."""
        a, b, D = self._parts(False)
        g = ld(g)
        z, s = np.zeros(self.P, LD), LD(0)
        for c in range(self.P):
            z[c] = (g[c] - b[c] * s) / D[c]
            s += a[c] * z[c]
        return z

    def solve(self, z):
        """U x = z."""
        a, b, D = self._parts(False)
        z = ld(z)
        x, t = np.zeros(self.P, LD), LD(0)
        for r in range(self.P - 1, -1, -1):
            x[r] = (z[r] - a[r] * t) / D[r]
            t += b[r] * x[r]
        return x

    def ainv(self, c):
        return self.solve(self.solve_t(c))

    def solve_ratio(self, x, g, f32=False):
        aw = self.tmul(self.mul(np.abs(ld(x)), True), True).astype(np.float64)
        err = np.abs(ld(g) - self.tmul(self.mul(x)))
        return err_ratio(err, ((2 * self.P + 4) * U53 + (2.0 ** -24 if f32 else 0.0)) * aw)

    def drop_ref(self, sset, c):
        """solve(A[keep, keep], c[keep]) by the block-inverse identity, in np.longdouble."""
        S = list(sset)
        y = self.ainv(c)
        V = np.stack([self.ainv(np.eye(1, self.P, s)[0]) for s in S], axis=1)
        x = y - V @ ld_gauss_solve(V[S, :], y[S])
        keep = np.setdiff1d(np.arange(self.P), S)
        return keep, x[keep]


def big_case(P=BIG_P, sset=BIG_SET):
    """Inputs of the P = 8192 test (also built small by the CPU checks): the structured factor,
    one right-hand side, one drop set of two coordinates with its reference and bound."""
    R = RankOneUpper(P)
    rng = np.random.default_rng([40, P])
    g = rng.normal(0, 1, P)
    x0 = rng.normal(0, 1, P)
    U = R.dense()
    keep, ref = R.drop_ref(sset, g)
    state = np.zeros(P, np.uint8)
    t = drop_f64(U, state, tuple(sset), g)
    e = float(np.max(np.abs(ld(t[keep]) - ref)))
    floor = P * U53 * float(np.max(np.abs(ref)))
    return dict(P=P, R=R, U=U, g=g, x0=x0, sset=np.array(sset, np.int32), keep=keep, ref=ref,
                e_ref=e, floor=floor, bound=16 * max(e, floor), trans=t)


# ------------------------------------------------------------------------------ through the engine
@lru_cache(maxsize=None)
def engine_case():
    """600 x 20: columns 2, 9, 16 a one-hot triple (their sum is the ones column, so the intercept
    is the dependent pivot), column 12 a copy of column 4."""
    rng = np.random.default_rng(41)
    n, p = 600, 20
    X = (rng.random((n, p)) < 0.3).astype(np.float64)
    pick = rng.integers(0, 3, n)
    for t, col in enumerate((2, 9, 16)):
        X[:, col] = pick == t
    X[:, 12] = X[:, 4]
    y = X @ rng.normal(0, 1, p) + 0.4 + rng.normal(0, 0.5, n)
    return dict(X=X, y=y, onehot=(2, 9, 16), copy=(12, 4))
