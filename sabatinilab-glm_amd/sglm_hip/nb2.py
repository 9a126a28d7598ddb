"""NB2 dispersion by maximum likelihood and the log-likelihood of the count families.

With integer counts y, mu = exp(eta), x = kappa mu and the engine's NB2 loss
l_k = (y + 1/k) log(1 + k e^eta) - y eta:

    log p(y) = -l_k(y, eta) + S(y, k) - lgamma(y + 1),     S(y, k) = sum_{j < y} log1p(k j)
    d/dk log p = S'(y, k) + mu^2 g(x) - y mu / (1 + x),     S' = sum_{j < y} j / (1 + k j)
    g(x) = (log1p(x) - x / (1 + x)) / x^2

(Poisson: -(e^eta - y eta) - lgamma(y + 1); Binomial: -loss.)  The y-only terms are sums over
the tail histogram T[j] = sum_i m_i [y_i > j] of a (mask, response) pair,

    sum m S = sum_j T[j] log1p(k j),  sum m S' = sum_j T[j] j / (1 + k j),
    sum m lgamma(y + 1) = sum_j T[j] ln(j + 1),

so one integer histogram (``count_tails``: sglm_count_hist) serves every kappa and family, and
the eta-dependent half is one row pass for a whole batch of fits (sglm_nb2_kappa_sums).
``kappa_profile`` maximises the likelihood over kappa at fixed predictors for many fits at
once; ``NegativeBinomialRegressor(kappa='ml')`` alternates it with the fixed-kappa fit.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from . import engine as E

KAPPA_LO, KAPPA_HI = 2.0 ** -20, 2.0 ** 10        # the search interval of kappa
THETA_TOL = 2.0 ** -30                            # |step in ln kappa| at which the search stops
YMAX_LIMIT = 1 << 20                              # counts at or above this are refused
MAX_PASSES = 100
START_LO, START_HI = 2.0 ** -6, 2.0 ** 6          # the moment estimate is clipped to this


def _nyi(msg):
    from .estimators import NotYetImplementedError
    return NotYetImplementedError(msg)


def family_name(family: int, power: float) -> str:
    if family == E.FAM_SQUARED:
        return "Normal"
    if family == E.FAM_TWEEDIE_LOG:
        return {1.0: "Poisson", 2.0: "Gamma"}.get(float(power), f"Tweedie(power={power:g})")
    return {E.FAM_BINOMIAL_LOGIT: "Binomial", E.FAM_NB2_LOG: "NB2"}[family]


def check_ll_family(family: int, power: float):
    """The 'll' score exists for Poisson, NB2 and Binomial; every other family is refused."""
    if family in (E.FAM_BINOMIAL_LOGIT, E.FAM_NB2_LOG):
        return
    if family == E.FAM_TWEEDIE_LOG and float(power) == 1.0:
        return
    raise _nyi(f"score_method='ll' on the {family_name(family, power)} family: the "
               "log-likelihood score covers Poisson, NB2 and Binomial")


def needs_counts(family: int) -> bool:
    return family in (E.FAM_TWEEDIE_LOG, E.FAM_NB2_LOG)


# ------------------------------------------------------------------------------ tails
def count_tails(prob: E.Problem, comm=None) -> np.ndarray:
    """Tail histograms of every (mask, response) pair of ``prob`` as int64 [F][R][ymax]:
    T[f][r][j] = sum_i M[f][i] [Y[r][i] > j].  One sglm_count_hist pass with nbins = ymax + 1
    (ymax: the device maximum over the rows some mask holds).  Counts >= 2^20 raise
    NotYetImplementedError; a negative, non-integer or non-finite value on a masked-in row
    raises ValueError.  Under a row-sharded ``comm`` the histograms add over the slabs."""
    import torch
    from . import _lib
    E.require_gpu()
    n = prob.design.n
    Yd = prob.y64_rows()                                   # R x n float64
    M = prob.M
    F, R = M.shape[0], Yd.shape[0]
    used = (M[:, :n] > 0).any(dim=0)
    top = torch.where(used[None, :], Yd, torch.zeros_like(Yd)).max().reshape(1)
    if comm is not None:
        top = top.contiguous()
        comm.max_(top)
    ymax = float(top.item())
    if not math.isfinite(ymax):
        raise ValueError("integer counts are required: a response value is not finite")
    if ymax >= YMAX_LIMIT:
        raise _nyi(f"counts >= 2^20 (max y = {ymax:g}): the tail histogram of the "
                   "log-likelihood is limited to 2^20 bins")
    nbins = max(int(math.floor(ymax)), 0) + 1
    hist = torch.empty((R, F, nbins), dtype=torch.int64, device=Yd.device)
    flags = torch.empty((R, F), dtype=torch.int32, device=Yd.device)
    _lib.call("sglm_count_hist", M.data_ptr(), M.shape[1], F, Yd.data_ptr(), R, n, nbins,
              hist.data_ptr(), flags.data_ptr(), E._stream())
    if comm is not None:
        comm.sum_(hist)
        comm.max_(flags)
    T = hist.flip(-1).cumsum(-1).flip(-1)[:, :, 1:]        # T[j] = sum_{v > j} hist[v]
    if bool(flags.any().item()):
        raise ValueError("integer counts are required: a response value on a fitted or scored "
                         "row is negative or not an integer")
    return np.ascontiguousarray(T.permute(1, 0, 2).cpu().numpy())


def tail_np(y, m=None) -> np.ndarray:
    """Host tail histogram of integer counts (float64 / int array), multiplicities ``m``."""
    y = check_counts(y)
    h = np.bincount(y.astype(np.int64), weights=None if m is None else np.asarray(m, float))
    return np.cumsum(h[::-1])[::-1][1:].astype(np.float64)


def check_counts(y) -> np.ndarray:
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(y) & (y >= 0) & (y == np.floor(y))):
        raise ValueError("integer counts are required: a response value is negative or not "
                         "an integer")
    if y.size and y.max() >= YMAX_LIMIT:
        raise _nyi(f"counts >= 2^20 (max y = {y.max():g})")
    return y


def ll_const(T, family: int, kappa: Optional[float] = None) -> float:
    """The y-only part of the summed log-likelihood of one (mask, response) pair from its tail
    histogram, float64: NB2 sum m (S(y, kappa) - lgamma(y + 1)), Poisson -sum m lgamma(y + 1),
    Binomial 0.  log-likelihood = -(summed loss) + ll_const."""
    if family == E.FAM_BINOMIAL_LOGIT:
        return 0.0
    T = np.asarray(T, dtype=np.float64)
    j = np.arange(T.size, dtype=np.float64)
    if family == E.FAM_NB2_LOG:
        return float(np.sum(T * (np.log1p(float(kappa) * j) - np.log(j + 1.0))))
    if family == E.FAM_TWEEDIE_LOG:
        return -float(np.sum(T * np.log(j + 1.0)))
    raise _nyi(f"log-likelihood of family {family}")


def tail_score(T, kappa: float):
    """(sum m S'(y, kappa), its derivative in kappa) from the tail histogram."""
    T = np.asarray(T, dtype=np.float64)
    j = np.arange(T.size, dtype=np.float64)
    q = j / (1.0 + kappa * j)
    return float(np.sum(T * q)), -float(np.sum(T * q * q))


def moment_kappa(T, cnt: float) -> float:
    """The moment estimate (s^2 - ybar) / ybar^2 of a (mask, response) pair from its tail
    histogram (sum m y = sum T, sum m y (y - 1) = 2 sum j T[j]), clipped to [2^-6, 2^6]."""
    T = np.asarray(T, dtype=np.float64)
    if cnt <= 0 or T.size == 0:
        return START_LO
    s1 = float(T.sum())
    s2 = 2.0 * float(np.sum(T * np.arange(T.size))) + s1          # sum m y^2
    ym = s1 / cnt
    if ym <= 0:
        return START_LO
    k = (s2 / cnt - ym * ym - ym) / (ym * ym)
    return float(min(max(k, START_LO), START_HI)) if math.isfinite(k) else START_LO


# ------------------------------------------------------------------------------ host likelihoods
def loglik_np(family: int, y, eta, kappa: Optional[float] = None) -> float:
    """Summed log-likelihood in host float64 from the linear predictor: Poisson, NB2 (at
    ``kappa``) or Binomial (y in {0, 1})."""
    from .estimators import binomial_loss_np, check_binomial_y, nb2_loss_np
    eta = np.asarray(eta, dtype=np.float64).reshape(-1)
    if family == E.FAM_BINOMIAL_LOGIT:
        return -float(np.sum(binomial_loss_np(check_binomial_y(y), eta)))
    y = check_counts(y)
    if y.shape != eta.shape:
        raise ValueError(f"y has {y.shape[0]} rows, the prediction {eta.shape[0]}")
    T = tail_np(y)
    if family == E.FAM_NB2_LOG:
        return -float(np.sum(nb2_loss_np(kappa, y, eta))) + ll_const(T, family, kappa)
    return -float(np.sum(np.exp(eta) - y * eta)) + ll_const(T, E.FAM_TWEEDIE_LOG)


# ------------------------------------------------------------------------------ the search
def kappa_sums(prob: E.Problem, eta, slots, fit_resp, fit_mask, kappa: np.ndarray, comm=None):
    """out [nfit][K][3] (float64, host) of sglm_nb2_kappa_sums for launch rows ``slots`` of the
    resident ``eta``; ``kappa`` [nfit][K]."""
    import torch
    from . import _lib
    d = prob.design
    dev = d.device
    kappa = np.ascontiguousarray(kappa, dtype=np.float64)
    nfit, K = kappa.shape
    sl = torch.tensor(np.asarray(slots, dtype=np.int32), dtype=torch.int32, device=dev)
    fr = torch.tensor(np.asarray(fit_resp, dtype=np.int32), dtype=torch.int32, device=dev)
    fm = torch.tensor(np.asarray(fit_mask, dtype=np.int32), dtype=torch.int32, device=dev)
    kd = torch.from_numpy(kappa).to(dev)
    out = torch.empty((nfit, K, 3), dtype=torch.float64, device=dev)
    work = torch.empty(max(_lib.query("sglm_nb2_kappa_sums_work_bytes", nfit, K, d.n), 8),
                       dtype=torch.uint8, device=dev)
    _lib.call("sglm_nb2_kappa_sums", d.n, d.ld, nfit, sl.data_ptr(), eta.data_ptr(),
              prob.Y.data_ptr(), prob.M.data_ptr(), fr.data_ptr(), fm.data_ptr(), kd.data_ptr(),
              K, out.data_ptr(), work.data_ptr(), E._stream())
    if comm is not None:
        comm.sum_(out)
    return out.cpu().numpy()


def profile(prob: E.Problem, eta, slots: Sequence[int], fit_resp: Sequence[int],
            fit_mask: Sequence[int], tails: np.ndarray, start=None, comm=None):
    """The maximiser over kappa in [2^-20, 2^10] of the NB2 likelihood at the predictors
    ``eta[slots[f]]`` (device f32 [*][ld]) for every fit f, in one batch.

    A safeguarded Newton search on the score s(theta) = sum m d/dk log p in theta = ln kappa:
    the first pass evaluates both ends of the interval and the start (K = 3), every later pass
    one point per unfinished fit (one sglm_nb2_kappa_sums launch for all of them, plus the host
    tail sums).  A Newton step that leaves the bracket, or a derivative of the wrong sign, is
    replaced by the bracket's midpoint.  Stops at |step| <= 2^-30.  s <= 0 at the lower end (no
    over-dispersion) returns the lower bound with ``at_bound``; s >= 0 at the upper end the
    upper bound.  Returns (kappa [nfit] float64, at_bound [nfit] bool, passes)."""
    nfit = len(slots)
    slots = np.asarray(slots, dtype=np.int32)
    fit_resp = np.asarray(fit_resp, dtype=np.int32)
    fit_mask = np.asarray(fit_mask, dtype=np.int32)
    lo, hi = math.log(KAPPA_LO), math.log(KAPPA_HI)
    Ts = [tails[int(fit_mask[f]), int(fit_resp[f])] for f in range(nfit)]
    if start is None:
        start = [moment_kappa(Ts[f], prob.mask_count(int(fit_mask[f]))) for f in range(nfit)]
    th = np.clip(np.log(np.asarray(start, dtype=np.float64).reshape(nfit)),
                 lo + 1.0, hi - 1.0)
    kappa = np.full(nfit, np.nan)
    at_bound = np.zeros(nfit, dtype=bool)
    a = np.full(nfit, lo)                    # s(a) > 0
    b = np.full(nfit, hi)                    # s(b) < 0
    done = np.zeros(nfit, dtype=bool)

    def score(f, k, sums):
        s1, s2 = tail_score(Ts[f], k)
        return s1 + sums[1], s2 + sums[2]

    def advance(f, t, s, ds):
        """Bracket update at theta t with score s, then the next point (None: finished)."""
        if s == 0.0:
            return None, t
        if s > 0:
            a[f] = t
        else:
            b[f] = t
        dth = math.exp(t) * ds               # d s / d theta
        new = t - s / dth if dth < 0 else math.nan
        if not (a[f] < new < b[f]):
            if b[f] - a[f] <= THETA_TOL:
                return None, 0.5 * (a[f] + b[f])
            return 0.5 * (a[f] + b[f]), None
        if abs(new - t) <= THETA_TOL:
            return None, new
        return new, None

    kk = np.stack([np.full(nfit, KAPPA_LO), np.full(nfit, KAPPA_HI), np.exp(th)], axis=1)
    out = kappa_sums(prob, eta, slots, fit_resp, fit_mask, kk, comm)
    passes = 1
    for f in range(nfit):
        if score(f, KAPPA_LO, out[f, 0])[0] <= 0:
            kappa[f], at_bound[f], done[f] = KAPPA_LO, True, True
        elif score(f, KAPPA_HI, out[f, 1])[0] >= 0:
            kappa[f], at_bound[f], done[f] = KAPPA_HI, True, True
        else:
            s, ds = score(f, kk[f, 2], out[f, 2])
            nxt, fin = advance(f, th[f], s, ds)
            if nxt is None:
                kappa[f], done[f] = math.exp(fin), True
            else:
                th[f] = nxt
    while not done.all() and passes < MAX_PASSES:
        act = np.flatnonzero(~done)
        out = kappa_sums(prob, eta, slots[act], fit_resp[act], fit_mask[act],
                         np.exp(th[act])[:, None], comm)
        passes += 1
        for q, f in enumerate(act):
            s, ds = score(f, math.exp(th[f]), out[q, 0])
            nxt, fin = advance(f, th[f], s, ds)
            if nxt is None:
                kappa[f], done[f] = math.exp(fin), True
            else:
                th[f] = nxt
    kappa[~done] = np.exp(th[~done])
    return kappa, at_bound, passes


def kappa_profile(X, y, coefs, intercepts, rows=None):
    """The ML dispersion at fixed predictors for a batch of fits: fit f has coefficients
    ``coefs[f]`` ([B][p], or [p] for one fit), intercept ``intercepts[f]`` and is taken over
    ``rows[f]`` (row indices, repeats count; None = every row; ``rows=None``: every fit on every
    row).  ``X``: a host design, a lagged frame, or an engine Design.  Returns
    (kappa [B], at_bound [B]): the maximiser over [2^-20, 2^10] of the NB2 likelihood in
    kappa, found to |d ln kappa| <= 2^-30; ``at_bound`` marks a fit whose likelihood still rises
    at an end of the interval (the lower end: no over-dispersion, the Poisson limit)."""
    import torch
    from . import folds
    from .estimators import _as2d
    from .lagframe import LagFrame
    E.require_gpu()
    if isinstance(X, E.Design):
        d = X
    elif isinstance(X, LagFrame):
        d = X.design()
    else:
        d = E.Design.from_host(_as2d(X))
    coefs = np.atleast_2d(np.asarray(coefs, dtype=np.float64))
    B = coefs.shape[0]
    b0 = np.broadcast_to(np.asarray(intercepts, dtype=np.float64).reshape(-1), (B,))
    if coefs.shape[1] != d.p:
        raise ValueError(f"coefs has {coefs.shape[1]} columns, X has {d.p}")
    y = check_counts(y)
    if y.shape[0] != d.n:
        raise ValueError(f"y has {y.shape[0]} rows, X has {d.n}")
    if rows is None:
        masks, fit_mask = [np.ones(d.n, np.uint8)], [0] * B
    else:
        if len(rows) != B:
            raise ValueError(f"rows: one entry per fit ({B}), got {len(rows)}")
        masks = [np.ones(d.n, np.uint8) if r is None else folds.mask_from_idx(r, d.n)
                 for r in rows]
        fit_mask = list(range(B))
    prob = E.Problem(d, [y], masks)
    beta = np.zeros((B, d.P), dtype=np.float32)
    beta[:, : d.p] = coefs
    beta[:, d.p] = b0
    eta = d.eta(torch.from_numpy(beta).to(d.device))
    T = count_tails(prob)
    k, ab, _ = profile(prob, eta, list(range(B)), [0] * B, fit_mask, T)
    return k, ab
