"""Standard errors, covariance matrices and per-group Wald tests of fitted models, batched over
many models on one resident design (csrc/infer.hip).

For a converged fit (w, b) of an ``'irls'`` objective with penalty lam on w (the engine's sum
scaling, ``FitReq.lam``), J = X~^T diag(m v(eta)) X~ is the expected information (X~ the design
with its ones column, v the Fisher weight of the family) and A = J + diag(lam on w, 0 on b):

  cov_type='model'   C = phi A^-1 J A^-1 = phi (A^-1 - lam A^-1 D A^-1)   (default; at lam = 0
                     phi J^-1: statsmodels ``cov_params()``, R ``vcov``)
  cov_type='bayes'   C = phi A^-1
  cov_type='robust'  C = A^-1 M A^-1, M = X~^T diag(m s^2) X~, s = dloss/deta   (HC0)
  cov_type='cluster' C = kappa A^-1 M A^-1, M = sum_c g_c g_c^T, g_c = sum_{i in c} m_i s_i x~_i
                     over the clusters c of ``clusters=`` (one label per row: trial or session
                     ids), kappa = G/(G-1) (n-1)/(n-k) with G clusters, n = sum m and k kept
                     coordinates (statsmodels ``cov_type='cluster'`` / Stata), kappa = 1 with
                     ``cluster_correction=False`` (CR0).  Rows of one cluster need not be
                     contiguous.  M has rank <= G: a group Wald test with more than G - 1
                     degrees of freedom is NaN (status 3, one warning).  csrc/cluster.hip;
                     DESIGN.md §30.

phi = 1 for Poisson, Binomial and NB2 and the Pearson estimate sum m (y - mu)^2 / V(mu) / (n - df)
for Normal, Gamma and Tweedie, df = tr(A^-1 J); ``scale='pearson'`` forces the estimate on any
family (quasi-Poisson), a float fixes phi.  A ``NegativeBinomialRegressor(kappa='ml')`` model is
taken at its fitted ``kappa_`` as if that were known: the errors do not carry the uncertainty of
the dispersion.

``predict_bands`` carries C to the fitted trace: per evaluated row eta = x~^T beta with the
standard error sqrt(x~^T C x~), the mean and its band through the inverse link, and per column
group the share X_g w_g with sqrt(x_g^T C_gg x_g) (csrc/predict.hip).

Not covered (refused where it can be told): two-way clustering, HAC and leverage-corrected
(CR2 / CR3) covariances, mixed or non-binary designs, models fitted with an L1 or group penalty
(naive errors after selection are wrong), likelihood-ratio tests, t and F reference
distributions.
"""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import engine as E
from .estimators import NotYetImplementedError

# the cov_type sglm_cov_groups is called with ('cluster' hands it its own meat as 'robust' does)
COV_TYPES = {"model": 0, "bayes": 1, "robust": 2, "cluster": 2}
ST_RANK = 3     # group status: more degrees of freedom than the clustered meat has rank (G - 1)
MAX_P = 4096
# device bytes the float64 P x P buffers of one chunk of fits may take (factor, inverse and its
# work, Grams, the optional covariance)
INFER_BYTES = float(os.environ.get("SGLM_INFER_BYTES", "8e9"))
# families whose dispersion is 1 unless scale= says otherwise
_UNIT_SCALE = (E.FAM_BINOMIAL_LOGIT, E.FAM_NB2_LOG)


@dataclass
class Inference:
    """Inference of one fitted model (see the module docstring).  ``se`` / ``z`` / ``pvalues``
    are per coefficient (NaN at a coefficient of an all-zero column); the ``group_*`` arrays are
    per group of ``groups`` in the order of ``group_ids`` (None without groups); ``cov`` is the
    (p + 1) x (p + 1) matrix with the intercept last, when asked for; ``n_clusters`` is the
    number of clusters of ``cov_type='cluster'`` (None for the other types)."""
    coef: np.ndarray
    intercept: float
    se: np.ndarray
    intercept_se: float
    z: np.ndarray
    pvalues: np.ndarray
    scale: float
    df: float
    n: float
    group_ids: Optional[np.ndarray] = None
    group_dof: Optional[np.ndarray] = None
    group_stat: Optional[np.ndarray] = None
    group_pvalue: Optional[np.ndarray] = None
    cov: Optional[np.ndarray] = None
    # set per instance by cov_type='cluster'; not a dataclass field (the field list is the
    # constructor's positional order)
    n_clusters = None


@dataclass
class ClusterRuns:
    """Row clusters as the kernels take them: ``G`` clusters, the rows cut into ``R`` maximal
    runs of one cluster (run r = rows roff[r] .. roff[r + 1] - 1) and, unless every cluster is a
    single run (``coff`` None), the CSR of the runs of each cluster in ascending run order."""
    G: int
    R: int
    roff: np.ndarray
    coff: Optional[np.ndarray] = None
    cruns: Optional[np.ndarray] = None


def cluster_runs(clusters, n):
    """``ClusterRuns`` of one label per row (ints, strings, a Series, an index level), through
    ``np.unique(..., return_inverse=True)``; refuses a wrong length, missing labels and fewer
    than two clusters (no device)."""
    import pandas as pd
    ids = clusters.to_numpy() if isinstance(clusters, (pd.Series, pd.Index)) \
        else np.asarray(clusters)
    if ids.ndim == 2 and ids.shape[1] == 1:
        ids = ids[:, 0]
    if ids.ndim != 1 or ids.shape[0] != int(n):
        raise ValueError(f"clusters must hold one label per row: expected length {int(n)}. Got "
                         f"shape {ids.shape} instead.")
    if int(n) >= 2 ** 31:
        raise NotYetImplementedError(f"cov_type='cluster' with n = {int(n)} >= 2^31 rows")
    if bool(np.any(pd.isna(ids))):
        raise ValueError("clusters holds NaN or None labels: every row needs a cluster")
    try:
        u, inv = np.unique(ids, return_inverse=True)
    except TypeError as e:
        raise ValueError(f"clusters holds labels that cannot be ordered ({e})") from None
    inv = np.asarray(inv).reshape(-1)
    G = int(u.shape[0])
    if G < 2:
        raise ValueError(f"cov_type='cluster' needs at least 2 clusters. Got {G} instead.")
    starts = np.flatnonzero(np.r_[True, inv[1:] != inv[:-1]])
    R = int(starts.shape[0])
    roff = np.r_[starts, int(n)].astype(np.int32)
    if R == G:
        return ClusterRuns(G, R, roff)
    rc = inv[starts]
    coff = np.r_[0, np.cumsum(np.bincount(rc, minlength=G))].astype(np.int32)
    return ClusterRuns(G, R, roff, coff, np.argsort(rc, kind="stable").astype(np.int32))


def cluster_kappa(G, n, k):
    """The small-sample factor G/(G-1) (n-1)/(n-k) of statsmodels / Stata."""
    return float(G) / float(G - 1) * (float(n) - 1.0) / (float(n) - float(k))


def check_clusters(cov_type, clusters, n):
    """The ``ClusterRuns`` of ``clusters`` for cov_type='cluster', None for the other types;
    refuses one without the other (no device)."""
    if cov_type == "cluster":
        if clusters is None:
            raise ValueError("cov_type='cluster' needs clusters= (one label per row)")
        return cluster_runs(clusters, n)
    if clusters is not None:
        raise ValueError(f"clusters= is read by cov_type='cluster' only. Got cov_type="
                         f"{cov_type!r} instead.")
    return None


def check_run_bytes(runs, P):
    """Refuse a run-score buffer [R][P] float64 of a single fit beyond SGLM_INFER_BYTES."""
    if runs is not None and 8.0 * runs.R * P > INFER_BYTES:
        raise NotYetImplementedError(
            f"cov_type='cluster' with {runs.R} runs of rows ({runs.G} clusters, {P} columns): "
            f"the run scores of one fit take {8.0 * runs.R * P:.3g} bytes > SGLM_INFER_BYTES = "
            f"{INFER_BYTES:.3g} (sort the rows by cluster, or raise SGLM_INFER_BYTES)")


def check_models(models, cov_type="model", scale=None):
    """The objectives of fitted models that inference covers, refusing the rest (no device)."""
    if cov_type not in COV_TYPES:
        raise ValueError(f"cov_type must be one of {sorted(COV_TYPES)}. Got {cov_type!r} instead.")
    if scale is not None and scale != "pearson":
        if isinstance(scale, str) or not (np.isfinite(float(scale)) and float(scale) > 0):
            raise ValueError(f"scale must be None, 'pearson' or a float > 0. Got {scale!r} instead.")
    objs = []
    for m in models:
        if not hasattr(m, "_objective") and hasattr(m, "model"):
            m = m.model                            # a sglm.GLM wrapper
        if not hasattr(m, "coef_"):
            raise AttributeError(f"This {type(m).__name__} instance is not fitted yet: call fit "
                                 "before inference")
        obj = m._objective()
        if obj.kind != "irls":
            what = {"cd": "an L1 / elastic-net penalty (Lasso, ElasticNet)",
                    "gcd": "a group-lasso penalty (GroupLasso)",
                    "pn": "an L1 / elastic-net penalty on a log link"}.get(obj.kind, obj.kind)
            raise NotYetImplementedError(
                f"inference on a model fitted with {what} (objective kind {obj.kind!r}): naive "
                "standard errors after selection are wrong")
        if m.coef_.shape[0] > MAX_P - 1:
            raise NotYetImplementedError(f"inference with p = {m.coef_.shape[0]} > {MAX_P - 1} "
                                         "columns")
        objs.append((m, obj))
    return objs


def check_design(d):
    """Refuse the designs inference does not cover (mixed, non-binary, row-sharded, p > 4096)."""
    if d.slab is not None:
        raise NotYetImplementedError("inference on a row-sharded problem")
    if d.cont is not None:
        raise NotYetImplementedError("inference on a mixed 0/1 + continuous design")
    if d.xbits is None:
        raise NotYetImplementedError("inference on a non-binary design")
    if d.P > MAX_P:
        raise NotYetImplementedError(f"inference with p = {d.p} > {MAX_P - 1} columns")


def group_lists(groups, p):
    """(ids, goff, gcols, sizes) of one integer id per column (glasso.group_csr's CSR)."""
    from . import glasso
    ids = np.asarray(groups).reshape(-1)
    goff, gcols = glasso.group_csr(ids, p)
    return np.unique(ids), goff, gcols, np.diff(goff)


class _Grams:
    """The caller-owned buffers E._syrk forms Grams from outside a solve: weights W [B][ld] and
    Grams H [B][P][P] by slot, the slots' masks and the problem (no ``wlink``: W is ours)."""

    def __init__(self, prob, fit_mask, B, dev):
        d = prob.design
        self.prob, self.fit_mask, self.up = prob, np.asarray(fit_mask, dtype=np.int32), None
        self.W = None
        self.H = torch.empty((B, d.P, d.P), dtype=torch.float32, device=dev)

    def gram64(self, W, masks, exact, st):
        """triu(X~^T diag(W[k]) X~) of every row k of W (mask masks[k]) in float64 (bf16 MFMA,
        f32 accumulate; W is bf16-exact, so the products are exact)."""
        d = self.prob.design
        self.W, self.fit_mask = W, np.asarray(masks, dtype=np.int32)
        B = W.shape[0]
        E._syrk(d, self, np.arange(B, dtype=np.int32), (d.n + 31) // 32,
                (d.P // 256) * (d.P // 256 + 1) // 2, None, st, exact=exact)
        return torch.triu(self.H[:B]).double()


def _row_pass(prob, fam, power, mode, sel, eta, fit_resp_d, fit_mask_d, want_sums, st):
    """sglm_infer_rows over the fits ``sel`` (slots of eta): planes [3][len(sel)][ld], sums."""
    d = prob.design
    dev = d.device
    nb = len(sel)
    Wp = torch.empty((3, nb, d.ld), dtype=torch.float32, device=dev)
    sums = torch.zeros((nb, 2), dtype=torch.float64, device=dev) if want_sums else None
    work = E._work(E._lib.query("sglm_infer_rows_work_bytes", nb, d.ld), dev, "infer") \
        if want_sums else None
    slots = torch.from_numpy(np.asarray(sel, dtype=np.int32)).to(dev)
    E._lib.call("sglm_infer_rows", int(fam), float(power), int(mode), d.n, d.ld, nb, E._p(slots),
                E._p(eta), E._p(prob.Y), E._p(prob.M), E._p(fit_resp_d), E._p(fit_mask_d),
                E._p(Wp), E._p(sums), E._p(work), st)
    return Wp, sums


def _cluster_meat(prob, runs, s64, st):
    """M[q] = sum_c g_c g_c^T of the fits of s64 [nb][ld] (their signed scores): one pass over
    the design's planes for the run scores, the merge of a cluster's runs, the rank-G update."""
    d = prob.design
    dev = d.device
    nb = s64.shape[0]
    roff_d = torch.from_numpy(runs.roff).to(dev)
    S = torch.empty((nb, runs.R, d.P), dtype=torch.float64, device=dev)
    E._lib.call("sglm_cluster_scores", E._p(d.xbits), d.ld, d.P, d.n, E._p(s64), nb,
                E._p(roff_d), runs.R, E._p(S), st)
    M64 = torch.empty((nb, d.P, d.P), dtype=torch.float64, device=dev)
    coff_d = cruns_d = work = None
    if runs.coff is not None:
        coff_d = torch.from_numpy(runs.coff).to(dev)
        cruns_d = torch.from_numpy(runs.cruns).to(dev)
        work = torch.empty(E._lib.query("sglm_cluster_meat_work_bytes", d.P, nb, runs.G),
                           dtype=torch.uint8, device=dev)
    E._lib.call("sglm_cluster_meat", E._p(S), d.P, nb, runs.R, E._p(coff_d), E._p(cruns_d),
                runs.G, E._p(M64), E._p(work), st)
    return M64


def infer_problem(prob, fams, powers, lams, icpts, coefs, intercepts, resps, masks,
                  goff=None, gcols=None, cov_type="model", scale=None, return_cov=False,
                  runs=None, cluster_correction=True, _on_chunk=None, _extra_bytes=0):
    """Inference of B fits on one problem: per fit its family, power (kappa for NB2), penalty
    ``lam`` (sum scaling), whether it has an intercept, its coefficients, response and mask.
    ``runs``: the ``ClusterRuns`` of cov_type='cluster' (one for every fit).
    Returns a dict of host arrays: var (B, P), state (B, P), scale, df, n (B), stat / dof /
    status (B, ng) with groups, cov (B, P, P) when asked for.
    ``_on_chunk(sel, beta_d, cov, state, kap)`` (internal: predict_bands' row pass) is called once
    per chunk of fits ``sel`` with the chunk's device coefficients [nb][P], covariance
    [nb][P][P] and state [nb][P] and the host factors ``kap`` [nb] the clustered covariance is
    still to be multiplied by (None for the other types); the covariance is then formed on the
    device whether or not ``return_cov`` copies it.  ``_extra_bytes``: device bytes per fit the
    callback allocates, counted into the chunk size."""
    d = prob.design
    check_design(d)
    P, p, ld, dev = d.P, d.p, d.ld, d.device
    B = len(fams)
    ct = COV_TYPES[cov_type]
    clustered = cov_type == "cluster"
    if clustered and runs is None:
        raise ValueError("cov_type='cluster' needs the runs of its clusters")
    check_run_bytes(runs if clustered else None, P)
    st = E._stream()
    ng = 0 if goff is None else len(goff) - 1
    goff_d = gcols_d = None
    if ng:
        goff_d = torch.from_numpy(np.asarray(goff, dtype=np.int32)).to(dev)
        gcols_d = torch.from_numpy(np.asarray(gcols, dtype=np.int32)).to(dev)
    out = {k: [] for k in ("var", "state", "scale", "df", "n", "stat", "dof", "status", "cov")}
    # P x P float64 buffers alive per fit: U, T, Ainv, the Gram sum (+ M, + cov), f32 H twice
    want_cov = bool(return_cov) or _on_chunk is not None
    per = 8 * P * P * (4 + (ct == 2) + want_cov) + 8 * P * P + int(_extra_bytes)
    if clustered:       # the scores, the run scores and the merged cluster scores
        per += 8 * (ld + runs.R * P + (runs.G * P if runs.coff is not None else 0))
    chunk = max(1, int(INFER_BYTES // per))
    for c0 in range(0, B, chunk):
        sel = np.arange(c0, min(B, c0 + chunk))
        nb = len(sel)
        beta = np.zeros((nb, P))
        for i, k in enumerate(sel):
            beta[i, :p] = coefs[k]
            beta[i, p] = intercepts[k] if icpts[k] else 0.0
        beta_d = torch.from_numpy(beta).to(dev)
        eta = d.eta(beta_d.float())
        fr = torch.tensor([int(resps[k]) for k in sel], dtype=torch.int32, device=dev)
        fm_h = np.array([int(masks[k]) for k in sel], dtype=np.int32)
        fm = torch.from_numpy(fm_h).to(dev)
        gr = _Grams(prob, fm_h, nb, dev)
        J32 = torch.zeros((nb, P, P), dtype=torch.float32, device=dev)
        M64 = torch.zeros((nb, P, P), dtype=torch.float64, device=dev) \
            if ct == 2 and not clustered else None
        s64 = torch.empty((nb, ld), dtype=torch.float64, device=dev) if clustered else None
        sums = torch.zeros((nb, 2), dtype=torch.float64, device=dev)
        exact = np.zeros(nb, dtype=bool)
        for fam, power in sorted(set((int(fams[k]), float(powers[k])) for k in sel)):
            loc = np.array([i for i, k in enumerate(sel)
                            if (int(fams[k]), float(powers[k])) == (fam, power)])
            loc_d = torch.from_numpy(loc).to(dev)
            if fam == E.FAM_SQUARED:
                # the exact integer Gram at the mask multiplicities (as engine._gram_ls)
                W = prob.M[fm[loc_d].long()].float()
                J32[loc_d] = gr.gram64(W, fm_h[loc], True, st).float()
                exact[loc] = True
                _, s = _row_pass(prob, fam, power, 0, loc, eta, fr, fm, True, st)
            else:
                Wp, s = _row_pass(prob, fam, power, 0, loc, eta, fr, fm, True, st)
                J = gr.gram64(Wp[0], fm_h[loc], False, st)
                J += gr.gram64(Wp[1], fm_h[loc], False, st)
                J += gr.gram64(Wp[2], fm_h[loc], False, st)
                J32[loc_d] = J.float()          # the f32 triangle sglm_chol64_factor reads
            sums[loc_d] = s
            if clustered:
                sq = torch.empty((len(loc), ld), dtype=torch.float64, device=dev)
                slots = loc_d.int()
                E._lib.call("sglm_infer_scores", int(fam), float(power), d.n, ld, len(loc),
                            E._p(slots), E._p(eta), E._p(prob.Y), E._p(prob.M), E._p(fr),
                            E._p(fm), E._p(sq), st)
                s64[loc_d] = sq
            elif ct == 2:
                Wp, _ = _row_pass(prob, fam, power, 1, loc, eta, fr, fm, False, st)
                Mm = gr.gram64(Wp[0], fm_h[loc], False, st)
                Mm += gr.gram64(Wp[1], fm_h[loc], False, st)
                Mm += gr.gram64(Wp[2], fm_h[loc], False, st)
                M64[loc_d] = Mm + torch.triu(Mm, 1).transpose(1, 2)
        if clustered:
            M64 = _cluster_meat(prob, runs, s64, st)
            del s64
        # A = J + diag(lam on w, 0 on b): float64 factor, then the inverse
        lam = np.array([float(lams[k]) for k in sel])
        fi = np.array([1.0 if icpts[k] else 0.0 for k in sel])
        lam_d = torch.from_numpy(lam).to(dev)
        dshift = torch.full((nb, P), -1.0, dtype=torch.float32, device=dev)
        dshift[:, :p] = lam_d[:, None].float()
        dshift[:, p] = torch.from_numpy(fi - 1.0).to(dev).float()
        lamp = torch.zeros((nb, P), dtype=torch.float64, device=dev)
        lamp[:, :p] = lam_d[:, None]
        U = torch.empty((nb, P, P), dtype=torch.float64, device=dev)
        state = torch.empty((nb, P), dtype=torch.uint8, device=dev)
        nulls = torch.empty((nb, P), dtype=torch.int32, device=dev)
        counts = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
        ident = torch.arange(nb, dtype=torch.int32, device=dev)
        work = E._work(E._lib.query("sglm_chol64_work_bytes", P, nb), dev, "chol64")
        # an exact (integer) Gram takes the exact rank threshold, an f32-accumulated one the f32
        # threshold, as engine._Factor64; a chunk mixing both takes the f32 one
        small = max(prob.mask_count(int(v)) for v in fm_h) < 2 ** 24
        tol = E.RANK_TOL_EXACT if exact.all() and small else E.RANK_TOL_F32
        E._lib.call("sglm_chol64_factor", E._p(J32), P, E._p(ident), E._p(dshift), E._p(lamp),
                    E._p(ident), nb, tol, E._p(U), E._p(state), E._p(nulls), E._p(counts),
                    E._p(work), st)
        cnt = counts.cpu().numpy()
        if cnt[:, 0].any():
            bad = int(np.argmax(cnt[:, 0] > 0))
            raise ValueError(f"the model is not identified: {int(cnt[bad, 0])} coordinate(s) of "
                             f"fit {int(sel[bad])} are linearly dependent on the others (add a "
                             "penalty or drop the columns)")
        Ainv = torch.empty((nb, P, P), dtype=torch.float64, device=dev)
        T = torch.empty(E._lib.query("sglm_chol64_inverse_work_bytes", P, nb), dtype=torch.uint8,
                        device=dev)
        E._lib.call("sglm_chol64_inverse", E._p(U), P, E._p(state), nb, E._p(Ainv), E._p(T), st)
        del U, T
        # df = tr(A^-1 J) = kept coordinates - lam sum_{j < p} (A^-1)_jj; the Pearson scale
        kept = (state == 0).sum(dim=1).double()
        df = kept - lam_d * torch.diagonal(Ainv, dim1=1, dim2=2)[:, :p].sum(dim=1)
        nrow = sums[:, 1]
        pearson = sums[:, 0] / (nrow - df)
        if scale == "pearson":
            phi = pearson
        elif scale is not None:
            phi = torch.full_like(pearson, float(scale))
        else:
            unit = np.array([int(fams[k]) in _UNIT_SCALE
                             or (int(fams[k]) == E.FAM_TWEEDIE_LOG and float(powers[k]) == 1.0)
                             for k in sel])
            phi = torch.where(torch.from_numpy(unit).to(dev), torch.ones_like(pearson), pearson)
        phi = phi.contiguous()
        var = torch.zeros((nb, P), dtype=torch.float64, device=dev)
        stat = torch.zeros((nb, max(ng, 1)), dtype=torch.float64, device=dev)
        dof = torch.zeros((nb, max(ng, 1)), dtype=torch.int32, device=dev)
        status = torch.zeros((nb, max(ng, 1)), dtype=torch.int32, device=dev)
        cov = torch.zeros((nb, P, P), dtype=torch.float64, device=dev) if want_cov else None
        E._lib.call("sglm_cov_groups", E._p(Ainv), P, p, None, E._p(state), E._p(M64), ct, nb,
                    E._p(lam_d), E._p(phi), E._p(beta_d), E._p(goff_d), E._p(gcols_d), ng,
                    E._p(var), E._p(stat), E._p(dof), E._p(status), E._p(cov), st)
        for key, t in (("var", var), ("state", state), ("scale", phi), ("df", df), ("n", nrow),
                       ("stat", stat), ("dof", dof), ("status", status)):
            out[key].append(t.cpu().numpy())
        if return_cov:
            out["cov"].append(cov.cpu().numpy())
        kap = None
        if clustered:
            # kappa on the results (sglm_cov_groups is as it was); the meat's rank is <= G
            # (G - 1 where the g_c sum to zero), so a larger block has no Wald statistic
            kap = np.array([cluster_kappa(runs.G, nn, kk) if cluster_correction else 1.0
                            for nn, kk in zip(out["n"][-1], kept.cpu().numpy())])
            out["var"][-1] = out["var"][-1] * kap[:, None]
            if return_cov:
                out["cov"][-1] = out["cov"][-1] * kap[:, None, None]
            over = (out["dof"][-1] > runs.G - 1) & (out["status"][-1] != 2)
            out["stat"][-1] = np.where(over, np.nan, out["stat"][-1] / kap[:, None])
            out["status"][-1] = np.where(over, ST_RANK, out["status"][-1]).astype(np.int32)
        if _on_chunk is not None:
            _on_chunk(sel, beta_d, cov, state, kap)
    res = {k: np.concatenate(v) for k, v in out.items() if v}
    if not ng:
        for k in ("stat", "dof", "status"):
            res.pop(k)
    return res


def _resolve_models(y, models, groups, cov_type, scale, clusters):
    """The host-side checks infer and predict_bands share (no device): (single, (model,
    objective) pairs, responses, response slot per model, ClusterRuns or None, p, and the group
    ids / goff / gcols / sizes of ``groups`` or four Nones)."""
    single = not isinstance(models, (list, tuple))
    models = [models] if single else list(models)
    pairs = check_models(models, cov_type, scale)
    B = len(pairs)
    if isinstance(y, (list, tuple)) and len(y) == B and np.ndim(y[0]) >= 1:
        ys = [np.asarray(v, dtype=np.float64).reshape(-1) for v in y]
    else:
        ys = [np.asarray(y, dtype=np.float64).reshape(-1)]
    resps = list(range(B)) if len(ys) == B and B > 1 else [0] * B
    runs = check_clusters(cov_type, clusters, ys[0].shape[0])
    p = pairs[0][0].coef_.shape[0]
    check_run_bytes(runs, E.pad_to(p + 1, E.COL_PAD))
    for m, _ in pairs:
        if m.coef_.shape[0] != p:
            raise ValueError("the models have different numbers of coefficients")
    ids = goff = gcols = sizes = None
    if groups is not None:
        ids, goff, gcols, sizes = group_lists(groups, p)
    return single, pairs, ys, resps, runs, p, ids, goff, gcols, sizes


def _resolve_design(pairs, X, p):
    """The resident design of ``X`` through the models' ``_design``, refused as ``check_design``
    refuses it."""
    d = pairs[0][0]._design(X)
    if d.p != p:
        raise ValueError(f"X has {d.p} features, but the models are expecting {p} features")
    check_design(d)
    return d


def infer(X, y, models, groups=None, cov_type="model", scale=None, return_cov=False,
          clusters=None, cluster_correction=True):
    """Inference of one fitted estimator or a list of them (e.g. one per alpha or per
    response) on the design ``X`` they were fitted on: a list of ``Inference`` (one, not a list,
    for a single model).  ``y``: one response vector, or one per model.  ``groups``: one integer
    id per column (``sglm_ez.event_groups``) for per-group Wald tests.  ``clusters``: one label
    per row (trial or session ids; any labels ``np.unique`` orders) for ``cov_type='cluster'``,
    shared by every model; ``cluster_correction=False`` drops the small-sample factor (CR0)."""
    import scipy.special
    single, pairs, ys, resps, runs, p, ids, goff, gcols, sizes = _resolve_models(
        y, models, groups, cov_type, scale, clusters)
    B = len(pairs)
    d = _resolve_design(pairs, X, p)
    if groups is not None:
        kmax = E._lib.query("sglm_cov_groups_kmax")
        if np.any(sizes > kmax):
            warnings.warn(f"{int(np.sum(sizes > kmax))} group(s) have more than {kmax} columns: "
                          "their Wald statistics are NaN", UserWarning, stacklevel=2)
    prob = E.Problem(d, ys, [np.ones(d.n, np.uint8)])
    r = infer_problem(prob, [o.family for _, o in pairs], [o.power for _, o in pairs],
                      [o.lam(float(d.n)) for _, o in pairs],
                      [o.fit_intercept for _, o in pairs], [m.coef_ for m, _ in pairs],
                      [m.intercept_ for m, _ in pairs], resps, [0] * B, goff, gcols, cov_type,
                      scale, return_cov, runs, cluster_correction)
    if runs is not None and groups is not None and np.any(r["status"] == ST_RANK):
        warnings.warn(f"{int(np.sum(r['status'] == ST_RANK))} group test(s) have more degrees of "
                      f"freedom than the {runs.G} clusters leave (G - 1 = {runs.G - 1}): their "
                      "Wald statistics are NaN", UserWarning, stacklevel=2)
    res = []
    for k, (m, o) in enumerate(pairs):
        var = r["var"][k].copy()
        var[r["state"][k] != 0] = np.nan
        with np.errstate(invalid="ignore", divide="ignore"):
            se_all = np.sqrt(var)
            coef = np.asarray(m.coef_, dtype=np.float64)
            z = coef / se_all[:p]
            pv = scipy.special.erfc(np.abs(z) / np.sqrt(2.0))
        inf = Inference(coef=coef.copy(), intercept=float(m.intercept_), se=se_all[:p],
                        intercept_se=float(se_all[p]) if o.fit_intercept else float("nan"),
                        z=z, pvalues=pv, scale=float(r["scale"][k]), df=float(r["df"][k]),
                        n=float(r["n"][k]))
        if runs is not None:
            inf.n_clusters = runs.G
        if groups is not None:
            stat, dof = r["stat"][k], r["dof"][k].astype(np.int64)
            with np.errstate(invalid="ignore", divide="ignore"):
                gp = np.where(dof > 0, scipy.special.gammaincc(np.maximum(dof, 1) / 2.0,
                                                               stat / 2.0), np.nan)
            inf.group_ids, inf.group_dof, inf.group_stat, inf.group_pvalue = ids, dof, stat, gp
        if return_cov:
            keep = np.r_[np.arange(p), p]
            inf.cov = r["cov"][k][np.ix_(keep, keep)]
        res.append(inf)
    return res[0] if single else res



# ------------------------------------------------------------------------------ fitted traces
@dataclass
class PredictionBands:
    """Pointwise bands of one fitted model's trace over the evaluated rows (``predict_bands``;
    statsmodels ``get_prediction().summary_frame()``).  ``eta`` / ``eta_se``: the linear
    predictor and its standard error sqrt(x~^T C x~); ``mean`` the inverse link of eta,
    ``mean_se`` the delta-method |dmu/deta| eta_se, ``lo`` / ``hi`` the inverse link of
    eta -+ z_level eta_se.  With groups, ``group_eta`` / ``group_se`` / ``group_lo`` /
    ``group_hi`` (ng x rows, link scale, no intercept) are each group's share X_g w_g of eta in
    the order of ``group_ids`` (NaN for a group of more than 64 columns)."""
    eta: np.ndarray
    eta_se: np.ndarray
    mean: np.ndarray
    mean_se: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    level: float
    group_ids: Optional[np.ndarray] = None
    group_eta: Optional[np.ndarray] = None
    group_se: Optional[np.ndarray] = None
    group_lo: Optional[np.ndarray] = None
    group_hi: Optional[np.ndarray] = None


def normalize_rows(rows, n):
    """``rows`` of ``predict_bands`` as an int32 index array into the n evaluated rows (None:
    every row): a slice, or integers in [0, n) in any order, repeats allowed (no device)."""
    if rows is None:
        return None
    if isinstance(rows, slice):
        return np.ascontiguousarray(np.arange(int(n), dtype=np.int32)[rows])
    idx = np.asarray(rows)
    if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
        raise ValueError(f"rows must be a slice or a 1-D array of integer row indices. Got "
                         f"shape {idx.shape}, dtype {idx.dtype} instead.")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= int(n)):
        raise ValueError(f"rows must lie in [0, {int(n)}). Got a range of [{int(idx.min())}, "
                         f"{int(idx.max())}] instead.")
    return np.ascontiguousarray(idx, dtype=np.int32)


def level_quantile(level):
    """z of a two-sided normal band at ``level``; refuses a level outside (0, 1)."""
    import scipy.special
    if isinstance(level, (str, bytes)) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie in (0, 1). Got {level!r} instead.")
    return float(np.sqrt(2.0) * scipy.special.erfinv(float(level)))


def link_bands(family, eta, se, zq):
    """(mean, mean_se, lo, hi) of a predictor and its standard error: the inverse link of eta
    and of eta -+ zq se (so the band stays inside the mean's range), mean_se = |dmu/deta| se;
    host float64, the logistic function from exp(-|eta|) (no overflow)."""
    from .estimators import sigmoid_np
    eta, se = np.asarray(eta, dtype=np.float64), np.asarray(se, dtype=np.float64)
    a, b = eta - zq * se, eta + zq * se
    if family == E.FAM_BINOMIAL_LOGIT:
        e = np.exp(-np.abs(eta))
        return sigmoid_np(eta), e / (1.0 + e) ** 2 * se, sigmoid_np(a), sigmoid_np(b)
    if family in (E.FAM_TWEEDIE_LOG, E.FAM_NB2_LOG):
        mu = np.exp(eta)
        return mu, mu * se, np.exp(a), np.exp(b)
    return eta.copy(), se.copy(), a, b


def check_new_design(X_new, p):
    """The host-side refusals of ``X_new`` (no device): another column count, entries that are
    not 0/1 (a device-resident lagged frame is 0/1 by construction).  Returns its row count."""
    from .estimators import _as2d
    from .lagframe import LagFrame
    Xn = _as2d(X_new)
    if Xn.shape[1] != p:
        raise ValueError(f"X_new has {Xn.shape[1]} features, but the models are expecting {p} "
                         "features")
    if not isinstance(Xn, LagFrame) and not bool(np.all((Xn == 0) | (Xn == 1))):
        raise ValueError("X_new must be a 0/1 design with the columns of X: it holds entries "
                         "that are neither 0 nor 1")
    return int(Xn.shape[0])


def check_band_bytes(nr, ng):
    """Refuse an output of a single fit (eta and variance of the trace and of ng groups over nr
    rows, float64) beyond SGLM_INFER_BYTES; returns its bytes."""
    nbytes = 16.0 * nr * (1 + ng)
    if nbytes > INFER_BYTES:
        raise NotYetImplementedError(
            f"predict_bands over {nr} rows and {ng} groups: the output of one fit takes "
            f"{nbytes:.3g} bytes > SGLM_INFER_BYTES = {INFER_BYTES:.3g} (pass rows=, or raise "
            "SGLM_INFER_BYTES)")
    return int(nbytes)


def predict_bands(X, y, models, X_new=None, rows=None, groups=None, level=0.95,
                  cov_type="model", scale=None, clusters=None, cluster_correction=True):
    """Pointwise confidence bands of the fitted trace of one fitted estimator or a list of them
    (as ``infer``: one per alpha or per response on one resident design): a ``PredictionBands``
    each.  The covariance C is ``infer``'s, from ``(X, y)`` the models were fitted on; the trace
    is evaluated on ``X_new`` (a 0/1 design with the same columns, e.g. holdout rows; default
    ``X``), on its rows ``rows`` (a slice or an index array, any order, repeats allowed; default
    all).  ``groups``: one integer id per column (``sglm_ez.event_groups``) for each group's
    share of the predictor with its own band.  C and the coefficients stay on the device
    (csrc/predict.hip); the fits are chunked against SGLM_INFER_BYTES with their
    outputs counted in, and an output of one fit beyond it is refused (pass ``rows``).
    Pointwise, normal-theory bands of the mean: not simultaneous, not prediction intervals."""
    zq = level_quantile(level)
    single, pairs, ys, resps, runs, p, ids, goff, gcols, sizes = _resolve_models(
        y, models, groups, cov_type, scale, clusters)
    B = len(pairs)
    n_eval = ys[0].shape[0] if X_new is None else check_new_design(X_new, p)
    idx = normalize_rows(rows, n_eval)
    nr = n_eval if idx is None else int(idx.shape[0])
    ng = 0 if groups is None else len(goff) - 1
    out_bytes = check_band_bytes(nr, ng)
    d = _resolve_design(pairs, X, p)
    dn = d
    if X_new is not None:
        dn = pairs[0][0]._design(X_new)
        if dn.xbits is None or dn.cont is not None:
            raise ValueError("X_new must be a 0/1 design with the columns of X")
        check_design(dn)
    if dn.n != n_eval:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: "
                         f"[{dn.n}, {n_eval}]")
    if dn.rbits is None:
        raise NotYetImplementedError("predict_bands on a design without row-major bit planes")
    if groups is not None:
        kmax = E._lib.query("sglm_cov_groups_kmax")
        if np.any(sizes > kmax):
            warnings.warn(f"{int(np.sum(sizes > kmax))} group(s) have more than {kmax} columns: "
                          "their traces are NaN", UserWarning, stacklevel=2)
    dev = dn.device
    eta = np.zeros((B, nr))
    var = np.zeros((B, nr))
    geta = np.zeros((B, ng, nr)) if ng else None
    gvar = np.zeros((B, ng, nr)) if ng else None
    goff_d = gcols_d = None
    if ng:
        goff_d = torch.from_numpy(np.asarray(goff, dtype=np.int32)).to(dev)
        gcols_d = torch.from_numpy(np.asarray(gcols, dtype=np.int32)).to(dev)
    idx_d = None if idx is None else torch.from_numpy(idx).to(dev)

    def row_pass(sel, beta_d, cov, state, kap):
        # one launch over all nr rows: the chunk of fits already counts its outputs
        # (_extra_bytes), and one fit's output fits SGLM_INFER_BYTES (check_band_bytes)
        nb = len(sel)
        st = E._stream()
        ic = torch.tensor([1 if pairs[k][1].fit_intercept else 0 for k in sel],
                          dtype=torch.int32, device=dev)
        e_d = torch.empty((nb, nr), dtype=torch.float64, device=dev)
        v_d = torch.empty((nb, nr), dtype=torch.float64, device=dev)
        E._lib.call("sglm_predict_rows", E._p(dn.rbits), dn.ld, dn.P, dn.p, dn.n, E._p(idx_d),
                    nr, E._p(beta_d), E._p(cov), E._p(state), E._p(ic), nb, E._p(e_d),
                    E._p(v_d), st)
        eta[sel] = e_d.cpu().numpy()
        v = v_d.cpu().numpy()
        var[sel] = v if kap is None else v * kap[:, None]
        if ng:
            ge_d = torch.empty((nb, ng, nr), dtype=torch.float64, device=dev)
            gv_d = torch.empty((nb, ng, nr), dtype=torch.float64, device=dev)
            E._lib.call("sglm_predict_groups", E._p(dn.rbits), dn.ld, dn.P, dn.p, dn.n,
                        E._p(idx_d), nr, E._p(beta_d), E._p(cov), E._p(state), nb,
                        E._p(goff_d), E._p(gcols_d), ng, E._p(ge_d), E._p(gv_d), st)
            geta[sel] = ge_d.cpu().numpy()
            gv = gv_d.cpu().numpy()
            gvar[sel] = gv if kap is None else gv * kap[:, None, None]

    if nr:
        prob = E.Problem(d, ys, [np.ones(d.n, np.uint8)])
        infer_problem(prob, [o.family for _, o in pairs], [o.power for _, o in pairs],
                      [o.lam(float(d.n)) for _, o in pairs],
                      [o.fit_intercept for _, o in pairs], [m.coef_ for m, _ in pairs],
                      [m.intercept_ for m, _ in pairs], resps, [0] * B, None, None, cov_type,
                      scale, False, runs, cluster_correction, _on_chunk=row_pass,
                      _extra_bytes=out_bytes)
    res = []
    for k, (_, o) in enumerate(pairs):
        with np.errstate(invalid="ignore"):
            se = np.sqrt(var[k])
            mean, mean_se, lo, hi = link_bands(o.family, eta[k], se, zq)
            pb = PredictionBands(eta=eta[k], eta_se=se, mean=mean, mean_se=mean_se, lo=lo, hi=hi,
                                 level=float(level))
            if groups is not None:
                gse = np.sqrt(gvar[k])
                pb.group_ids, pb.group_eta, pb.group_se = ids, geta[k], gse
                pb.group_lo, pb.group_hi = geta[k] - zq * gse, geta[k] + zq * gse
        res.append(pb)
    return res[0] if single else res
