"""Elastic-net penalised Poisson / Gamma / Tweedie (log link) fits: batched proximal Newton.

Objective of one fit on n rows (sum of its mask's multiplicities), in the engine's sum scaling:

    sum_i m_i loss_power(y_i, eta_i) + l1 |w|_1 + l2/2 |w|^2,   eta = X w + b,
    l1 = alpha rho n,  l2 = alpha (1 - rho) n,  b unpenalised

(pyglmnet's Poisson objective, which the reference's requirements pin; sklearn's
TweedieRegressor objective at rho = 0).  Every outer iteration joins pieces the IRLS engine
already has -- the link, the exact float64-summed gradient, the bf16-weight MFMA Gram (dense
bit-plane or event-structured), the trial-loss row pass -- with the kernels of csrc/pn.hip:
the float64 quadratic model with the intercept eliminated (sglm_pn_model), a warm-started
coordinate descent with an active set on one weighted Hessian per fit (sglm_enet_cd_warm), and
the direction, Armijo decrease, trial penalties and KKT violation (sglm_pn_step).

The Hessian carries bf16 weights in an f32 triangle.  That is safe: it only shapes the model,
whose minimiser is u = w exactly when the exact gradient meets the KKT conditions at w, so the
fixed point depends on the gradient alone.

Device state is held per slot as in engine.irls; stopped fits cost nothing.  One host round
trip per outer iteration (a second one only for fits whose first four trial steps all fail).
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import engine as E
from .cd import CD_TOL

CD_MAX_SWEEPS = 10000
# bytes of float64 Q (p x p per fit) held at once: the fits of an iteration are modelled and
# solved in chunks of at most this (at p = 2000 one Q is 32 MB)
Q_BUDGET = float(os.environ.get("SGLM_PN_Q_BYTES", str(2 << 30)))
MAX_P = 4096


def _unsupported(msg):
    from .estimators import NotYetImplementedError
    return NotYetImplementedError(msg)


def prox_newton(prob: E.Problem, reqs: List[E.FitReq], stats: Optional[E.IrlsStats] = None,
                comm=None):
    """Solve the requests (one log-link family and power; ``lam`` = l2, ``l1`` = l1, both in
    the sum scaling); returns (results, final eta tensor [B][ld]) like engine.irls."""
    E.require_gpu()
    if not reqs:
        return [], None
    if comm is not None:
        raise _unsupported("row-sharded solve of elastic-net log-link objectives")
    d = prob.design
    fam, power = reqs[0].family, float(reqs[0].power)
    if fam != E.FAM_TWEEDIE_LOG or any(r.family != fam or float(r.power) != power for r in reqs):
        raise ValueError("prox_newton(): one log-link family and power per batch")
    if any(r.drop >= 0 for r in reqs):
        raise _unsupported("drop sets on the log-link IRLS path (Poisson / Gamma / Tweedie "
                           "objectives)")
    if d.slab is not None:
        raise _unsupported("row-sharded solve of elastic-net log-link objectives")
    if d.xbits is None or d.rbits is None or d.cont is not None or d.xf is not None:
        raise _unsupported("elastic-net log-link fits need a 0/1 design (a mixed or "
                           "non-binary design is not supported)")
    B0, P, ld, n, p = len(reqs), d.P, d.ld, d.n, d.p
    if p > MAX_P:
        raise _unsupported(f"elastic-net log-link fits hold p <= {MAX_P} predictors")
    dev = d.device
    bf = E._scratch().buf.get(B0, P, ld, dev)
    st = E._stream()
    _p = E._p
    tol = E.STOP_TOL

    up = E._Uploads(dev)
    l1 = np.array([float(r.l1) for r in reqs])
    l2 = np.array([float(r.lam) for r in reqs])
    fi = np.array([1 if r.fit_intercept else 0 for r in reqs], dtype=np.uint8)
    icpt = np.zeros(B0)
    beta = np.zeros((B0, P), dtype=np.float64)
    warm = any(r.coef0 is not None for r in reqs)
    for k, r in enumerate(reqs):
        if r.coef0 is not None:
            beta[k, :p] = r.coef0
            icpt[k] = (r.intercept0 or 0.0) if r.fit_intercept else 0.0
        elif r.fit_intercept:
            ym = prob.mask_stats(r.resp, r.mask)[2]
            if ym <= 0:
                raise ValueError("Some value(s) of y are out of the valid range of the loss")
            icpt[k] = math.log(ym)
    beta[:, p] = icpt
    beta64_d = torch.from_numpy(beta).to(dev)
    bf.beta[:B0].copy_(beta64_d)
    if warm:
        d.eta(bf.beta, bf.eta)
    else:
        bf.eta[:, :n].copy_(bf.beta[:, p:p + 1].expand(B0, n))
        bf.eta[:, n:].zero_()
    fresp_h = np.array([r.resp for r in reqs], dtype=np.int32)
    fmask_h = np.array([r.mask for r in reqs], dtype=np.int32)
    fit_resp = torch.from_numpy(fresp_h).to(dev)
    fit_mask = torch.from_numpy(fmask_h).to(dev)
    ts_h = np.concatenate([[0.0, 1.0, 0.5, 0.25, 0.125], E.TV2.astype(np.float32)])
    nts = int(ts_h.size)
    ts_all = torch.from_numpy(ts_h.astype(np.float64)).to(dev)
    tv1, tv2 = ts_all[:5].float(), ts_all[5:].float()
    l1_d, l2_d = torch.from_numpy(l1).to(dev), torch.from_numpy(l2).to(dev)
    fi_d = torch.from_numpy(fi).to(dev)
    rows = np.array([prob.mask_stats(r.resp, r.mask)[0] for r in reqs], dtype=np.float64)

    # what _syrk / _link_weights read (see engine.irls)
    bf.prob, bf.fit_mask, bf.fit_mask_d, bf.up = prob, fmask_h, fit_mask, up
    bf.wlink = (fam, power, n, ld, prob.Y, prob.M, fit_resp, fit_mask)
    bf.mixS = {}
    nsteps = (n + 31) // 32
    ntile1 = (P // 256) * (P // 256 + 1) // 2

    rp_buf = E._work(3 * E.pad_to(B0, 32) * ld * 2, dev, "rp")
    gx_work = E._work(_lib.query("sglm_xtr_bits_packed_work_bytes", P, B0, ld), dev, "xtr")
    row_work = E._work(_lib.query("sglm_rowsum_work_bytes", B0, 8, n), dev)
    chunk = max(1, min(B0, int(Q_BUDGET // (8.0 * p * p))))
    Q = E._work(chunk * p * p * 8, dev, "pnQ")
    qv = torch.empty((B0, p), dtype=torch.float64, device=dev)
    u = torch.empty((B0, p), dtype=torch.float64, device=dev)
    Ltr = torch.zeros(B0 * 8, dtype=torch.float64, device=dev)
    # the iteration's record, read back with one copy: for its na active fits the trial losses
    # [na][5] f64, the step record [na][4 + 2 nts] f64, the sweeps [na][2] and non-zero counts
    # [na] i32, dmax [na] f32 (the kernels write through pointers into it)
    nrec = 4 + 2 * nts
    rec_d = torch.zeros(B0 * (8 * (5 + nrec) + 16), dtype=torch.uint8, device=dev)
    rec_h = E._pinned("pnrec", rec_d.numel(), torch.uint8)

    active = np.ones(B0, dtype=bool)
    n_iter = np.zeros(B0, dtype=np.int64)
    converged = np.zeros(B0, dtype=bool)
    prev_rel = np.full(B0, np.inf)
    max_iter = np.array([max(1, int(r.max_iter)) for r in reqs])
    ts = np.array([0.0, 1.0, 0.5, 0.25, 0.125])
    ts2 = E.TV2.astype(np.float32).astype(np.float64)

    @contextlib.contextmanager
    def timed(name):
        """Device events around the new kernels' launches (stats.record only: tools)."""
        if stats is None or not stats.record:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        stats.pn_events.append((name, e0, e1))

    try:
        for it in range(int(max_iter.max()) + 1):
            act = np.flatnonzero(active)
            na = int(act.size)
            if na == 0:
                break
            bp = E.pad_to(na, 32)
            act_d = up(act, np.int32)
            sel_d = up(act, np.int64)
            # ---- gradient: the link (packed R), then X^T R exactly summed in float64
            _lib.call("sglm_link_update", fam, power, n, ld, na, _p(act_d), _p(bf.eta),
                      _p(prob.Y), _p(prob.M), _p(fit_resp), _p(fit_mask), None, None,
                      _p(rp_buf), None, None, st)
            _lib.call("sglm_xtr_bits_packed_bp", _p(d.cbits_full()), ld, P, n, _p(rp_buf), na,
                      bp, _p(act_d), _p(bf.g), _p(gx_work), st)
            # ---- Hessian: each active fit's own weighted Gram at its own predictor
            E._syrk(d, bf, act.astype(np.int32), nsteps, ntile1, stats, st, rows=rows)
            # ---- quadratic model and its warm-started coordinate descent, in chunks
            o_l = 0
            o_r = o_l + 8 * na * 5
            o_s = o_r + 8 * na * nrec
            o_z = o_s + 4 * na * 2
            o_m = o_z + 4 * na
            o_e = o_m + 4 * na
            Lrec = rec_d[o_l:o_r].view(torch.float64)
            rec = rec_d[o_r:o_s].view(torch.float64)
            sweeps = rec_d[o_s:o_z].view(torch.int32)
            nnz = rec_d[o_z:o_m].view(torch.int32)
            dmax_d = rec_d[o_m:o_e].view(torch.float32)
            l1a, l2a, fia = l1_d[sel_d], l2_d[sel_d], fi_d[sel_d]
            u[:na] = beta64_d[sel_d, :p]
            for c0 in range(0, na, chunk):
                nc = min(chunk, na - c0)
                with timed("sglm_pn_model"):
                    _lib.call("sglm_pn_model", _p(bf.H), P, p, _p(act_d[c0:]), _p(fia[c0:]), nc,
                              _p(bf.g), _p(beta64_d), _p(Q), _p(qv[c0:]), st)
                with timed("sglm_enet_cd_warm"):
                    _lib.call("sglm_enet_cd_warm", _p(Q), p, nc, _p(qv[c0:]), _p(l1a[c0:]),
                              _p(l2a[c0:]), CD_MAX_SWEEPS, CD_TOL, _p(u[c0:]),
                              _p(sweeps[2 * c0:]), _p(nnz[c0:]), st)
            # ---- direction, Armijo decrease, trial penalties, KKT violation
            with timed("sglm_pn_step"):
                _lib.call("sglm_pn_step", _p(bf.H), P, p, _p(act_d), _p(fia), na, _p(bf.g),
                          _p(beta64_d), _p(u), _p(l1a), _p(l2a), _p(ts_all), nts, _p(bf.delta),
                          _p(rec), st)
            # X delta with the f32 direction as it is (three bf16 pieces): at t = 1 the
            # coefficients become u itself, zeros included, and eta follows to f32 rounding
            d.eta(bf.delta, bf.deta, slots=act_d, direction=False)
            _lib.call("sglm_loss_trials_max", fam, power, n, ld, na, _p(act_d), _p(bf.eta),
                      _p(bf.deta), _p(prob.Y), _p(prob.M), _p(fit_resp), _p(fit_mask), _p(tv1),
                      5, _p(Lrec), _p(dmax_d), _p(row_work), st)
            rec_h[:o_e].copy_(rec_d[:o_e], non_blocking=True)
            torch.cuda.current_stream().synchronize()          # the iteration's round trip
            up.synced()
            if stats is not None:
                stats.roundtrips += 1
            rn = rec_h.numpy()
            L = rn[o_l:o_r].view(np.float64).reshape(na, 5).copy()
            sc = rn[o_r:o_s].view(np.float64).reshape(na, nrec).copy()
            sw = rn[o_s:o_z].view(np.int32).reshape(na, 2).copy()
            db, dec, maxd = np.abs(sc[:, 0]), sc[:, 1], sc[:, 3]
            pen, maxb = sc[:, 4:4 + nts], sc[:, 4 + nts:4 + 2 * nts]
            # ---- line search: Armijo on loss + penalty over t = 1, 1/2, 1/4, 1/8, then TV2
            step_a = np.zeros(na)
            tix = np.zeros(na, dtype=np.int64)
            obj = L + pen[:, :5]
            ok = ((obj[:, 1:] - obj[:, :1] <= E.ARMIJO_SIGMA * ts[None, 1:] * dec[:, None]) |
                  (np.abs(obj[:, 1:] - obj[:, :1]) <= 1e-13 * np.abs(obj[:, :1])))
            first = np.argmax(ok, axis=1)
            hit = ok[np.arange(na), first]
            step_a[hit] = ts[1:][first[hit]]
            tix[hit] = 1 + first[hit]
            # a direction that moves no coefficient, and the intercept by no more than the
            # tolerance, is the f32 predictor's noise in g_p: it is not taken (an all-zero fit
            # ends on its closed-form intercept exactly, a refit from a solution where it began)
            stay = (maxd == 0.0) & (db <= tol)
            more = np.flatnonzero(~hit & ~stay)
            if more.size:
                sub_d = up(act[more], np.int32)
                _lib.call("sglm_loss_trials", fam, power, n, ld, int(more.size), _p(sub_d),
                          _p(bf.eta), _p(bf.deta), _p(prob.Y), _p(prob.M), _p(fit_resp),
                          _p(fit_mask), _p(tv2), 7, _p(Ltr), _p(row_work), st)
                L2 = Ltr[: more.size * 7].view(more.size, 7).cpu().numpy()
                if stats is not None:
                    stats.roundtrips += 1
                o2 = L2 + pen[more, 5:]
                ok2 = o2 - obj[more, :1] <= E.ARMIJO_SIGMA * ts2[None, :] * dec[more, None]
                f2 = np.argmax(ok2, axis=1)
                h2 = ok2[np.arange(more.size), f2]
                step_a[more[h2]] = ts2[f2[h2]]
                tix[more[h2]] = 5 + f2[h2]
            # ---- the engine's step rule on t delta (see engine.irls)
            scale = np.maximum(maxb[np.arange(na), tix], E.STOP_SCALE_FLOOR)
            prop = np.maximum(maxd / scale, db)
            step_a[stay] = 0.0
            relv = step_a * prop
            ls_fail = (step_a == 0.0) & ~stay
            stop_tol = stay | (~ls_fail & (relv <= tol))
            stop_stag = (~ls_fail & ~stop_tol & (relv < 1e-4) & (relv >= 0.5 * prev_rel[act]))
            stop = stop_tol | stop_stag | ls_fail
            conv_now = stop_tol | (ls_fail & (prop <= tol))
            n_iter[act] += 1
            out_of_iters = ~stop & (n_iter[act] >= max_iter[act])
            step_d = up(step_a, np.float64)
            t32_d = up(step_a, np.float32)
            _lib.call("sglm_pn_update", P, p, _p(act_d), na, _p(step_d), _p(u), _p(rec), nrec,
                      _p(beta64_d), st)
            _lib.call("sglm_eta_axpy", n, ld, na, _p(act_d), _p(t32_d), _p(bf.deta),
                      _p(bf.eta), st)
            if stats is not None:
                stats.newton_iters += 1
                stats.fit_iters += na
                stats.gram_fits += na
                stats.gram_fit_iters += na
                stats.pn_fit_iters += na
                stats.cd_full_sweeps += int(sw[:, 0].sum())
                stats.cd_active_sweeps += int(sw[:, 1].sum())
                stats.stops["tol"] += int(np.sum(stop_tol))
                stats.stops["stagnation"] += int(np.sum(stop_stag))
                stats.stops["line_search_converged"] += int(np.sum(ls_fail & (prop <= tol)))
                stats.stops["line_search_failed"] += int(np.sum(ls_fail & (prop > tol)))
                stats.stops["max_iter"] += int(np.sum(out_of_iters))
            prev_rel[act] = relv
            active[act[stop | out_of_iters]] = False
            converged[act[stop]] = conv_now[stop]
        # the final predictor from the final coefficients (the scores read it)
        bf.beta[:B0].copy_(beta64_d)
        d.eta(bf.beta, bf.eta)
        out_beta = beta64_d.cpu().numpy()
    finally:
        bf.prob = bf.keep = bf.up = bf.fit_mask_d = bf.wlink = None
        bf.mixS = None
    res = [E.FitResult(coef=out_beta[k, :p].copy(),
                       intercept=float(out_beta[k, p]) if r.fit_intercept else 0.0,
                       n_iter=int(n_iter[k]), converged=bool(converged[k]))
           for k, r in enumerate(reqs)]
    return res, bf.eta
