"""What pointwise bands of the fitted trace cost next to the fit and its inference, on the
C3-size workload, and against the route there was before: the covariance copied to the host and
an einsum over a dense host copy of the design.

Shape: 100k rows x 500 predictors (25 events x 20 lags, sglm_hip.synth), a device-resident lag
design, Poisson fits at 1 and at 20 alphas (logspace(-4, 1)), 'model' covariance, one GPU.

Arms, interleaved in one process (alternating order), median of --runs timed runs after --warmup
untimed ones, each a host clock around work that ends in a device synchronise:
  fit            engine.irls
  fit+infer      + inference.infer_problem with per-event Wald groups (as tools/infer_ab.py)
  fit+bands      + infer_problem handing its device covariance to sglm_predict_rows, eta and
                 variance of every row copied to the host
  fit+bands+ev   + sglm_predict_groups for the 25 events as well
  fit+host       + infer_problem(return_cov=True), then eta and einsum('ij,jk,ik->i') on the
                 host (--host-runs timed runs: it is seconds per fit)
A last instrumented run puts device events around the two new entry points.  There is no bar.

    python tools/predict_ab.py --out profiles/predict_ab.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--events", type=int, default=25)
    ap.add_argument("--L", type=int, default=10, help="lags -L .. L-1")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_ab.json"))
    a = ap.parse_args()
    for q in (ROOT, os.path.join(ROOT, "sabatinilab-glm_amd")):
        if q not in sys.path:
            sys.path.insert(0, q)

    import torch
    from sglm_hip import _lib, engine as E, inference, synth
    E.require_gpu()
    s = synth.make(N=a.rows, m=a.events, L=a.L, family="poisson", rho=0.02, seed=0)
    d = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    prob = E.Problem(d, [s.y], [np.ones(d.n, np.uint8)])
    n, p, P, dev = d.n, d.p, d.P, d.device
    cols = np.arange(p)
    ev = cols % a.events if d.lag is not None and d.lag.layout == 0 else cols // (2 * a.L)
    ids, goff, gcols, sizes = inference.group_lists(ev, p)
    ng = len(ids)
    goff_d = torch.from_numpy(np.asarray(goff, np.int32)).to(dev)
    gcols_d = torch.from_numpy(np.asarray(gcols, np.int32)).to(dev)
    # the dense host copy the old route needs (ones column last), from the design itself
    Xt = d.xb[:p + 1, :n].to(torch.float64).t().contiguous().cpu().numpy()
    ones_per_row = float(Xt.sum(axis=1).mean())

    def fit(alphas):
        reqs = [E.FitReq(E.FAM_TWEEDIE_LOG, 1.0, float(al) * n, 0, 0) for al in alphas]
        res, _ = E.irls(prob, reqs)
        return reqs, res

    def infer(reqs, res, groups=True, **kw):
        B = len(reqs)
        return inference.infer_problem(
            prob, [r.family for r in reqs], [r.power for r in reqs], [r.lam for r in reqs],
            [True] * B, [r.coef for r in res], [r.intercept for r in res], [0] * B, [0] * B,
            goff if groups else None, gcols if groups else None, "model", **kw)

    def bands(reqs, res, events):
        got = {}

        def row_pass(sel, beta_d, cov, state, kap):
            nb = len(sel)
            st = E._stream()
            ic = torch.ones(nb, dtype=torch.int32, device=dev)
            e_d = torch.empty((nb, n), dtype=torch.float64, device=dev)
            v_d = torch.empty((nb, n), dtype=torch.float64, device=dev)
            _lib.call("sglm_predict_rows", E._p(d.rbits), d.ld, P, p, n, None, n, E._p(beta_d),
                      E._p(cov), E._p(state), E._p(ic), nb, E._p(e_d), E._p(v_d), st)
            got["eta"], got["var"] = e_d.cpu().numpy(), v_d.cpu().numpy()
            if events:
                ge = torch.empty((nb, ng, n), dtype=torch.float64, device=dev)
                gv = torch.empty((nb, ng, n), dtype=torch.float64, device=dev)
                _lib.call("sglm_predict_groups", E._p(d.rbits), d.ld, P, p, n, None, n,
                          E._p(beta_d), E._p(cov), E._p(state), nb, E._p(goff_d), E._p(gcols_d),
                          ng, E._p(ge), E._p(gv), st)
                got["geta"], got["gvar"] = ge.cpu().numpy(), gv.cpu().numpy()
        infer(reqs, res, groups=False, _on_chunk=row_pass,
              _extra_bytes=16 * n * (1 + (ng if events else 0)))
        return got

    def host(reqs, res):
        r = infer(reqs, res, groups=False, return_cov=True)
        keep = np.arange(p + 1)
        eta, var = [], []
        for k, fr in enumerate(res):
            C = r["cov"][k][np.ix_(keep, keep)]
            eta.append(Xt @ np.r_[fr.coef, fr.intercept])
            var.append(np.einsum("ij,ij->i", Xt @ C, Xt))      # einsum('ij,jk,ik->i') via BLAS
        return {"eta": np.array(eta), "var": np.array(var)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    out = {"shape": {"rows": int(n), "p": int(p), "P": int(P), "events": a.events,
                     "lags": 2 * a.L, "groups": int(ng), "group_columns": int(sizes.max()),
                     "ones_per_row": round(ones_per_row, 2)},
           "device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup,
           "host_runs": a.host_runs, "family": "poisson", "cov_type": "model", "models": {}}
    real_call = _lib.call
    arms = {"fit": lambda q, r: None, "fit+infer": lambda q, r: infer(q, r),
            "fit+bands": lambda q, r: bands(q, r, False),
            "fit+bands+ev": lambda q, r: bands(q, r, True)}
    for count in (1, 20):
        alphas = np.logspace(-4, 1, count) if count > 1 else np.array([1e-3])
        times = {v: [] for v in arms}
        order = list(arms)
        for it in range(a.warmup + a.runs):
            for v in order:
                def work():
                    reqs, res = fit(alphas)
                    arms[v](reqs, res)
                t, _ = timed(work)
                if it >= a.warmup:
                    times[v].append(t)
            order = order[::-1]
        times["fit+host"] = []
        for it in range(1 + a.host_runs):
            def work():
                reqs, res = fit(alphas)
                return host(reqs, res)
            t, ref = timed(work)
            if it >= 1:
                times["fit+host"].append(t)
        med = {v: float(np.median(t)) for v, t in times.items()}
        reqs, res = fit(alphas)
        evs = []

        def call(name, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real_call(name, *args)
            e1.record()
            evs.append((name, e0, e1))
            return r
        _lib.call = call
        try:
            got = bands(reqs, res, True)
        finally:
            _lib.call = real_call
        torch.cuda.synchronize()
        per = {}
        for name, e0, e1 in evs:
            if name.startswith("sglm_predict"):
                k = per.setdefault(name, [0, 0.0])
                k[0] += 1
                k[1] += e0.elapsed_time(e1)
        terms = ones_per_row * (ones_per_row + 1) / 2 * n * count
        out["models"][str(count)] = {
            "alphas": [float(x) for x in alphas],
            "ms": {v: [round(x * 1e3, 2) for x in t] for v, t in times.items()},
            "median_ms": {v: round(m * 1e3, 2) for v, m in med.items()},
            "spread_ms": {v: round((max(t) - min(t)) * 1e3, 2) for v, t in times.items()},
            "bands_over_fit_infer": round((med["fit+bands"] - med["fit+infer"]) / med["fit+infer"], 3),
            "host_route_over_bands": round((med["fit+host"] - med["fit"])
                                           / (med["fit+bands"] - med["fit"]), 1),
            "entry_points_ms": {k: {"calls": v[0], "ms": round(v[1], 3)} for k, v in per.items()},
            "predict_rows_C_reads_per_s": round(terms / (per["sglm_predict_rows"][1] * 1e-3), 0),
            "output_bytes": {"bands": int(16 * n * count), "bands+ev": int(16 * n * count * (1 + ng))},
            # the same fits through both routes: the new pass against the host einsum
            "max_rel_diff_var_vs_host": float(np.max(np.abs(got["var"] - ref["var"]) / ref["var"])),
            "max_abs_diff_eta_vs_host": float(np.max(np.abs(got["eta"] - ref["eta"]))),
        }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
