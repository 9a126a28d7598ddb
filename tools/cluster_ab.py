"""What cluster-robust inference costs next to the fit it follows and next to the 'robust' and
'model' covariances, on the C3-size workload.

Shape: 100k rows x 500 predictors (25 events x 20 lags, sglm_hip.synth), a device-resident lag
design, Poisson fits at 1 and at 20 alphas (logspace(-4, 1)), one GPU; --trials contiguous trials
of equal length are the clusters (1000 of 100 rows by default).

For each model count, interleaved in one process (alternating order): the fits alone
(engine.irls) and the fits followed by inference.infer_problem with per-event Wald groups, for
'model', 'robust' and 'cluster'; median of --runs timed runs after --warmup untimed ones, each a host clock around
work that ends in a device synchronise.  A last instrumented run per (count, cov_type) puts
device events around every C ABI call inference makes and reports the time per entry point;
"cluster_kernels_ms" is the split between the three entry points of csrc/cluster.hip.
There is no bar: the output states the cost of inference as a multiple of the fit.

Writes one JSON file.

    python tools/infer_ab.py --out profiles/cluster_ab.json
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
    ap.add_argument("--trials", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_ab.json"))
    a = ap.parse_args()
    for q in (ROOT, os.path.join(ROOT, "sabatinilab-glm_amd")):
        if q not in sys.path:
            sys.path.insert(0, q)

    import torch
    from sglm_hip import _lib, engine as E, inference, synth
    E.require_gpu()
    s = synth.make(N=a.rows, m=a.events, L=a.L, family="poisson", rho=0.02, seed=0)
    design = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    prob = E.Problem(design, [s.y], [np.ones(design.n, np.uint8)])
    n, p = design.n, design.p
    # one Wald group per event: its 2 L shifted columns
    cols = np.arange(p)
    ev = cols % a.events if design.lag is not None and design.lag.layout == 0 else cols // (2 * a.L)
    ids, goff, gcols, sizes = inference.group_lists(ev, p)
    trial = np.arange(n) // -(-n // a.trials)
    runs = inference.cluster_runs(trial, n)
    cov_types = ("model", "robust", "cluster")

    def fit(alphas):
        reqs = [E.FitReq(E.FAM_TWEEDIE_LOG, 1.0, float(al) * n, 0, 0) for al in alphas]
        res, _ = E.irls(prob, reqs)
        return reqs, res

    def infer(reqs, res, cov_type):
        B = len(reqs)
        return inference.infer_problem(
            prob, [r.family for r in reqs], [r.power for r in reqs], [r.lam for r in reqs],
            [True] * B, [r.coef for r in res], [r.intercept for r in res], [0] * B, [0] * B,
            goff, gcols, cov_type, runs=runs if cov_type == "cluster" else None)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    out = {"shape": {"rows": int(n), "p": int(p), "P": int(design.P), "events": a.events,
                     "lags": 2 * a.L, "groups": int(len(ids)), "group_columns": int(sizes.max()),
                     "clusters": int(runs.G), "runs_of_rows": int(runs.R)},
           "device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup,
           "family": "poisson", "models": {}}
    real_call = _lib.call
    for count in (1, 20):
        alphas = np.logspace(-4, 1, count) if count > 1 else np.array([1e-3])
        variants = ["fit"] + [f"fit+{c}" for c in cov_types]
        times = {v: [] for v in variants}
        order = list(variants)
        for it in range(a.warmup + a.runs):
            for v in order:
                def work():
                    reqs, res = fit(alphas)
                    if v != "fit":
                        infer(reqs, res, v[4:])
                t, _ = timed(work)
                if it >= a.warmup:
                    times[v].append(t)
            order = order[::-1]
        med = {v: float(np.median(t)) for v, t in times.items()}
        rec = {"alphas": [float(x) for x in alphas],
               "ms": {v: [round(x * 1e3, 2) for x in t] for v, t in times.items()},
               "median_ms": {v: round(m * 1e3, 2) for v, m in med.items()},
               "spread_ms": {v: round((max(t) - min(t)) * 1e3, 2) for v, t in times.items()},
               "inference_over_fit": {v[4:]: round((med[v] - med["fit"]) / med["fit"], 3)
                                      for v in variants[1:]},
               "entry_points_ms": {}}
        # one instrumented run per cov_type: device events around every ABI call of inference
        reqs, res = fit(alphas)
        for c in cov_types:
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
                infer(reqs, res, c)
            finally:
                _lib.call = real_call
            torch.cuda.synchronize()
            per = {}
            for name, e0, e1 in evs:
                k = per.setdefault(name, [0, 0.0])
                k[0] += 1
                k[1] += e0.elapsed_time(e1)
            rec["entry_points_ms"][c] = {k: {"calls": v[0], "ms": round(v[1], 3)}
                                         for k, v in per.items()}
        rec["cluster_kernels_ms"] = {k: v["ms"] for k, v in rec["entry_points_ms"]["cluster"].items()
                                     if k in ("sglm_infer_scores", "sglm_cluster_scores",
                                              "sglm_cluster_meat")}
        out["models"][str(count)] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
