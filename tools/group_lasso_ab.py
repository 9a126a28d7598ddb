"""A/B of the group-lasso lambda path against the elastic-net path, on the C5 shape.

Shape: 1M rows x 1000 predictors (50 events x 20 lags, sglm_hip.synth), a device-resident lag
design, 64 responses x 20 alphas (logspace(-4, 1)) x (5 trial-id splits + refit) = 7680 fits,
l1_ratio 0.5, one GPU.

Three variants of ``enet.cv_enet_path``, interleaved in one process (the order rotates every
round), median of --runs timed runs after --warmup untimed ones, each a host clock around work
that ends in a device synchronise:

  enet        the elastic-net path (sglm_enet_cd_grouped), as it has always run
  glasso      groups = one per event (50 groups of 20 lag columns): sglm_group_cd_shared
  singletons  groups = one per column: sglm_group_cd_shared on the elastic-net objective --
              the group kernel against the coordinate-descent kernel on the same problem

Every timed run also records the descent stage alone (device events around it; for the group
variants that stage includes sglm_group_bound and the sort of the fits), the sweep counts and
the stage's flop rate at 2 p^2 flop per sweep and fit.  Writes one JSON file.

    python tools/group_lasso_ab.py --out profiles/group_lasso_ab.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in (ROOT, os.path.join(ROOT, "sabatinilab-glm_amd")):
    if q not in sys.path:
        sys.path.insert(0, q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--events", type=int, default=50)
    ap.add_argument("--L", type=int, default=10, help="lags -L .. L-1")
    ap.add_argument("--responses", type=int, default=64)
    ap.add_argument("--splits", type=int, default=5)
    ap.add_argument("--alphas", type=int, default=20)
    ap.add_argument("--l1-ratio", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_lasso_ab.json"))
    a = ap.parse_args()

    import pandas as pd
    import torch
    from sglm_hip import engine as E, enet, folds, synth
    E.require_gpu()
    s = synth.make(N=a.rows, m=a.events, L=a.L, family="gaussian", rho=0.02, seed=0)
    design = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    p = design.p
    rng = np.random.default_rng(5)
    Y = np.stack([s.y + rng.normal(0, 1, s.N) for _ in range(a.responses)], 1)
    Yd = torch.from_numpy(Y).cuda()
    codes = folds.trial_keys_codes(pd.DataFrame({"nTrial": s.trial}), ["nTrial"]).values
    np.random.seed(3)
    cv_idx = folds.cv_idx_from_bucket_ids(codes, num_folds=a.splits)
    alphas = np.logspace(-4, 1, a.alphas)
    # the lag design's columns are shift-major (block b = shift b of every event): column j is
    # a lag of event j mod m
    event_of = np.arange(p) % a.events
    groups = {"enet": None, "glasso": event_of, "singletons": np.arange(p)}

    def run(k, stats=None):
        return enet.cv_enet_path(design, Yd, cv_idx, alphas, l1_ratio=a.l1_ratio, stats=stats,
                                 groups=groups[k])

    recs = {k: [] for k in groups}
    order = list(groups)
    last = {}
    for it in range(a.warmup + a.runs):
        for k in order:
            st = {"record": True}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = run(k, st)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if it >= a.warmup:
                recs[k].append({"wall_ms": round(wall * 1e3, 2),
                                "descent_ms": round(st["cd_ms"], 2),
                                "descent_tflops": round(st["cd_flop"] / (st["cd_ms"] * 1e-3) / 1e12,
                                                        4),
                                "sweeps_total": int(st["cd_sweeps_total"]),
                                "sweeps_max": int(st["cd_sweeps_max"])})
        order = order[1:] + order[:1]

    def med(k, key):
        return float(np.median([r[key] for r in recs[k]]))

    detail = {}
    for k, out in last.items():
        nz = [int(np.count_nonzero(r["refit_coef"])) for per in out for r in per]
        d = {"converged": bool(all(r["converged"] for per in out for r in per)),
             "mean_nonzero_refit_coefs_per_alpha": [
                 round(float(np.mean([np.count_nonzero(out[r][j]["refit_coef"])
                                      for r in range(len(out))])), 1)
                 for j in range(a.alphas)],
             "nonzero_refit_coefs_total": int(np.sum(nz))}
        if k == "glasso":
            d["mean_events_in_refit_per_alpha"] = [
                round(float(np.mean([len(set(event_of[np.flatnonzero(out[r][j]["refit_coef"])]))
                                     for r in range(len(out))])), 1) for j in range(a.alphas)]
        detail[k] = d
    # singleton groups solve the elastic-net objective: the two kernels agree on the refits
    dist = max(float(np.max(np.abs(last["singletons"][r][j]["refit_coef"]
                                   - last["enet"][r][j]["refit_coef"])))
               / max(float(np.max(np.abs(last["enet"][r][j]["refit_coef"]))), 1e-300)
               for r in range(a.responses) for j in range(a.alphas)
               if np.any(last["enet"][r][j]["refit_coef"]))
    fits = a.responses * a.alphas * (a.splits + 1)
    res = {
        "shape": {"rows": int(design.n), "p": int(p), "events": a.events, "lags": 2 * a.L,
                  "responses": a.responses, "splits": a.splits, "alphas": a.alphas, "fits": fits,
                  "l1_ratio": a.l1_ratio, "alpha_range": [float(alphas[0]), float(alphas[-1])]},
        "device": torch.cuda.get_device_name(0),
        "runs": a.runs, "warmup": a.warmup,
        "per_run": recs,
        "median_wall_ms": {k: round(med(k, "wall_ms"), 2) for k in groups},
        "median_descent_ms": {k: round(med(k, "descent_ms"), 2) for k in groups},
        "median_descent_tflops": {k: round(med(k, "descent_tflops"), 4) for k in groups},
        "sweeps_total": {k: recs[k][0]["sweeps_total"] for k in groups},
        "sweeps_max": {k: recs[k][0]["sweeps_max"] for k in groups},
        "glasso_over_enet_wall": round(med("glasso", "wall_ms") / med("enet", "wall_ms"), 3),
        "glasso_over_enet_descent": round(med("glasso", "descent_ms") / med("enet", "descent_ms"),
                                          3),
        "singletons_over_enet_descent": round(med("singletons", "descent_ms")
                                              / med("enet", "descent_ms"), 3),
        "singletons_vs_enet_refit_distance": dist,
        "detail": detail,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
