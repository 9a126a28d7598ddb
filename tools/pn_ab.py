"""A/B of the Poisson CV grid with and without an L1 term, on the C3-size workload.

Shape: 100k rows x 500 predictors (25 events x 20 lags, sglm_hip.synth), a device-resident
lag design, 5 trial-id splits x 20 alphas (logspace(-4, 1)) + the 20 refits = 120 fits, one GPU.

Two variants, interleaved in one process (alternating order), median of --runs timed runs after
--warmup untimed ones, each a host clock around work that ends in a device synchronise:

  pn    l1_ratio = 0.5: the proximal Newton solve (sglm_hip/pn.py)
  irls  l1_ratio = 0:   the same grid on the IRLS path, as it has always run

After the timed runs each variant runs once more with statistics (and, for pn, device events
around the three new kernels): outer iterations, coordinate-descent sweeps split into full and
restricted, and the share of the grid's wall time spent in the new kernels.  Writes one JSON
file.

    python tools/pn_ab.py --out profiles/pn_ab.json
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
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--events", type=int, default=25)
    ap.add_argument("--L", type=int, default=10, help="lags -L .. L-1")
    ap.add_argument("--splits", type=int, default=5)
    ap.add_argument("--alphas", type=int, default=20)
    ap.add_argument("--l1-ratio", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pn_ab.json"))
    a = ap.parse_args()

    import pandas as pd
    import torch
    from sglm_hip import engine as E, folds, grid, synth
    from sglm_hip.estimators import PoissonRegressor
    E.require_gpu()
    s = synth.make(N=a.rows, m=a.events, L=a.L, family="poisson", rho=0.02, seed=0)
    design = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    codes = folds.trial_keys_codes(pd.DataFrame({"nTrial": s.trial}), ["nTrial"]).values
    np.random.seed(3)
    cv_idx = folds.cv_idx_from_bucket_ids(codes, num_folds=a.splits)
    alphas = np.logspace(-4, 1, a.alphas)
    objs = {"pn": [PoissonRegressor(alpha=float(al), l1_ratio=a.l1_ratio).objective()
                   for al in alphas],
            "irls": [PoissonRegressor(alpha=float(al)).objective() for al in alphas]}
    assert all(o.kind == k for k, v in objs.items() for o in v)
    rolls = [0] * a.alphas

    def run(k, stats=None):
        return grid.run(design, s.y, cv_idx, objs[k], rolls, stats=stats)

    times = {k: [] for k in objs}
    order = list(objs)
    for it in range(a.warmup + a.runs):
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append(time.perf_counter() - t0)
        order = order[::-1]

    detail = {}
    for k in objs:
        st = E.IrlsStats(record=(k == "pn"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(k, st)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        d = {"outer_iterations": int(st.newton_iters), "fit_iterations": int(st.fit_iters),
             "roundtrips": int(st.roundtrips), "stops": dict(st.stops),
             "converged": bool(all(r["converged"] for r in out)),
             "max_fit_iterations": int(max(max(r["n_iter"]) for r in out)),
             "nonzero_refit_coefs": [int(np.count_nonzero(r["refit_coef"])) for r in out]}
        if k == "pn":
            ker = {}
            for name, e0, e1 in st.pn_events:
                ker[name] = ker.get(name, 0.0) + e0.elapsed_time(e1)
            d["cd_sweeps"] = {"full": int(st.cd_full_sweeps), "active": int(st.cd_active_sweeps)}
            d["recorded_run_ms"] = round(wall * 1e3, 2)
            d["kernel_ms"] = {n: round(v, 3) for n, v in ker.items()}
            d["kernel_share_of_recorded_run"] = {n: round(v / (wall * 1e3), 4)
                                                 for n, v in ker.items()}
        detail[k] = d

    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {
        "shape": {"rows": int(design.n), "p": int(design.p), "P": int(design.P),
                  "events": a.events, "lags": 2 * a.L, "splits": a.splits, "alphas": a.alphas,
                  "fits": (a.splits + 1) * a.alphas, "l1_ratio": a.l1_ratio,
                  "alpha_range": [float(alphas[0]), float(alphas[-1])]},
        "device": torch.cuda.get_device_name(0),
        "runs": a.runs, "warmup": a.warmup,
        "ms_per_grid": {k: [round(t * 1e3, 2) for t in v] for k, v in times.items()},
        "median_ms": {k: round(v * 1e3, 2) for k, v in med.items()},
        "spread_ms": {k: round(float(max(v) - min(v)) * 1e3, 2) for k, v in times.items()},
        "pn_over_irls": round(med["pn"] / med["irls"], 3),
        "detail": detail,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
