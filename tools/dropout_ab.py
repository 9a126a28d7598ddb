"""A/B of the leave-one-event-out CV grid on a production-like synthetic shape.

The reference drivers wrap their whole OLS fit in a loop over leave_one_out_list: the full model,
then one run per event with that event's columns removed.  Shape here: 18 events x 42 lags
(-21 .. 20, sglm_hip.synth), 50 splits + refit, alpha = [0] (LinearRegression), one GPU.

Three variants, interleaved in one process (rotating order), median of --runs timed runs after
--warmup untimed ones, each a host clock around work that ends in a device synchronise:

  a  today's way: grid.run over each column-deleted HOST matrix (a fresh Design per variant)
  b  grid.run(..., drop_sets=...) with SGLM_DROP_ROUTE=exclude (a factor per drop variant)
  c  grid.run(..., drop_sets=...) default (reduced solves off the full model's factor)

b and c start from the host matrix too (their one Design build is inside the timed window).
The outputs of the three variants are compared at the timed size.  Writes one JSON file.

    python tools/dropout_ab.py --out profiles/dropout_ab.json
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
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--events", type=int, default=18)
    ap.add_argument("--L", type=int, default=21, help="lags -L .. L-1")
    ap.add_argument("--splits", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_ab.json"))
    a = ap.parse_args()

    import torch
    from sglm_hip import engine, grid, synth
    from sglm_hip.estimators import LinearRegression
    engine.require_gpu()
    s = synth.make(a.rows, a.events, a.L, family="gaussian", rho=0.02, seed=3)
    X = s.dense_X()
    y = s.y
    n, p = X.shape
    m = a.events
    nlag = p // m
    drops = [[]] + [[b * m + e for b in range(nlag)] for e in range(m)]     # shift-major columns
    rng = np.random.default_rng(4)
    trials = np.unique(s.trial)
    cv = []
    for _ in range(a.splits):
        te_t = rng.choice(trials, size=max(1, len(trials) // 5), replace=False)
        te = np.isin(s.trial, te_t)
        cv.append((np.flatnonzero(~te), np.flatnonzero(te)))
    objs, rolls = [LinearRegression().objective()], [0]

    def run_a():
        out = []
        for ds in drops:
            Xd = np.delete(X, ds, axis=1) if ds else X
            out.append(grid.run(Xd, y, cv, objs, rolls))
        return out

    def run_new(route):
        os.environ["SGLM_DROP_ROUTE"] = route
        try:
            return grid.run(X, y, cv, objs, rolls, drop_sets=drops)
        finally:
            os.environ.pop("SGLM_DROP_ROUTE", None)

    variants = {"a": run_a, "b": lambda: run_new("exclude"), "c": lambda: run_new("auto")}
    times = {k: [] for k in variants}
    outs = {}
    order = list(variants)
    for it in range(a.warmup + a.runs):
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = variants[k]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                times[k].append(dt)
            outs[k] = r
        order = order[1:] + order[:1]

    # same results: (a)'s reduced-length coefficients against the kept rows of (b) and (c)
    def maxrel(new):
        worst = 0.0
        for ds, ra, rn in zip(drops, outs["a"], new):
            keep = np.setdiff1d(np.arange(p), ds)
            for u, v in ((ra[0]["cv_coefs"], rn[0]["cv_coefs"][keep]),
                         (ra[0]["refit_coef"], rn[0]["refit_coef"][keep])):
                worst = max(worst, float(np.max(np.abs(u - v)) / np.max(np.abs(u))))
            worst = max(worst, float(np.max(np.abs(ra[0]["cv_scores_test"] - rn[0]["cv_scores_test"])
                                            / np.abs(ra[0]["cv_scores_test"]))))
        return worst

    st = engine.IrlsStats()
    grid.run(X, y, cv, objs, rolls, drop_sets=drops, stats=st)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {
        "shape": {"rows": n, "p": p, "P": int(engine.pad_to(p + 1, engine.COL_PAD)), "events": m,
                  "lags": nlag, "splits": a.splits, "drop_sets": len(drops),
                  "fits": len(drops) * (a.splits + 1), "alpha": [0]},
        "device": torch.cuda.get_device_name(0),
        "runs": a.runs, "warmup": a.warmup,
        "seconds": {k: [round(t, 4) for t in v] for k, v in times.items()},
        "median_s": {k: round(v, 4) for k, v in med.items()},
        "spread_s": {k: round(float(max(v) - min(v)), 4) for k, v in times.items()},
        "speedup_c_over_a": round(med["a"] / med["c"], 3),
        "speedup_c_over_b": round(med["b"] / med["c"], 3),
        "max_rel_diff_vs_a": {"b": maxrel(outs["b"]), "c": maxrel(outs["c"])},
        "default_route_fits": {"reduced": st.drop_reduced, "excluded": st.drop_excluded},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
