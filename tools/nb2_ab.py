"""NB2 (negative binomial, log link, kappa = 1) next to Poisson on the C3-size workload, and the
NB2 trial-loss branches.

Shape: 100k rows x 500 predictors (25 events x 20 lags, sglm_hip.synth), a device-resident lag
design, 5 trial-id splits x 20 alphas (logspace(-4, 1)) + the 20 refits = 120 fits, one GPU.

1. Grids.  On the one resident design, the Poisson grid on Poisson counts (the yardstick, as it
   has always run) and the NB2 grid (--kappa, default 1) on Gamma-Poisson counts drawn from the
   same predictor, interleaved in one process (alternating order), median of --runs timed runs
   after --warmup untimed ones, each a host clock around work that ends in a device synchronise.
   With --poisson-only the script runs on a tree without the NB2 family: run so from a checkout
   of the parent commit (--root) and from this tree, alternating, and pass the files they write
   as --parent-record / --self-record: the Poisson grid alone in its process at both commits is
   carried into the output (the interleaved figure shares its process with the NB2 grids).

2. Trial-loss kernel.  sglm_loss_trials_max at family 3, T = 5, on 120 fits x 100k rows: the step
   lengths {0, 1, 1/2, 1/4, 1/8} (the difference branch) against the same lengths with the last
   one moved by one ulp (the general float64 branch, the same arithmetic otherwise), interleaved,
   device events around each launch, median of --kernel-runs.

Writes one JSON file.

    python tools/nb2_ab.py --out profiles/nb2_ab.json
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
    ap.add_argument("--root", default=ROOT, help="tree whose engine is measured")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--events", type=int, default=25)
    ap.add_argument("--L", type=int, default=10, help="lags -L .. L-1")
    ap.add_argument("--splits", type=int, default=5)
    ap.add_argument("--alphas", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-runs", type=int, default=30)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--poisson-only", action="store_true")
    ap.add_argument("--parent-record", nargs="*", default=[],
                    help="JSON files written by --poisson-only runs of the parent commit")
    ap.add_argument("--self-record", nargs="*", default=[],
                    help="JSON files written by --poisson-only runs of this tree (the Poisson "
                         "grid alone in its process, as the parent's runs have it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nb2_ab.json"))
    a = ap.parse_args()
    for q in (a.root, os.path.join(a.root, "sabatinilab-glm_amd")):
        if q not in sys.path:
            sys.path.insert(0, q)

    import pandas as pd
    import torch
    from sglm_hip import _lib, engine as E, folds, grid, synth
    from sglm_hip.estimators import Objective
    E.require_gpu()
    s = synth.make(N=a.rows, m=a.events, L=a.L, family="poisson", rho=0.02, seed=0)
    design = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    codes = folds.trial_keys_codes(pd.DataFrame({"nTrial": s.trial}), ["nTrial"]).values
    np.random.seed(3)
    cv_idx = folds.cv_idx_from_bucket_ids(codes, num_folds=a.splits)
    alphas = np.logspace(-4, 1, a.alphas)
    rolls = [0] * a.alphas
    objs = {"poisson": [Objective("irls", E.FAM_TWEEDIE_LOG, 1.0, float(al), "n", True, 100)
                        for al in alphas]}
    ys = {"poisson": s.y}
    if not a.poisson_only:
        # Gamma-Poisson counts from the design's own predictor (the events and coefficients of
        # the Poisson counts, intercept -1)
        eta = np.full(s.N, s.intercept)
        Bm = s.beta.reshape(len(s.shifts), a.events)
        for bi, sh in enumerate(s.shifts):
            r0 = s.L - 1 - sh
            eta += s.E[r0:r0 + s.N].astype(np.float64) @ Bm[bi]
        kappa = float(np.float32(a.kappa))
        rg = np.random.default_rng(2)
        ys["nb2"] = rg.poisson(np.exp(eta) * rg.gamma(1.0 / kappa, kappa, s.N)).astype(np.float64)
        objs["nb2"] = [Objective("irls", E.FAM_NB2_LOG, kappa, float(al), "n", True, 100)
                       for al in alphas]

    def run(k, stats=None):
        return grid.run(design, ys[k], cv_idx, objs[k], rolls, stats=stats)

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
        st = E.IrlsStats()
        out = run(k, st)
        detail[k] = {"newton_iterations": int(st.newton_iters), "fit_iterations": int(st.fit_iters),
                     "gram_fits": int(st.gram_fits), "lag_grams": int(st.lag_grams),
                     "aliased": int(st.aliased), "reused": int(st.reused),
                     "converged": bool(all(r["converged"] for r in out)),
                     "max_fit_iterations": int(max(max(r["n_iter"]) for r in out)),
                     "mean_y": float(np.mean(ys[k])), "var_y": float(np.var(ys[k]))}
    res = {
        "shape": {"rows": int(design.n), "p": int(design.p), "P": int(design.P),
                  "events": a.events, "lags": 2 * a.L, "splits": a.splits, "alphas": a.alphas,
                  "fits": (a.splits + 1) * a.alphas,
                  "alpha_range": [float(alphas[0]), float(alphas[-1])]},
        "device": torch.cuda.get_device_name(0),
        "runs": a.runs, "warmup": a.warmup,
        "grid_ms": {k: [round(t * 1e3, 2) for t in v] for k, v in times.items()},
        "grid_median_ms": {k: round(float(np.median(v)) * 1e3, 2) for k, v in times.items()},
        "grid_spread_ms": {k: round(float(max(v) - min(v)) * 1e3, 2) for k, v in times.items()},
        "grid_detail": detail,
    }
    def alone(files, note):
        recs = []
        for fn in files:
            with open(fn) as f:
                pr = json.load(f)
            recs.append({"median_ms": pr["grid_median_ms"]["poisson"],
                         "ms": pr["grid_ms"]["poisson"],
                         "spread_ms": pr["grid_spread_ms"]["poisson"], "device": pr["device"]})
        return {"processes": recs, "note": note,
                "median_of_medians_ms": round(float(np.median([q["median_ms"] for q in recs])), 2)}
    if a.parent_record:
        res["poisson_grid_at_parent_commit"] = alone(
            a.parent_record, "the same script with --poisson-only on a checkout of the parent "
            "commit, one process per record, alternating with this commit's on one device")
    if a.self_record:
        res["poisson_grid_alone_at_this_commit"] = alone(
            a.self_record, "the same script with --poisson-only on this tree, one process per "
            "record: the like-for-like figure next to the parent's")

    if not a.poisson_only:
        # ---- the T = 5 trial-loss kernel: difference branch against the general branch
        n, ld, B = design.n, design.ld, (a.splits + 1) * a.alphas
        rng = np.random.default_rng(5)
        dev = design.device
        Y = torch.zeros((1, ld), dtype=torch.float32, device=dev)
        Y[0, :n] = torch.from_numpy(ys["nb2"].astype(np.float32)).to(dev)
        M = torch.zeros((2, ld), dtype=torch.uint8, device=dev)
        M[0, :n] = 1
        M[1, :n] = torch.from_numpy((rng.random(n) < 0.8).astype(np.uint8)).to(dev)
        fr = torch.zeros(B, dtype=torch.int32, device=dev)
        # five fold fits (the 0.8 mask) to one refit (every row)
        fm = torch.from_numpy((np.arange(B) % 6 != 5).astype(np.int32)).to(dev)
        eta = torch.zeros((B, ld), dtype=torch.float32, device=dev)
        deta = torch.zeros((B, ld), dtype=torch.float32, device=dev)
        eta[:, :n] = torch.from_numpy(rng.normal(-1.0, 1.0, (B, n)).astype(np.float32)).to(dev)
        deta[:, :n] = torch.from_numpy(rng.normal(0.0, 0.3, (B, n)).astype(np.float32)).to(dev)
        tv = {"difference": np.array([0, 1, .5, .25, .125], dtype=np.float32)}
        tv["general"] = tv["difference"].copy()
        tv["general"][4] = np.nextafter(np.float32(.125), np.float32(1))
        tvd = {k: torch.from_numpy(v).to(dev) for k, v in tv.items()}
        out = torch.zeros(B * 5, dtype=torch.float64, device=dev)
        dm = torch.zeros(B, dtype=torch.float32, device=dev)
        wk = torch.empty(_lib.query("sglm_rowsum_work_bytes", B, 8, n), dtype=torch.uint8,
                         device=dev)
        st = E._stream()

        def launch(k):
            _lib.call("sglm_loss_trials_max", E.FAM_NB2_LOG, kappa, n, ld, B, None,
                      eta.data_ptr(), deta.data_ptr(), Y.data_ptr(), M.data_ptr(), fr.data_ptr(),
                      fm.data_ptr(), tvd[k].data_ptr(), 5, out.data_ptr(), dm.data_ptr(),
                      wk.data_ptr(), st)
        kt = {k: [] for k in tv}
        sums = {}
        order = list(tv)
        for it in range(5 + a.kernel_runs):
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(k)
                e1.record()
                e1.synchronize()
                if it >= 5:
                    kt[k].append(e0.elapsed_time(e1))
                sums[k] = out.view(B, 5).cpu().numpy().copy()
            order = order[::-1]
        guard = float((deta[:, :n].abs() > 3).float().mean())
        dd = sums["difference"][:, 1:] - sums["difference"][:, :1]
        dg = sums["general"][:, 1:] - sums["general"][:, :1]
        res["trial_loss_kernel"] = {
            "fits": B, "rows": int(n), "runs": a.kernel_runs,
            "includes": "the kernel, the dmax memset and the chunk reduction of one call",
            "median_us": {k: round(float(np.median(v)) * 1e3, 1) for k, v in kt.items()},
            "min_us": {k: round(float(np.min(v)) * 1e3, 1) for k, v in kt.items()},
            "max_us": {k: round(float(np.max(v)) * 1e3, 1) for k, v in kt.items()},
            "general_over_difference": round(float(np.median(kt["general"])
                                                   / np.median(kt["difference"])), 3),
            "rows_on_float64_guard": guard,
            "max_rel_gap_of_differences": float(np.max(np.abs(dd - dg) / np.abs(dg))),
        }
        gm = res["grid_median_ms"]
        res["kappa"] = kappa
        res["nb2_over_poisson"] = round(gm["nb2"] / gm["poisson"], 3)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
