"""NB2 dispersion by maximum likelihood and the 'll' score on the C3-size workload.

Shape: 100k rows x 500 predictors (25 events x 20 lags, sglm_hip.synth), a device-resident lag
design, 5 trial-id splits x 20 alphas (logspace(-4, 1)) + the 20 refits = 120 fits, one GPU.
Gamma-Poisson counts (--kappa, default 1) drawn from the design's own predictor, as tools/nb2_ab.py
draws them.

1. ML fit.  NegativeBinomialRegressor(kappa='ml', alpha=--alpha) on the resident design next to
   the fixed-kappa fit at the kappa_ it finds, interleaved, median of --runs host-clocked runs.
2. Kernel.  sglm_nb2_kappa_sums on 120 fits x 100k rows (five fold fits on a 0.8 mask to one
   refit on every row) at K = 1 and K = 4, interleaved, device events around each call (kernel
   and chunk reduction), median of --kernel-runs, and the GB/s it implies on 9 B per row per fit
   (f32 eta, f32 y, one mask byte).
3. Grids.  The NB2 grid at score_method='ll' next to 'mse', interleaved.
4. With --poisson-only: the Poisson 'mse' grid alone in its process.  Run so from a checkout of
   the parent commit (--root) and from this tree, alternating, and pass the files as
   --parent-record / --self-record (as tools/nb2_ab.py does).

    python tools/nb2_kappa_ab.py --out profiles/nb2_kappa_ab.json
"""
import argparse
import json
import os
import sys
import time
import warnings

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
    ap.add_argument("--alpha", type=float, default=1e-2, help="penalty of the ML fit")
    ap.add_argument("--poisson-only", action="store_true")
    ap.add_argument("--parent-record", nargs="*", default=[])
    ap.add_argument("--self-record", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nb2_kappa_ab.json"))
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
    res = {
        "shape": {"rows": int(design.n), "p": int(design.p), "P": int(design.P),
                  "events": a.events, "lags": 2 * a.L, "splits": a.splits, "alphas": a.alphas,
                  "fits": (a.splits + 1) * a.alphas,
                  "alpha_range": [float(alphas[0]), float(alphas[-1])]},
        "device": torch.cuda.get_device_name(0),
        "runs": a.runs, "warmup": a.warmup,
    }

    def timed(fns):
        """{name: [seconds]} of the callables, interleaved in alternating order."""
        times = {k: [] for k in fns}
        order = list(fns)
        for it in range(a.warmup + a.runs):
            for k in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fns[k]()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append(time.perf_counter() - t0)
            order = order[::-1]
        return times

    def summary(times):
        return {"ms": {k: [round(t * 1e3, 2) for t in v] for k, v in times.items()},
                "median_ms": {k: round(float(np.median(v)) * 1e3, 2) for k, v in times.items()},
                "spread_ms": {k: round(float(max(v) - min(v)) * 1e3, 2)
                              for k, v in times.items()}}

    pois = [Objective("irls", E.FAM_TWEEDIE_LOG, 1.0, float(al), "n", True, 100) for al in alphas]
    if a.poisson_only:
        t = summary(timed({"poisson": lambda: grid.run(design, s.y, cv_idx, pois, rolls)}))
        res.update({"grid_ms": t["ms"], "grid_median_ms": t["median_ms"],
                    "grid_spread_ms": t["spread_ms"]})
    else:
        from sglm_hip.estimators import NegativeBinomialRegressor
        eta = np.full(s.N, s.intercept)
        Bm = s.beta.reshape(len(s.shifts), a.events)
        for bi, sh in enumerate(s.shifts):
            r0 = s.L - 1 - sh
            eta += s.E[r0:r0 + s.N].astype(np.float64) @ Bm[bi]
        kappa = float(np.float32(a.kappa))
        rg = np.random.default_rng(2)
        y = rg.poisson(np.exp(eta) * rg.gamma(1.0 / kappa, kappa, s.N)).astype(np.float64)

        # ---- 1. the ML fit next to the fixed-kappa fit at its kappa_, on the resident design
        # shape only (no host values are read: the design is resident)
        X = np.broadcast_to(np.float32(0), (design.n, design.p))
        ml = NegativeBinomialRegressor(kappa="ml", alpha=a.alpha)
        ml._resident = {id(X): (X, design)}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ml.fit(X, y)
        fx = NegativeBinomialRegressor(kappa=ml.kappa_, alpha=a.alpha)
        fx._resident = ml._resident
        t = summary(timed({"ml": lambda: ml.fit(X, y), "fixed": lambda: fx.fit(X, y)}))
        res["ml_fit"] = {"alpha": a.alpha, "kappa_generating": kappa, "kappa_": ml.kappa_,
                         "rounds": ml.kappa_n_rounds_, "converged": ml.kappa_converged_,
                         "at_bound": ml.kappa_at_bound_, "irls_iterations_ml": ml.n_iter_,
                         "irls_iterations_fixed": fx.n_iter_,
                         "max_coef_gap": float(np.max(np.abs(ml.coef_ - fx.coef_))), **t}

        # ---- 2. sglm_nb2_kappa_sums, K = 1 and K = 4
        n, ld, B = design.n, design.ld, (a.splits + 1) * a.alphas
        rng = np.random.default_rng(5)
        dev = design.device
        Y = torch.zeros((1, ld), dtype=torch.float32, device=dev)
        Y[0, :n] = torch.from_numpy(y.astype(np.float32)).to(dev)
        M = torch.zeros((2, ld), dtype=torch.uint8, device=dev)
        M[0, :n] = 1
        M[1, :n] = torch.from_numpy((rng.random(n) < 0.8).astype(np.uint8)).to(dev)
        fr = torch.zeros(B, dtype=torch.int32, device=dev)
        fm = torch.from_numpy((np.arange(B) % 6 != 5).astype(np.int32)).to(dev)
        et = torch.zeros((B, ld), dtype=torch.float32, device=dev)
        et[:, :n] = torch.from_numpy(rng.normal(-1.0, 1.0, (B, n)).astype(np.float32)).to(dev)
        kd = {K: torch.from_numpy(np.tile(np.array([0.5, 1.0, 2.0, 4.0])[:K], (B, 1))).to(dev)
              for K in (1, 4)}
        out = {K: torch.zeros((B, K, 3), dtype=torch.float64, device=dev) for K in (1, 4)}
        wk = torch.empty(_lib.query("sglm_nb2_kappa_sums_work_bytes", B, 4, n), dtype=torch.uint8,
                         device=dev)
        st = E._stream()
        kt = {K: [] for K in (1, 4)}
        order = [1, 4]
        for it in range(5 + a.kernel_runs):
            for K in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.call("sglm_nb2_kappa_sums", n, ld, B, None, et.data_ptr(), Y.data_ptr(),
                          M.data_ptr(), fr.data_ptr(), fm.data_ptr(), kd[K].data_ptr(), K,
                          out[K].data_ptr(), wk.data_ptr(), st)
                e1.record()
                e1.synchronize()
                if it >= 5:
                    kt[K].append(e0.elapsed_time(e1))
            order = order[::-1]
        nbytes = 9.0 * n * B
        res["kappa_sums_kernel"] = {
            "fits": B, "rows": int(n), "runs": a.kernel_runs,
            "includes": "the kernel and the chunk reduction of one call",
            "bytes_model": "9 B per row per fit (f32 eta, f32 y, one mask byte)",
            "median_us": {f"K{K}": round(float(np.median(v)) * 1e3, 1) for K, v in kt.items()},
            "min_us": {f"K{K}": round(float(np.min(v)) * 1e3, 1) for K, v in kt.items()},
            "max_us": {f"K{K}": round(float(np.max(v)) * 1e3, 1) for K, v in kt.items()},
            "GBps": {f"K{K}": round(nbytes / (float(np.median(v)) * 1e-3) / 1e9, 1)
                     for K, v in kt.items()},
            "finite": bool(all(torch.isfinite(o).all().item() for o in out.values())),
        }

        # ---- 3. the NB2 grid at 'll' next to 'mse'
        nb2 = [Objective("irls", E.FAM_NB2_LOG, kappa, float(al), "n", True, 100) for al in alphas]
        t = summary(timed({m: (lambda m=m: grid.run(design, y, cv_idx, nb2, rolls, score_method=m))
                           for m in ("mse", "ll")}))
        ll = grid.run(design, y, cv_idx, nb2, rolls, score_method="ll")
        res["nb2_grid"] = {"kappa": kappa, **t,
                           "ll_over_mse": round(t["median_ms"]["ll"] / t["median_ms"]["mse"], 3),
                           "best_alpha_by_ll": float(alphas[int(np.argmax(
                               [r["cv_mean_score"] for r in ll]))]),
                           "best_cv_mean_ll": float(max(r["cv_mean_score"] for r in ll))}

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

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
