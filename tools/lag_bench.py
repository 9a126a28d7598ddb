"""Micro-benchmark of the gradient kernels on the C4 design (development tool), for B active
fits, HIP events on the launch stream:
  bits   sglm_xtr_bits_packed_bp  (bit-plane MFMA, the dense kernel)
  walk   sglm_lag_xtr_packed_bp   (occurrence walk on the packed R, two workgroups per CU)
  walk1  the same, one workgroup per CU
  lag    sglm_lag_xtr             (the f32-row occurrence kernel; only when named)
and the max |difference| of walk and bits.  The walk's LDS-read floor is its occurrence x lag x
fit reads of 4 bytes at 128 B/clk on 256 CUs at 2.4 GHz.

usage: lag_bench.py [fits,fits,...] [kernel,kernel,...]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sabatinilab-glm_amd")]

LDS_BYTES_PER_S = 256 * 128 * 2.4e9


def main():
    import torch
    from sglm_hip import _lib, engine as E, synth
    s = synth.make(N=1_000_000, m=50, L=20, family="poisson", rho=0.02, seed=0)
    d = E.Design.from_events(s.E, s.shifts, s.L - 1, s.N)
    lg = d.lag
    st = torch.cuda.current_stream().cuda_stream
    sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else \
        [6, 30, 47, 65, 78, 120]
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else ["bits", "walk", "walk1"]
    nocc = int(lg.occ.numel())
    for B in sizes:
        rng = np.random.default_rng(B)
        R = torch.zeros((B, d.ld), dtype=torch.float32, device="cuda")
        R[:, :d.n] = torch.from_numpy(rng.normal(size=(B, d.n)).astype(np.float32)).cuda()
        slots = torch.arange(B, dtype=torch.int32, device="cuda")
        g = {k: torch.zeros((B, d.P), dtype=torch.float64, device="cuda") for k in names}
        w1 = torch.empty(_lib.query("sglm_lag_xtr_work_bytes", d.P, lg.K, B, d.n),
                         dtype=torch.uint8, device="cuda")
        # the packed operand: R as three bf16 pieces, [3][ceil(B/32)*32][ld]
        Bp = (B + 31) // 32 * 32
        hi = R.to(torch.bfloat16)
        mid = (R - hi.float()).to(torch.bfloat16)
        lo = (R - hi.float() - mid.float()).to(torch.bfloat16)
        rp = torch.zeros((3, Bp, d.ld), dtype=torch.bfloat16, device="cuda")
        rp[0, :B], rp[1, :B], rp[2, :B] = hi, mid, lo
        w2 = torch.empty(_lib.query("sglm_xtr_bits_packed_work_bytes", d.P, B, d.ld),
                         dtype=torch.uint8, device="cuda")
        w3 = torch.empty(E.lag_xtr_plan(d.n, B, lg.K, d.P)["work_bytes"], dtype=torch.uint8,
                         device="cuda")

        def lag():
            _lib.call("sglm_lag_xtr", lg.occ.data_ptr(), lg.tbeg.data_ptr(), lg.tend.data_ptr(),
                      lg.shifts.data_ptr(), lg.m, lg.K, lg.layout, lg.row0, d.n, d.P,
                      R.data_ptr(), d.ld, slots.data_ptr(), B, g["lag"].data_ptr(),
                      w1.data_ptr(), st)

        def bits():
            _lib.call("sglm_xtr_bits_packed_bp", d.cbits_full().data_ptr(), d.ld, d.P, d.n,
                      rp.data_ptr(), B, Bp, slots.data_ptr(), g["bits"].data_ptr(),
                      w2.data_ptr(), st)

        def walk(name="walk", per_cu=2):
            _lib.call("sglm_lag_xtr_packed_bp", lg.occ.data_ptr(), nocc, lg.px[0].data_ptr(),
                      lg.px[1].data_ptr(), lg.m, lg.K, lg.smin, lg.smax, lg.layout, lg.row0,
                      d.n, d.ld, d.P, rp.data_ptr(), B, Bp, slots.data_ptr(),
                      g[name].data_ptr(), w3.data_ptr(), per_cu, st)
        fns = {"lag": lag, "bits": bits, "walk": walk, "walk1": lambda: walk("walk1", 1)}
        out = {"fits": B}
        for name in names:
            fn = fns[name]
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name + "_ms"] = round(e0.elapsed_time(e1) / 10, 4)
        floor_ms = 1e3 * nocc * lg.K * 4.0 * B / LDS_BYTES_PER_S
        out["lds_floor_ms"] = round(floor_ms, 4)
        for name in ("walk", "walk1"):
            if name in names:
                out[name + "_over_floor"] = round(out[name + "_ms"] / floor_ms, 2)
        if "walk" in names and "bits" in names:
            out["rel_diff"] = float((g["walk"] - g["bits"]).abs().max() / g["bits"].abs().max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
