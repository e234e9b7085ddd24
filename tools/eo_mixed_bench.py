#!/usr/bin/env python3
"""Mixed-precision even-odd CG against the fp64 even-odd solve, whole solves to 1e-10.

    python tools/eo_mixed_bench.py [--sizes 1024,4096] [--pairs 3] [--hmc 1024] [--out FILE]

Per size (sigma 0.2374, m0 -0.06: configs 2 and 3 of BASELINE.md): one context,
the fp64 and the mixed solve through sm_eo_cg_dev alternating in pairs (after
one warm-up solve of each, which also allocates the fp32 buffers). Per size:
wall time, iterations and us per iteration of each mode, the reliable updates,
the fp64 solve's run-to-run spread (max - min over its repeats, as a fraction
of the median) and the ratio of the medians. --hmc N adds one even-odd HMC
trajectory at N^2 (beta 2, m0 0.1, 10 steps, tau 0.5; the second of two from
one start) in each mode. The records go to stdout as JSON lines and, together,
to profiles/eo_cg_mixed_<build id>.json (or --out).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--m0", type=float, default=-0.06)
    ap.add_argument("--sigma", type=float, default=0.2374)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=100000, help="cut the solves short (profiler runs)")
    ap.add_argument("--modes", default="double,mixed", help="profiler runs: one mode only")
    ap.add_argument("--hmc", type=int, default=0, help="also time one even-odd HMC trajectory at this size")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import schwingermodel_amd as sm
    vp = ctypes.c_void_p
    modes = a.modes.split(",")
    build_id = sm.lib.sm_build_id().decode()
    records = []
    for N in (int(s) for s in a.sizes.split(",") if s):
        L = sm.Lattice(N, N)
        V = L.V
        s = torch.cuda.Stream()
        torch.cuda.set_stream(s)
        sm.check(sm.lib.sm_set_stream(L.ctx, vp(s.cuda_stream)))
        U = torch.empty(4 * V, dtype=torch.float64)
        p = torch.empty(4 * V, dtype=torch.float64)
        Un, pn = U.numpy(), p.numpy()
        sm.lib.sm_fill_gauge(4321, a.sigma, N, 0, N, 0, N, Un.ctypes.data, Un[2 * V:].ctypes.data)
        sm.lib.sm_fill_spinor(91011, N, 0, N, 0, N, pn.ctypes.data, pn[2 * V:].ctypes.data)
        dU, dp = U.cuda(), p.cuda()
        x = torch.empty_like(dp)
        sm.check(sm.lib.sm_upload_gauge_dev(L.ctx, vp(dU.data_ptr())))
        res = sm.CGResult()

        def solve(mode):
            L.eo_cg_precision(mode)
            torch.cuda.synchronize()
            t = time.perf_counter()
            sm.check(sm.lib.sm_eo_cg_dev(L.ctx, vp(dp.data_ptr()), vp(x.data_ptr()), a.m0, a.tol, a.max_iter,
                                         ctypes.byref(res)))
            torch.cuda.synchronize()
            return time.perf_counter() - t, res.iterations, res.converged, res.residual / res.phi_norm

        out = {m: [] for m in modes}
        for mode in out:
            solve(mode)  # warm-up
        info = None
        for _ in range(a.pairs):
            for mode in out:
                out[mode].append(solve(mode))
                if mode == "mixed":
                    info = L.last_eo_cg_mixed
        rec = {"N": N, "build_id": build_id, "tol": a.tol, "pairs": a.pairs}
        for mode, runs in out.items():
            walls = [r[0] for r in runs]
            med = statistics.median(walls)
            rec[mode] = {"solve_ms": [round(w * 1e3, 3) for w in walls], "median_ms": round(med * 1e3, 3),
                         "iterations": runs[-1][1], "converged": runs[-1][2], "relres": runs[-1][3],
                         "us_per_iteration": round(med * 1e6 / max(runs[-1][1], 1), 2),
                         "spread": round((max(walls) - min(walls)) / med, 4)}
        if info is not None:
            rec["mixed"].update(reliable_updates=info.reliable_updates, inner_iterations=info.inner_iterations,
                                fp64_iterations=info.fp64_iterations, fell_back=info.fell_back)
        if "double" in rec and "mixed" in rec:
            rec["time_ratio_double_over_mixed"] = round(rec["double"]["median_ms"] / rec["mixed"]["median_ms"], 4)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        L.close()
    if a.hmc:
        N = a.hmc
        rec = {"hmc_N": N, "build_id": build_id, "beta": 2.0, "m0": 0.1, "steps": 10, "tau": 0.5}
        for mode in modes:
            L = sm.Lattice(N, N)
            sm.check(sm.lib.sm_fill_gauge_dev(L.ctx, 77, 0.2374))
            L.eo_cg_precision(mode)
            prm = sm.HMCParams(0.1, 2.0, 0.5, 10, a.tol, 10000, 2024, 1)
            r = sm.HMCResult()
            walls = []
            for traj in range(2):
                t = time.perf_counter()
                sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(prm), traj, ctypes.byref(r)))
                walls.append(time.perf_counter() - t)
            rec[mode] = {"trajectory_s": round(walls[-1], 5), "first_trajectory_s": round(walls[0], 5), "dH": r.dH,
                         "cg_iterations": r.cg_iterations, "cg_failures": r.cg_failures}
            L.close()
        print(json.dumps(rec), flush=True)
        records.append(rec)
    path = a.out or os.path.join(REPO, "profiles", f"eo_cg_mixed_{build_id}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"build_id": build_id, "records": records}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
