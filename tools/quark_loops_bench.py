#!/usr/bin/env python3
"""Stochastic quark loops in one call against what a caller had before them, and
the fused contraction kernel's own time.

    python tools/quark_loops_bench.py --out profiles/quark_loops_<build id>.json
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- \\
        python tools/quark_loops_bench.py --kernel-run <dir>/plan.json
    python tools/quark_loops_bench.py --merge-trace <dir> --out profiles/quark_loops_<build id>.json

Whole calls. For every lattice N x N and ensemble size R, nnoise vectors per
replica on beta = 2 fields thermalised by the ensemble itself (as
tools/ens_pion_bench.py: even-odd action, m0 = 0, at most --fields distinct
fields), m0 = 0, tol 1e-10:
  ensemble    sm_ens_quark_loops, solver 0 (D D^dag) and solver 1 (even-odd);
  lone        R = 1 only: sm_quark_loops on a lone context, both solvers (all
              nnoise vectors in one batched solve);
  before      per replica: sm_ens_download_gauge, sm_upload_gauge into the lone
              context, the nnoise noise vectors on the host (sm_fill_noise), one
              sm_cg_batch of nnoise columns, D^dag of every solution through the
              public apply (sm_dirac, dagger = 1), and the slice sums in numpy.
After one warm-up call of each, --pairs interleaved rounds are timed with the
host clock around the synchronous calls. A row reports the medians, the
baseline's spread (max - min over its rounds, relative to its median), the
speed-ups, and credits a path only where its median beats the baseline's by
more than that spread. --seq-cap C (0: off) runs the baseline over the first C
replicas only when R > C and scales its time by R / C ("before_replicas_run").
The baseline's loops are compared with the ensemble's (they differ by the
solvers' rounding only): "max_rel_dev_vs_before".

The kernel. --kernel-run makes, under a kernel trace, --reps calls per (N, K):
sm_quark_loops with nnoise = K on a lone context (one contraction launch of K
columns on one shared field, solver 0 = the fused form, solver 1 = the load-psi
form) and, for K = 64, sm_ens_quark_loops with R = 64 (64 fields, one launch per
vector), and writes the order of the contraction launches to the plan file.
--merge-trace matches the trace's loops_contract_kernel dispatches to that plan
in time order and adds "kernel_rows" to --out: the median duration per (N, K,
form, links) and the rate against the algorithmic 32 B per site and column (y
or psi; the links, 32 B per site of a field, are not counted).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BETA, M0, TAU, TOL, MAXIT = 2.0, 0.0, 0.3, 1e-10, 10000
START_SIGMA = 0.42
SEED0 = 1000


def md_steps(N):
    return 10 if N <= 64 else 16 if N <= 128 else 24


def thermalised(sm, N, nfields, ntherm):
    """nfields beta = 2 configurations as (2, V) complex128 host arrays (tools/ens_pion_bench.py's)."""
    L = sm.Lattice(N, N)
    E = L.ensemble(nfields)
    p = [sm.HMCParams(M0, BETA, TAU, md_steps(N), TOL, MAXIT, 1 + r, 1) for r in range(nfields)]
    for r in range(nfields):
        E.fill_gauge(r, 900 + r, START_SIGMA)
    acc = 0
    for t in range(ntherm):
        acc += sum(o.accepted for o in E.trajectory(p, t))
    sp, _ = E.plaquette([BETA] * nfields)
    fields = [E.download_gauge(r) for r in range(nfields)]
    E.close()
    L.close()
    return fields, acc / max(1, ntherm * nfields), float(np.mean(sp)) / (N * N)


def before(sm, L, N, U, nnoise, seed):
    """One replica the way a caller did it before sm_quark_loops: (loops (nnoise, N, 2), iterations, converged)."""
    V = N * N
    sm.check(sm.lib.sm_upload_gauge(L.ctx, U[0].ctypes.data, U[1].ctypes.data))
    eta = np.empty((nnoise, 2, V), dtype=np.complex128)
    for k in range(nnoise):
        sm.lib.sm_fill_noise(seed, k, N, 0, N, 0, N, eta[k, 0].ctypes.data, eta[k, 1].ctypes.data)
    y, res = L.cg_batch(eta, M0, tol=TOL, max_iter=MAXIT)
    psi = np.empty_like(y)
    for k in range(nnoise):
        sm.check(sm.lib.sm_dirac(L.ctx, y[k, 0].ctypes.data, y[k, 1].ctypes.data, psi[k, 0].ctypes.data,
                                 psi[k, 1].ctypes.data, M0, 1))
    w = (np.conj(eta) * psi).reshape(nnoise, 2, N, N)
    loops = np.stack([(w[:, 0] + w[:, 1]).sum(axis=1), (w[:, 0] - w[:, 1]).sum(axis=1)], axis=2)
    return loops, [x.iterations for x in res], all(x.converged for x in res)


def measure(sm, N, R, nnoise, fields, pairs, seq_cap):
    L = sm.Lattice(N, N)
    E = L.ensemble(R)
    for r in range(R):
        E.upload_gauge(r, fields[r % len(fields)])
    m0s, seeds = [M0] * R, [SEED0 + r for r in range(R)]
    nloop = R if not seq_cap or R <= seq_cap else seq_cap
    keep = {}

    def ens(solver):
        t0 = time.perf_counter()
        loops, res = E.quark_loops(m0s, nnoise, seeds, solver=solver, tol=TOL, max_iter=MAXIT)
        dt = time.perf_counter() - t0
        keep[solver] = loops
        return dt, [x.iterations for rr in res for x in rr], all(x.converged for rr in res for x in rr)

    def lone(solver):
        sm.check(sm.lib.sm_upload_gauge(L.ctx, fields[0][0].ctypes.data, fields[0][1].ctypes.data))
        t0 = time.perf_counter()
        _, res = L.quark_loops(M0, nnoise, seeds[0], solver=solver, tol=TOL, max_iter=MAXIT)
        return time.perf_counter() - t0, [x.iterations for x in res], all(x.converged for x in res)

    def loop():
        t0 = time.perf_counter()
        its, ok, out = [], True, []
        for r in range(nloop):
            U = E.download_gauge(r)
            loops, it, good = before(sm, L, N, U, nnoise, seeds[r])
            out.append(loops)
            its += it
            ok = ok and good
        keep["before"] = np.stack(out)
        return (time.perf_counter() - t0) * R / nloop, its, ok

    paths = [("plain", lambda: ens("plain")), ("even_odd", lambda: ens("even_odd")), ("before", loop)]
    if R == 1:
        paths += [("lone_plain", lambda: lone("plain")), ("lone_even_odd", lambda: lone("even_odd"))]
    for _, fn in paths:
        fn()
    t = {k: [] for k, _ in paths}
    its, ok = {}, True
    for _ in range(pairs):
        for key, fn in paths:
            dt, it, good = fn()
            t[key].append(dt)
            its[key] = float(np.mean(it))
            ok = ok and good
    E.close()
    L.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["before"]) - min(t["before"])) / med["before"]
    scale = np.abs(keep["before"]).max()
    row = {"N": N, "R": R, "nnoise": nnoise, "pairs": pairs, "before_replicas_run": nloop, "all_converged": bool(ok),
           "seconds": t, "median_s": med, "before_spread": spread, "iterations_per_column": its,
           "max_rel_dev_vs_before": {s: float(np.abs(keep[s][:nloop] - keep["before"]).max() / scale)
                                     for s in ("plain", "even_odd")}}
    for k in med:
        if k != "before":
            row[f"speedup_{k}"] = med["before"] / med[k]
            row[f"credited_{k}"] = bool(med[k] < med["before"] * (1.0 - spread))
    return row


def kernel_run(sm, plan_path, lattices, Ks, reps):
    """The calls whose contraction launches --merge-trace times; the plan lists those launches in order."""
    plan = []
    for N in lattices:
        L = sm.Lattice(N, N)
        sm.check(sm.lib.sm_fill_gauge_dev(L.ctx, 4321, 0.42))
        for K in Ks:
            for solver, form in (("plain", "fused"), ("even_odd", "load_psi")):
                for rep in range(reps + 1):         # the first call of a shape is the warm-up
                    L.quark_loops(M0, K, SEED0, solver=solver, tol=TOL, max_iter=MAXIT)
                    plan.append({"N": N, "K": K, "form": form, "links": "shared", "warmup": rep == 0})
        if 64 in Ks:
            E = L.ensemble(64)
            for r in range(64):
                E.fill_gauge(r, 4321 + r, 0.42)
            for solver, form in (("plain", "fused"), ("even_odd", "load_psi")):
                E.quark_loops([M0] * 64, reps + 1, list(range(64)), solver=solver, tol=TOL, max_iter=MAXIT)
                plan += [{"N": N, "K": 64, "form": form, "links": "per column", "warmup": rep == 0}
                         for rep in range(reps + 1)]
            E.close()
        L.close()
    with open(plan_path, "w") as f:
        json.dump({"build_id": sm.lib.sm_build_id().decode(), "launches": plan}, f)


def merge_trace(trace_dir, out_path):
    with open(os.path.join(trace_dir, "plan.json")) as f:
        plan = json.load(f)
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if "loops_contract_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(plan["launches"]):
        raise SystemExit(f"{len(rows)} contraction dispatches in the trace, {len(plan['launches'])} planned")
    groups = {}
    for r, p in zip(rows, plan["launches"]):
        want = "1" if p["form"] == "load_psi" else "0"
        name = r["Kernel_Name"]
        if f"<{want}>" not in name and f"ILi{want}E" not in name:
            raise SystemExit(f"dispatch {name} does not match the planned form {p['form']}")
        if int(r["Grid_Size_Y"]) != p["K"]:
            raise SystemExit(f"dispatch of {r['Grid_Size_Y']} columns, {p['K']} planned")
        if not p["warmup"]:
            groups.setdefault((p["N"], p["K"], p["form"], p["links"]), []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    krows = []
    for (N, K, form, links), d in sorted(groups.items()):
        med = statistics.median(d)
        byt = 32.0 * N * N * K
        krows.append({"N": N, "K": K, "form": form, "links": links, "launches": len(d), "median_us": med * 1e6,
                      "min_us": min(d) * 1e6, "max_us": max(d) * 1e6, "algorithmic_bytes": byt,
                      "TB_per_s": byt / med * 1e-12})
        print(json.dumps(krows[-1]), flush=True)
    result = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            result = json.load(f)
    result["kernel_build_id"] = plan["build_id"]
    result["kernel_rows"] = krows
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lattices", default="32,64,128,256")
    ap.add_argument("--R", default="1,4,16,64")
    ap.add_argument("--nnoise", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--therm", type=int, default=20)
    ap.add_argument("--fields", type=int, default=16)
    ap.add_argument("--seq-cap", type=int, default=16)
    ap.add_argument("--kernel-run", metavar="PLAN", help="make the traced calls and write their launch plan")
    ap.add_argument("--kernel-K", default="16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--merge-trace", metavar="DIR", help="add the kernel rows of a trace directory to --out")
    ap.add_argument("--out")
    a = ap.parse_args()
    lattices = [int(x) for x in a.lattices.split(",") if x]
    if a.merge_trace:
        if not a.out:
            ap.error("--merge-trace needs --out")
        return merge_trace(a.merge_trace, a.out)
    import schwingermodel_amd as sm
    if a.kernel_run:
        return kernel_run(sm, a.kernel_run, lattices, [int(x) for x in a.kernel_K.split(",") if x], a.reps)
    if not a.out:
        ap.error("--out is required")
    Rs = [int(x) for x in a.R.split(",") if x]
    result = {"build_id": sm.lib.sm_build_id().decode(),
              "params": {"beta": BETA, "m0": M0, "tol": TOL, "nnoise": a.nnoise, "therm_tau": TAU,
                         "therm_start_sigma": START_SIGMA, "therm_trajectories": a.therm,
                         "distinct_fields": a.fields, "seq_cap": a.seq_cap},
              "thermalisation": [], "rows": []}

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)

    for N in lattices:
        fields, acc, plaq = thermalised(sm, N, min(max(Rs), a.fields), a.therm)
        result["thermalisation"].append({"N": N, "fields": len(fields), "md_steps": md_steps(N), "acceptance": acc,
                                         "plaquette": plaq})
        print(json.dumps(result["thermalisation"][-1]), flush=True)
        for R in Rs:
            row = measure(sm, N, R, a.nnoise, fields, a.pairs, a.seq_cap)
            result["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "seconds"}), flush=True)
            dump()


if __name__ == "__main__":
    main()
