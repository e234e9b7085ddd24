#!/usr/bin/env python3
"""Pion correlators of a whole replica ensemble in one call against what a
caller had before it.

    python tools/ens_pion_bench.py --out profiles/ens_pion_<build id>.json

For every lattice N x N, ensemble size R and source count nsrc, on beta = 2
fields thermalised by the ensemble itself (even-odd action, m0 = 0; --therm
trajectories of tau 0.3 from Gaussian link angles of sigma 0.42, whose plaquette
exp(-2 sigma^2) is the pure-gauge value 0.70 at beta = 2, with 10 MD steps up to
64^2, 16 at 128^2 and 24 at 256^2; the acceptance and the final plaquette are
recorded; at most --fields distinct fields, replica r holds field r mod that),
m0 = 0, tol 1e-10:
  ensemble    sm_ens_pion_correlator, solver 0 (D D^dag) and solver 1 (even-odd);
  loop        per replica: sm_ens_download_gauge, sm_upload_gauge into the lone
              context, sm_pion_correlator (default settings) with the same sources.
After one warm-up call of each, --pairs interleaved rounds (solver 0, solver 1,
loop) are timed with the host clock around the synchronous calls. A row reports
the three medians, the loop's spread (max - min over its rounds, relative to
its median), both speed-ups, and credits a solver only where its median beats
the loop's by more than that spread. --seq-cap C (0: off) runs the loop over
the first C replicas only when R > C and scales its time by R / C; such rows
say so ("loop_replicas_run"). The mean iteration counts per column of both
solvers and their ratio are recorded too.
"""
import argparse
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


def md_steps(N):
    """dH grows with the square root of the volume at a fixed step: shorter steps on the larger lattices."""
    return 10 if N <= 64 else 16 if N <= 128 else 24


def sources(N, nsrc):
    base = [(0, 0), (N // 2, N // 3), (N - 1, N - 1), (1, 0)]
    return [base[i % 4] if i < 4 else ((7 * i) % N, (11 * i) % N) for i in range(nsrc)]


def thermalised(sm, N, nfields, ntherm):
    """nfields beta = 2 configurations as (2, V) complex128 host arrays."""
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


def measure(sm, N, R, nsrc, fields, pairs, seq_cap):
    L = sm.Lattice(N, N)
    E = L.ensemble(R)
    for r in range(R):
        E.upload_gauge(r, fields[r % len(fields)])
    src = sources(N, nsrc)
    m0s = [M0] * R
    nloop = R if not seq_cap or R <= seq_cap else seq_cap

    def ens(solver):
        t0 = time.perf_counter()
        _, res = E.pion_correlator(m0s, src, solver=solver, tol=TOL, max_iter=MAXIT)
        dt = time.perf_counter() - t0
        its = [x.iterations for rr in res for x in rr]
        return dt, its, all(x.converged for rr in res for x in rr)

    def loop():
        t0 = time.perf_counter()
        its, ok = [], True
        for r in range(nloop):
            U = E.download_gauge(r)
            sm.check(sm.lib.sm_upload_gauge(L.ctx, U[0].ctypes.data, U[1].ctypes.data))
            _, res = L.pion_correlator(M0, src, tol=TOL, max_iter=MAXIT)
            its += [x.iterations for x in res]
            ok = ok and all(x.converged for x in res)
        return (time.perf_counter() - t0) * R / nloop, its, ok

    ens("plain"), ens("even_odd"), loop()
    t = {"plain": [], "even_odd": [], "loop": []}
    its, ok = {}, True
    for _ in range(pairs):
        for key, fn in (("plain", lambda: ens("plain")), ("even_odd", lambda: ens("even_odd")), ("loop", loop)):
            dt, it, good = fn()
            t[key].append(dt)
            its[key] = float(np.mean(it))
            ok = ok and good
    E.close()
    L.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["loop"]) - min(t["loop"])) / med["loop"]
    return {
        "N": N, "R": R, "nsrc": nsrc, "pairs": pairs, "loop_replicas_run": nloop, "all_converged": bool(ok),
        "plain_s": t["plain"], "even_odd_s": t["even_odd"], "loop_s": t["loop"],
        "plain_median_s": med["plain"], "even_odd_median_s": med["even_odd"], "loop_median_s": med["loop"],
        "loop_spread": spread,
        "speedup_plain": med["loop"] / med["plain"], "speedup_even_odd": med["loop"] / med["even_odd"],
        "credited_plain": bool(med["plain"] < med["loop"] * (1.0 - spread)),
        "credited_even_odd": bool(med["even_odd"] < med["loop"] * (1.0 - spread)),
        "iterations_per_column": its, "iteration_ratio_even_odd_to_plain": its["even_odd"] / its["plain"],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lattices", default="32,64,128,256")
    ap.add_argument("--R", default="1,4,16,64")
    ap.add_argument("--nsrc", default="1,4")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--therm", type=int, default=20)
    ap.add_argument("--fields", type=int, default=16)
    ap.add_argument("--seq-cap", type=int, default=16)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import schwingermodel_amd as sm

    Rs = [int(x) for x in a.R.split(",") if x]
    result = {"build_id": sm.lib.sm_build_id().decode(),
              "params": {"beta": BETA, "m0": M0, "tol": TOL, "therm_tau": TAU, "therm_start_sigma": START_SIGMA,
                         "therm_trajectories": a.therm, "distinct_fields": a.fields, "seq_cap": a.seq_cap},
              "thermalisation": [], "rows": []}

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)

    for N in [int(x) for x in a.lattices.split(",") if x]:
        fields, acc, plaq = thermalised(sm, N, min(max(Rs), a.fields), a.therm)
        result["thermalisation"].append({"N": N, "fields": len(fields), "md_steps": md_steps(N), "acceptance": acc,
                                         "plaquette": plaq})
        print(json.dumps(result["thermalisation"][-1]), flush=True)
        for R in Rs:
            for nsrc in [int(x) for x in a.nsrc.split(",") if x]:
                row = measure(sm, N, R, nsrc, fields, a.pairs, a.seq_cap)
                result["rows"].append(row)
                print(json.dumps({k: row[k] for k in ("N", "R", "nsrc", "plain_median_s", "even_odd_median_s",
                                                      "loop_median_s", "loop_spread", "speedup_plain",
                                                      "speedup_even_odd", "credited_plain", "credited_even_odd",
                                                      "iteration_ratio_even_odd_to_plain", "loop_replicas_run",
                                                      "all_converged")}), flush=True)
                dump()


if __name__ == "__main__":
    main()
