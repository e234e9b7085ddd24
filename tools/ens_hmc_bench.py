#!/usr/bin/env python3
"""HMC throughput of a replica ensemble against the same chains run one after
another ("replica ensemble").

    python tools/ens_hmc_bench.py --out profiles/hmc_ensemble_<build id>.json

For every lattice N x N and ensemble size R: R chains with the recorded
reference chain's parameters (beta 2, m0 0, tau 0.3, md_steps 10; seeds 1..R)
start from the same R hot fields on both sides,
  ensemble    one sm_ens of R replicas, sm_ens_hmc_trajectory;
  sequential  one lone context, chain after chain through sm_hmc_trajectory
              (the field of the chain being timed is uploaded before and
              downloaded after its window, outside the clock).
After --warmup trajectories, --pairs interleaved pairs of windows of --traj
trajectories are timed with the host clock around the synchronous calls. A row
reports both medians and the sequential side's spread (max - min over its
windows, relative to the median); the ensemble is credited only where it beats
the sequential median by more than that spread. --seq-cap C (0: off) runs only
the first C chains of the sequential side when R > C and scales their time by
R / C; such rows say so ("seq_chains_run").

--even-odd times the even-odd ensemble (even_odd = 1 for every replica)
instead, against two baselines on identical parameters, seeds and start fields:
the plain-action ensemble (the path without this option), and -- with
--eo-seq -- the same chains one after another through
sm_hmc_trajectory(even_odd = 1) (--seq-cap applies). Pairs are interleaved and
medians reported as above; a row gives the time against the plain ensemble, CG
iterations per trajectory and replica for both, and "pays" only where the
even-odd median beats the plain one by more than the plain side's spread.
Output: profiles/hmc_ensemble_eo_<build id>.json.

--stats N,R runs the reference protocol (Ntherm 50, Nmeas 100, Nsteps 1) on an
ensemble and reports the mean of the replicas' Ep with its error from their
scatter next to the manifest's pooled reference value, and the pull.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BETA, M0, TAU, MD_STEPS, TOL, MAXIT = 2.0, 0.0, 0.3, 10, 1e-10, 10000


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def params(sm, R, even_odd=0):
    return [sm.HMCParams(M0, BETA, TAU, MD_STEPS, TOL, MAXIT, 1 + r, even_odd) for r in range(R)]


def hot_fields(sm, N, R):
    out = []
    for r in range(R):
        U = np.empty((2, N * N), dtype=np.complex128)
        sm.lib.sm_fill_gauge(900 + r, -1.0, N, 0, N, 0, N, vp(U[0]), vp(U[1]))
        out.append(U)
    return out


def lone_window(sm, L, p, U, first, n):
    """n trajectories of one chain on the lone context; returns (seconds, iterations)."""
    sm.check(sm.lib.sm_upload_gauge(L.ctx, vp(U[0]), vp(U[1])))
    res = sm.HMCResult()
    its = 0
    t0 = time.perf_counter()
    for t in range(first, first + n):
        sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(p), t, ctypes.byref(res)))
        its += res.cg_iterations
    dt = time.perf_counter() - t0
    sm.check(sm.lib.sm_download_gauge(L.ctx, vp(U[0]), vp(U[1])))
    return dt, its


def ens_window(E, p, first, n):
    its = 0
    t0 = time.perf_counter()
    for t in range(first, first + n):
        its += sum(o.cg_iterations for o in E.trajectory(p, t))
    return time.perf_counter() - t0, its


def measure(sm, N, R, ntraj, warmup, pairs, seq_cap):
    L = sm.Lattice(N, N)
    p = params(sm, R)
    fields = hot_fields(sm, N, R)
    E = L.ensemble(R)
    for r in range(R):
        E.upload_gauge(r, fields[r])
    nseq = R if not seq_cap or R <= seq_cap else seq_cap
    ens_window(E, p, 0, warmup)
    for r in range(nseq):
        lone_window(sm, L, p[r], fields[r], 0, warmup)
    ens_s, seq_s, ens_it, seq_it = [], [], 0, 0
    for i in range(pairs):
        first = warmup + i * ntraj
        dt, it = ens_window(E, p, first, ntraj)
        ens_s.append(dt)
        ens_it += it
        tot = 0.0
        for r in range(nseq):
            dt, it = lone_window(sm, L, p[r], fields[r], first, ntraj)
            tot += dt
            seq_it += it
        seq_s.append(tot * R / nseq)
    E.close()
    L.close()
    em, sq = statistics.median(ens_s), statistics.median(seq_s)
    spread = (max(seq_s) - min(seq_s)) / sq
    return {
        "N": N, "R": R, "trajectories": ntraj, "pairs": pairs, "seq_chains_run": nseq,
        "ens_s": ens_s, "seq_s": seq_s, "ens_median_s": em, "seq_median_s": sq, "seq_spread": spread,
        "speedup": sq / em, "credited": bool(em < sq * (1.0 - spread)),
        "ens_ms_per_traj_replica": 1e3 * em / (ntraj * R), "seq_ms_per_traj_chain": 1e3 * sq / (ntraj * R),
        "cg_iterations_per_traj_replica": {"ens": ens_it / (pairs * ntraj * R), "seq": seq_it / (pairs * ntraj * nseq)},
    }


def measure_eo(sm, N, R, ntraj, warmup, pairs, seq_cap, with_seq):
    """The even-odd ensemble against the plain-action ensemble (and, with_seq,
    lone even-odd chains one after another) from the same hot fields."""
    L = sm.Lattice(N, N)
    pe, pp = params(sm, R, 1), params(sm, R, 0)
    fields = hot_fields(sm, N, R)
    Ee, Ep = L.ensemble(R), L.ensemble(R)
    for r in range(R):
        Ee.upload_gauge(r, fields[r])
        Ep.upload_gauge(r, fields[r])
    nseq = 0 if not with_seq else (R if not seq_cap or R <= seq_cap else seq_cap)
    ens_window(Ee, pe, 0, warmup)
    ens_window(Ep, pp, 0, warmup)
    for r in range(nseq):
        lone_window(sm, L, pe[r], fields[r], 0, warmup)
    eo_s, pl_s, seq_s, eo_it, pl_it, seq_it = [], [], [], 0, 0, 0
    for i in range(pairs):
        first = warmup + i * ntraj
        dt, it = ens_window(Ee, pe, first, ntraj)
        eo_s.append(dt)
        eo_it += it
        dt, it = ens_window(Ep, pp, first, ntraj)
        pl_s.append(dt)
        pl_it += it
        tot = 0.0
        for r in range(nseq):
            dt, it = lone_window(sm, L, pe[r], fields[r], first, ntraj)
            tot += dt
            seq_it += it
        if nseq:
            seq_s.append(tot * R / nseq)
    Ee.close()
    Ep.close()
    L.close()
    em, pm = statistics.median(eo_s), statistics.median(pl_s)
    spread = (max(pl_s) - min(pl_s)) / pm
    n = pairs * ntraj * R
    row = {
        "N": N, "R": R, "trajectories": ntraj, "pairs": pairs, "eo_s": eo_s, "plain_s": pl_s,
        "eo_median_s": em, "plain_median_s": pm, "plain_spread": spread, "speedup_vs_plain": pm / em,
        "pays": bool(em < pm * (1.0 - spread)),
        "eo_ms_per_traj_replica": 1e3 * em / (ntraj * R), "plain_ms_per_traj_replica": 1e3 * pm / (ntraj * R),
        "cg_iterations_per_traj_replica": {"eo": eo_it / n, "plain": pl_it / n},
        "seq_chains_run": nseq,
    }
    if nseq:
        sq = statistics.median(seq_s)
        row.update({"seq_eo_s": seq_s, "seq_eo_median_s": sq, "speedup_vs_seq_eo": sq / em})
        row["cg_iterations_per_traj_replica"]["seq_eo"] = seq_it / (pairs * ntraj * nseq)
    return row


def stats_run(sm, N, R):
    with open(os.path.join(REPO, "tests", "golden", "manifest.json")) as f:
        m = json.load(f)
    ref = dict(m["hmc_stat"])
    ch = m["hmc_stat_chains"]["chains"]
    ref.update(m["hmc_stat_chains"]["pooled"])
    mean = sum(c["Ep"] for c in ch) / len(ch)
    ref_err = math.sqrt(sum((c["Ep"] - mean) ** 2 for c in ch) / (len(ch) - 1)) / math.sqrt(len(ch))
    L = sm.Lattice(N, N)
    E = L.ensemble(R)
    p = [sm.HMCParams(ref["m0"], ref["beta"], ref["tau"], ref["md_steps"], TOL, MAXIT, 20261100 + r, 0) for r in range(R)]
    t0 = time.perf_counter()
    out, _, _ = E.run(p, ref["Ntherm"], ref["Nmeas"], ref["Nsteps"], hot_start=True)
    dt = time.perf_counter() - t0
    E.close()
    L.close()
    eps = [o.Ep for o in out]
    em = sum(eps) / R
    err = math.sqrt(sum((e - em) ** 2 for e in eps) / (R - 1)) / math.sqrt(R)
    return {
        "N": N, "R": R, "Ntherm": ref["Ntherm"], "Nmeas": ref["Nmeas"], "Nsteps": ref["Nsteps"], "seconds": dt,
        "Ep_replicas": eps, "dEp_replicas": [o.dEp for o in out], "acceptance": [o.acceptance for o in out],
        "cg_failures": sum(o.cg_failures for o in out),
        "Ep_mean": em, "Ep_err_from_scatter": err, "ref_Ep": ref["Ep"], "ref_dEp_from_chain_scatter": ref_err,
        "ref_chains": len(ch), "pull_sigma": (em - ref["Ep"]) / math.hypot(err, ref_err),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lattices", default="32,64,128,256")
    ap.add_argument("--R", default="1,2,4,8,16,32,64")
    ap.add_argument("--traj", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--seq-cap", type=int, default=0)
    ap.add_argument("--even-odd", action="store_true")
    ap.add_argument("--eo-seq", action="store_true")
    ap.add_argument("--stats", default=None, metavar="N,R")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import schwingermodel_amd as sm

    result = {"build_id": sm.lib.sm_build_id().decode(), "params": {"beta": BETA, "m0": M0, "tau": TAU,
                                                                     "md_steps": MD_STEPS, "cg_tol": TOL},
              "rows": [], "stats": None}

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)

    for N in [int(x) for x in a.lattices.split(",") if x]:
        for R in [int(x) for x in a.R.split(",") if x]:
            if a.even_odd:
                row = measure_eo(sm, N, R, a.traj, a.warmup, a.pairs, a.seq_cap, a.eo_seq)
                result["rows"].append(row)
                print(json.dumps({k: row.get(k) for k in ("N", "R", "eo_median_s", "plain_median_s", "plain_spread",
                                                          "speedup_vs_plain", "pays", "speedup_vs_seq_eo",
                                                          "cg_iterations_per_traj_replica")}), flush=True)
                dump()
                continue
            row = measure(sm, N, R, a.traj, a.warmup, a.pairs, a.seq_cap)
            result["rows"].append(row)
            print(json.dumps({k: row[k] for k in ("N", "R", "ens_median_s", "seq_median_s", "seq_spread", "speedup",
                                                  "credited", "seq_chains_run")}), flush=True)
            dump()
    if a.stats:
        N, R = (int(x) for x in a.stats.split(","))
        result["stats"] = stats_run(sm, N, R)
        print(json.dumps(result["stats"]), flush=True)
        dump()


if __name__ == "__main__":
    main()
