#!/usr/bin/env python3
"""Wilson flow of a whole replica ensemble in one call against what a caller
has without the ensemble form.

    python tools/ens_flow_bench.py --out profiles/ens_flow_<build id>.json

For every lattice N x N and ensemble size R, on fields of Gaussian link angles
(sigma 0.42, drawn on the device; the flow's cost does not depend on the field),
--steps steps of eps 0.02 measured every --every steps:
  ensemble    sm_ens_wilson_flow: one launch per stage for all R replicas;
  loop        per replica: sm_ens_download_gauge, sm_upload_gauge into the lone
              context, sm_wilson_flow.
After one warm-up call of each, --pairs interleaved rounds (ensemble, loop) are
timed with the host clock around the synchronous calls. A row reports both
medians, the loop's spread (max - min over its rounds, relative to its median),
the speed-up, and credits the ensemble form only where its median beats the
loop's by more than that spread. Every row also checks that replica 0's series
is bitwise the lone context's.
Each row also times the ensemble's flow with two measured points only and
reports it per stage launch ("stage_us": host clock over the synchronous call
divided by 3 steps launches, the two measurements and the copy included) next
to the stage kernel's traffic, 256 B per site, replica and step (sm_flow.hip).
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

EPS, SIGMA = 0.02, 0.42
STEP_BYTES = 256   # per site and replica: stages of 80 + 96 + 80 B (sm_flow.hip)


def measure(sm, N, R, steps, every, pairs):
    L = sm.Lattice(N, N)
    E = L.ensemble(R)
    for r in range(R):
        E.fill_gauge(r, 900 + r, SIGMA)

    def ens(me=every):
        t0 = time.perf_counter()
        s = E.wilson_flow(EPS, steps, me)
        return time.perf_counter() - t0, s

    def loop():
        t0 = time.perf_counter()
        first = None
        for r in range(R):
            U = E.download_gauge(r)
            sm.check(sm.lib.sm_upload_gauge(L.ctx, U[0].ctypes.data, U[1].ctypes.data))
            s = L.wilson_flow(EPS, steps, every)
            first = s if first is None else first
        return time.perf_counter() - t0, first

    ens(), loop(), ens(steps)
    t = {"ens": [], "loop": [], "stage": []}
    same = True
    for _ in range(pairs):
        dt, se = ens()
        t["ens"].append(dt)
        dt, sl = loop()
        t["loop"].append(dt)
        t["stage"].append(ens(steps)[0])
        same = same and all(np.array_equal(a[0].view(np.uint64), b.view(np.uint64)) for a, b in zip(se[1:], sl[1:]))
    q = E.topology().q_geo
    E.close()
    L.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["loop"]) - min(t["loop"])) / med["loop"]
    stage_us = med["stage"] / (3 * steps) * 1e6
    return {
        "N": N, "R": R, "steps": steps, "meas_every": every, "pairs": pairs, "replica0_bitwise_lone": bool(same),
        "ens_s": t["ens"], "loop_s": t["loop"], "ens_median_s": med["ens"], "loop_median_s": med["loop"],
        "loop_spread": spread, "speedup": med["loop"] / med["ens"],
        "credited": bool(med["ens"] < med["loop"] * (1.0 - spread)),
        "stage_us": stage_us, "stage_bytes_per_site_step": STEP_BYTES,
        "stage_GBps": STEP_BYTES / 3.0 * N * N * R / (stage_us * 1e-6) / 1e9,
        "q_geo_unflowed_mean_abs": float(np.mean(np.abs(q))),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lattices", default="32,64,128,256")
    ap.add_argument("--R", default="1,4,16,64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import schwingermodel_amd as sm

    result = {"build_id": sm.lib.sm_build_id().decode(),
              "params": {"eps": EPS, "steps": a.steps, "meas_every": a.every, "field_sigma": SIGMA}, "rows": []}
    for N in [int(x) for x in a.lattices.split(",") if x]:
        for R in [int(x) for x in a.R.split(",") if x]:
            row = measure(sm, N, R, a.steps, a.every, a.pairs)
            result["rows"].append(row)
            print(json.dumps({k: row[k] for k in ("N", "R", "ens_median_s", "loop_median_s", "loop_spread", "speedup",
                                                  "credited", "stage_us", "stage_GBps", "replica0_bitwise_lone")}),
                  flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
