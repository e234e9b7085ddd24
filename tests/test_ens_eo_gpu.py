"""The even-odd action in the replica ensemble (sm_ens.cpp on sm_eobatch.hip):
sm_ens_hmc_trajectory with even_odd = 1 for every replica.

Geometries are the batched even-odd kernel's edges (a wave owns 56 k-columns,
k = t / 2): 6x10 (one partial tile), 16x62 (half-width 31), 64x64 (redundant
scalars), 260x122 (a second k-tile of 5 columns; 2 x 130 = 260 partial slots).
The parameter cycle, the start-field rule and every tolerance are
test_ens_gpu.py's, for the reasons given there: anything downstream of a CG
solve is compared with the lone chain to the two fp64 solvers' rounding (they
sum in different orders), everything else bitwise.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, bits_equal, ptr
from test_ens_gpu import (MAXIT, TOL, bits, entry, host_gauge, lone_download, lone_plaquette, lone_upload,
                          rel, run_logs, start_sigma)
from test_ens_gpu import prm as plain_prm

pytestmark = pytest.mark.gpu

GEOMS = [(6, 10), (16, 62), (64, 64), (260, 122)]
IDS = [f"{a}x{b}" for a, b in GEOMS]
BIG_R = {(6, 10), (64, 64)}  # R = 64 only here
SM_ERR_ARG = 1


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


@pytest.fixture(scope="module")
def lattices(sm):
    made = {}

    def get(Nx, Nt):
        if (Nx, Nt) not in made:
            made[(Nx, Nt)] = sm.Lattice(Nx, Nt)
        return made[(Nx, Nt)]

    yield get
    for L in made.values():
        L.close()


def prm(sm, i, seed=None, tau=None, even_odd=1):
    p = plain_prm(sm, i, seed=seed, tau=tau)
    p.even_odd = even_odd
    return p


def members(sm, E, probe, probe_at, salt):
    params = []
    for r in range(E.R):
        if r in probe_at:
            params.append(probe[0])
            E.upload_gauge(r, probe[1])
        else:
            params.append(prm(sm, salt + r + 1))
            E.fill_gauge(r, 5000 + 97 * salt + r, start_sigma(params[-1]))
    return params


# ---- a. bitwise independence --------------------------------------------------------
@pytest.mark.parametrize("Nx,Nt", GEOMS, ids=IDS)
def test_replica_independence_bitwise(sm, lattices, Nx, Nt):
    L = lattices(Nx, Nt)
    probe = (prm(sm, 1, seed=11), host_gauge(sm, Nx, Nt, 4242, 0.1))
    E = L.ensemble(1)
    want = run_logs(E, members(sm, E, probe, {0}, 0))[0]
    E.close()
    assert any(e[4] for e in want)  # the probe's field does move
    for pos in range(5):
        E = L.ensemble(5)
        got = run_logs(E, members(sm, E, probe, {pos}, 10 * pos), watch=[pos])[pos]
        E.close()
        assert got == want, f"R = 5, position {pos}"
    if (Nx, Nt) in BIG_R:
        E = L.ensemble(64)
        logs = run_logs(E, members(sm, E, probe, {37, 63}, 3), watch=[37, 63])
        E.close()
        assert logs[37] == want, "R = 64, position 37"
        assert logs[63] == want, "R = 64, position 63"


# ---- b. against the lone even-odd chain ------------------------------------------------
@pytest.mark.parametrize("Nx,Nt", GEOMS, ids=IDS)
def test_against_the_lone_even_odd_chain(sm, lattices, Nx, Nt):
    L = lattices(Nx, Nt)
    R = 4
    params = [prm(sm, i) for i in range(R)]
    fields = [host_gauge(sm, Nx, Nt, 300 + r, start_sigma(params[r])) for r in range(R)]
    E = L.ensemble(R)
    in_band = fields_compared = 0
    for t in range(3):
        for r in range(R):
            E.upload_gauge(r, fields[r])
        outs = E.trajectory(params, t)
        for r in range(R):
            o, lo = outs[r], sm.HMCResult()
            lone_upload(sm, L, fields[r])
            sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(params[r]), t, ctypes.byref(lo)))
            Ul = lone_download(sm, L)
            print(f"EO {Nx}x{Nt} traj {t} replica {r}: H_old {o.H_old!r} / {lo.H_old!r} H_new {o.H_new!r} / "
                  f"{lo.H_new!r} r {o.r!r} dH {o.dH!r} / {lo.dH!r} it {o.cg_iterations} / {lo.cg_iterations}")
            assert bits(o.r) == bits(lo.r)
            assert abs(o.H_old - lo.H_old) <= 1e-10 * abs(lo.H_old)
            assert abs(o.H_new - lo.H_new) <= 1e-10 * abs(lo.H_new)
            assert abs(o.cg_iterations - lo.cg_iterations) <= max(1, lo.cg_iterations // 100)
            assert o.cg_failures == 0 and lo.cg_failures == 0
            if min(abs(o.r - math.exp(-o.dH)), abs(lo.r - math.exp(-lo.dH))) > 1e-5:
                assert o.accepted == lo.accepted
            else:
                in_band += 1
            if o.accepted and lo.accepted:
                assert rel(E.download_gauge(r), Ul) <= 1e-8
                fields_compared += 1
            fields[r] = Ul
    E.close()
    assert in_band <= 1
    assert fields_compared >= 3


# ---- c. reject and restore ---------------------------------------------------------------
@pytest.mark.parametrize("Nx,Nt", GEOMS, ids=IDS)
def test_bookkeeping_per_replica(sm, lattices, Nx, Nt):
    """Replicas 3 and 4 take steps of eps = 1 (tau = 6), beyond the leapfrog's
    stability bound, so that rejects occur among the accepts."""
    L = lattices(Nx, Nt)
    R = 5
    params = [prm(sm, i) for i in range(3)] + [prm(sm, 3, tau=6.0), prm(sm, 4, tau=6.0)]
    betas = [p.beta for p in params]
    starts = [host_gauge(sm, Nx, Nt, 700 + r, start_sigma(params[r])) for r in range(R)]
    seen = set()
    E = L.ensemble(R)
    for r in range(R):
        E.upload_gauge(r, starts[r])
    before = [u.copy() for u in starts]
    for t in range(3):
        outs = E.trajectory(params, t)
        after = [E.download_gauge(r) for r in range(R)]
        for r, o in enumerate(outs):
            assert o.accepted == (1 if o.r <= math.exp(-o.dH) else 0)
            assert bits(o.dH) == bits(o.H_new - o.H_old)
            seen.add(o.accepted)
            if not o.accepted:
                assert bits_equal(after[r].view(np.float64), before[r].view(np.float64))
            else:
                assert not bits_equal(after[r].view(np.float64), before[r].view(np.float64))
            sp, act = lone_plaquette(sm, L, after[r], betas[r])
            assert bits(o.sp) == bits(sp) and bits(o.gauge_action) == bits(act)
        before = after
    E.close()
    assert seen == {0, 1}


# ---- d. plain and even-odd trajectories on one ensemble -------------------------------------
def test_plain_after_even_odd_and_neighbours_undisturbed(sm, lattices):
    Nx, Nt, m0 = 16, 62, 0.1
    L = lattices(Nx, Nt)
    V = Nx * Nt
    U = host_gauge(sm, Nx, Nt, 91, 0.4)
    lone_upload(sm, L, U)
    phi = np.empty((2, V), dtype=np.complex128)
    sm.lib.sm_fill_spinor(40, Nt, 0, Nx, 0, Nt, ptr(phi[0]), ptr(phi[1]))
    xx, tt = np.meshgrid(np.arange(Nx), np.arange(Nt), indexing="ij")
    phie = phi * ((xx + tt) % 2 == 0).reshape(-1)

    def solves():
        out = []
        for f, src in ((sm.lib.sm_cg, phi), (sm.lib.sm_eo_cg, phie)):
            x = np.empty((2, V), dtype=np.complex128)
            res = sm.CGResult()
            sm.check(f(L.ctx, ptr(src[0]), ptr(src[1]), ptr(x[0]), ptr(x[1]), m0, TOL, MAXIT, ctypes.byref(res)))
            out.append((x.tobytes(), res.iterations))
        return out

    R = 3
    pl = [prm(sm, i, even_odd=0) for i in range(R)]
    eo = [prm(sm, i) for i in range(R)]
    starts = [host_gauge(sm, Nx, Nt, 60 + r, start_sigma(pl[r])) for r in range(R)]

    def plain_log(E):
        for r in range(R):
            E.upload_gauge(r, starts[r])
        outs = E.trajectory(pl, 5)
        return [entry(outs[r], E.download_gauge(r)) for r in range(R)]

    before = solves()
    E = L.ensemble(R)
    fresh = plain_log(E)
    E.close()
    E = L.ensemble(R)
    for r in range(R):
        E.upload_gauge(r, starts[r])
    outs = E.trajectory(eo, 0)
    assert all(o.cg_failures == 0 for o in outs)
    assert plain_log(E) == fresh          # plain after even-odd: a fresh ensemble's bits
    E.trajectory(eo, 1)                   # and back again
    assert plain_log(E) == fresh
    E.close()
    assert bits_equal(lone_download(sm, L).view(np.float64), U.view(np.float64))
    assert solves() == before


# ---- e. odd geometry, bad values ------------------------------------------------------------
def test_refusals(sm, lattices):
    lib = sm.lib
    L = lattices(16, 61)
    E = L.ensemble(2)
    res = (sm.HMCResult * 2)()
    for r in range(2):
        E.fill_gauge(r, 10 + r, 0.1)
    eo = (sm.HMCParams * 2)(prm(sm, 1), prm(sm, 3))
    assert lib.sm_ens_hmc_trajectory(E.ens, eo, 0, res) == SM_ERR_ARG
    assert b"even" in lib.sm_last_error()
    outs = E.trajectory([prm(sm, 1, even_odd=0), prm(sm, 3, even_odd=0)], 0)  # the plain action still runs
    assert all(o.cg_failures == 0 for o in outs)
    E.close()
    L = lattices(6, 10)
    E = L.ensemble(2)
    for r in range(2):
        E.fill_gauge(r, 10 + r, 0.1)
    for values in ((2, 2), (1, 2), (0, 1), (1, 0), (-1, -1)):
        bad = (sm.HMCParams * 2)(prm(sm, 1, even_odd=values[0]), prm(sm, 3, even_odd=values[1]))
        assert lib.sm_ens_hmc_trajectory(E.ens, bad, 0, res) == SM_ERR_ARG
        assert b"even_odd" in lib.sm_last_error()
    outs = E.trajectory([prm(sm, 1), prm(sm, 3)], 0)
    assert all(o.cg_failures == 0 for o in outs)
    E.close()


# ---- f. statistics ----------------------------------------------------------------------------
def test_even_odd_ensemble_matches_reference_statistics(sm):
    """The hmc_stat protocol with R = 4 replicas, seeds 777 + r: the mean of the
    replicas' Ep against the reference program's recorded run under
    test_even_odd_hmc_matches_reference_statistics' criterion, the error of the
    mean from the replicas' jackknife errors."""
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        ref = json.load(f)["hmc_stat"]
    R = 4
    L = sm.Lattice(ref["Nx"], ref["Nt"])
    E = L.ensemble(R)
    params = [sm.HMCParams(ref["m0"], ref["beta"], ref["tau"], ref["md_steps"], 1e-10, MAXIT, 777 + r, 1)
              for r in range(R)]
    out, sp, gs = E.run(params, ref["Ntherm"], ref["Nmeas"], ref["Nsteps"], hot_start=True)
    E.close()
    L.close()
    Ep = sum(s.Ep for s in out) / R
    dEp = math.sqrt(sum(s.dEp ** 2 for s in out)) / R
    print(f"EO ENSEMBLE STAT: Ep {Ep:.6f} +- {dEp:.6f} (reference {ref['Ep']} +- {ref['dEp']}), acceptance "
          f"{[round(s.acceptance, 3) for s in out]}, CG iterations per trajectory "
          f"{[s.cg_iterations // s.trajectories for s in out]}")
    assert all(s.cg_failures == 0 for s in out)
    assert abs(Ep - ref["Ep"]) <= 4 * math.hypot(dEp, ref["dEp"]) + 1e-3, (Ep, dEp, ref["Ep"], ref["dEp"])
    assert all(s.acceptance >= ref["acceptance"] - 0.15 for s in out)
