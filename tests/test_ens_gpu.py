"""The replica ensemble (sm_ens_*, schwingermodel_amd/csrc/sm_ens.cpp): R HMC
chains in lockstep, one launch per step for all of them.

Geometries are the batched kernels' edges, not the workload: 6x10 (one partial
tile), 16x61 (a second t-tile holding one owned column), 64x64 (redundant
scalars, P = 128), 260x121 (P = 780 > 512: the scalar-kernel path).
Parameters: m0 in {0, 0.1, 0.2}, beta in {2, 3}, tau 0.3-0.5, md_steps 6,
tol 1e-10.

The per-column CG has no test-only entry through the ensemble, so the solve on
per-column links and masses is checked through the trajectory against the lone
chain (test_against_the_lone_chain: H_old and H_new hold the solves' fermion
terms, the evolved field every force solve), one trajectory at a time with the
start fields synchronised -- the two solvers sum in different orders, so free
chains would drift apart. Tolerances there are test_md_gpu.py's for anything
downstream of a CG solve (H relative 1e-10, fields relative 1e-8, iteration
totals +-1 %), justified there by the reference's own spread between
decompositions. Everything that involves no second solver is bitwise.

Start fields. With md_steps 6 the step is eps = 0.05-0.083, and a field far
from equilibrium has dH proportional to the volume: from a hot start dH is
+19 to +360 at 260x121 and every trajectory is rejected, so the field would
never move. A smooth start (angles of width 0.1) heats up instead: dH < 0 and
the first trajectories are accepted at every geometry. At m0 = 0 a smooth field
is an exceptional configuration (thousands of CG iterations), so those
replicas start from rough fields (width 0.4) and mostly reject on the larger
lattices. Between them the ensembles here hold accepting and rejecting
replicas side by side.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import bits_equal, ptr

pytestmark = pytest.mark.gpu

GEOMS = [(6, 10), (16, 61), (64, 64), (260, 121)]
IDS = [f"{a}x{b}" for a, b in GEOMS]
MD_STEPS, TOL, MAXIT = 6, 1e-10, 10000
M0S, BETAS, TAUS = (0.0, 0.1, 0.2), (2.0, 3.0), (0.3, 0.4, 0.5)
SM_ERR_ARG, SM_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


@pytest.fixture(scope="module")
def lattices(sm):
    """One context per geometry, shared by the tests of this module."""
    made = {}

    def get(Nx, Nt):
        if (Nx, Nt) not in made:
            made[(Nx, Nt)] = sm.Lattice(Nx, Nt)
        return made[(Nx, Nt)]

    yield get
    for L in made.values():
        L.close()


def prm(sm, i, seed=None, tau=None):
    """Parameter set number i of the cycle over (m0, beta, tau)."""
    return sm.HMCParams(M0S[i % 3], BETAS[i % 2], TAUS[(i // 2) % 3] if tau is None else tau, MD_STEPS, TOL, MAXIT,
                        1000 + i if seed is None else seed, 0)


def start_sigma(p):
    return 0.1 if p.m0 > 0 else 0.4


def host_gauge(sm, Nx, Nt, seed, sigma):
    U = np.empty((2, Nx * Nt), dtype=np.complex128)
    sm.lib.sm_fill_gauge(seed, sigma, Nt, 0, Nx, 0, Nt, ptr(U[0]), ptr(U[1]))
    return U


def lone_upload(sm, L, U):
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[0]), ptr(U[1])))


def lone_download(sm, L):
    U = np.empty((2, L.V), dtype=np.complex128)
    sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(U[0]), ptr(U[1])))
    return U


def lone_plaquette(sm, L, U, beta):
    lone_upload(sm, L, U)
    sp, act = ctypes.c_double(), ctypes.c_double()
    sm.check(sm.lib.sm_plaquette(L.ctx, beta, ctypes.byref(sp), ctypes.byref(act), None))
    return sp.value, act.value


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def bits(x):
    return np.float64(x).view(np.uint64)


def entry(o, U):
    """What a replica's log keeps of one trajectory."""
    return (bits(o.H_old), bits(o.H_new), bits(o.dH), bits(o.r), o.accepted, o.cg_iterations, o.cg_failures,
            bits(o.sp), bits(o.gauge_action), U.tobytes())


def run_logs(E, params, ntraj=3, watch=None):
    """Logs of the watched replicas (default all) over ntraj trajectories."""
    watch = range(E.R) if watch is None else watch
    logs = {r: [] for r in watch}
    for t in range(ntraj):
        outs = E.trajectory(params, t)
        for r in watch:
            logs[r].append(entry(outs[r], E.download_gauge(r)))
    return logs


def members(sm, E, probe, probe_at, salt):
    """Fill E: the probe (params, start field) at the positions probe_at,
    neighbours with other beta, m0, tau, seeds and start fields elsewhere."""
    params = []
    for r in range(E.R):
        if r in probe_at:
            params.append(probe[0])
            E.upload_gauge(r, probe[1])
        else:
            params.append(prm(sm, salt + r + 1))
            E.fill_gauge(r, 5000 + 97 * salt + r, start_sigma(params[-1]))
    return params


@pytest.mark.parametrize("Nx,Nt", GEOMS, ids=IDS)
def test_replica_independence_bitwise(sm, lattices, Nx, Nt):
    """A replica's log (H_old, H_new, dH, r, accepted, iterations, sp, action
    and the field's bytes after each of 3 trajectories) is the same alone, at
    every position of R = 5 and inside R = 64; two replicas with the same
    params, seed and start produce equal logs."""
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
    E = L.ensemble(64)
    logs = run_logs(E, members(sm, E, probe, {37, 63}, 3), watch=[37, 63])
    E.close()
    assert logs[37] == want, "R = 64, position 37"
    assert logs[63] == want, "R = 64, position 63 (same params, seed and start as 37)"


@pytest.mark.parametrize("Nx,Nt", GEOMS, ids=IDS)
def test_against_the_lone_chain(sm, lattices, Nx, Nt):
    """4 replicas x 3 trajectories against sm_hmc_trajectory on a lone context
    from the same start field, (seed, traj) and params; the lone chain's
    resulting field is the next start of both."""
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
            print(f"{Nx}x{Nt} traj {t} replica {r}: H_old {o.H_old!r} / {lo.H_old!r} H_new {o.H_new!r} / {lo.H_new!r} "
                  f"r {o.r!r} dH {o.dH!r} / {lo.dH!r} it {o.cg_iterations} / {lo.cg_iterations}")
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
    assert fields_compared >= 3  # the smooth-start replicas accept


@pytest.mark.parametrize("Nx,Nt", GEOMS, ids=IDS)
def test_bookkeeping_per_replica(sm, lattices, Nx, Nt):
    """accepted == (r <= exp(-dH)); a rejected replica keeps its field bitwise;
    sp and gauge_action are sm_plaquette's bits on the downloaded field, and so
    are sm_ens_plaquette's; two identical runs agree bitwise. Replicas 3 and 4
    take steps of eps = 1 (tau = 6), beyond the leapfrog's stability bound, so
    that rejects occur among the accepts."""
    L = lattices(Nx, Nt)
    R = 5
    params = [prm(sm, i) for i in range(3)] + [prm(sm, 3, tau=6.0), prm(sm, 4, tau=6.0)]
    betas = [p.beta for p in params]
    starts = [host_gauge(sm, Nx, Nt, 700 + r, start_sigma(params[r])) for r in range(R)]
    runs = []
    seen = set()
    for _ in range(2):
        E = L.ensemble(R)
        for r in range(R):
            E.upload_gauge(r, starts[r])
        before = [u.copy() for u in starts]
        log = []
        for t in range(3):
            outs = E.trajectory(params, t)
            after = [E.download_gauge(r) for r in range(R)]
            sp_e, act_e = E.plaquette(betas)
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
                assert bits(sp_e[r]) == bits(sp) and bits(act_e[r]) == bits(act)
                log.append(entry(o, after[r]))
            before = after
        E.close()
        runs.append(log)
    assert runs[0] == runs[1]
    assert seen == {0, 1}


def seq_mean(x):
    s = 0.0
    for v in x:
        s += v
    return s / len(x)


def test_run_driver(sm, lattices, tmp_path):
    N, R, Ntherm, Nmeas, Nsteps = 16, 4, 2, 5, 1
    V = N * N
    L = lattices(N, N)
    params = [prm(sm, i) for i in range(R)]
    E = L.ensemble(R)
    prefix = str(tmp_path / "conf")
    out, sp, gs = E.run(params, Ntherm, Nmeas, Nsteps, hot_start=True, first_traj=0, save_prefix=prefix)
    for r in range(R):
        s = out[r]
        assert s.trajectories == Ntherm + Nmeas + Nsteps * (Nmeas - 1)
        assert s.cg_failures == 0 and s.cg_iterations > 0
        assert s.Ep == seq_mean(sp[r]) / V
        assert s.dEp == sm.lib.sm_jackknife_error(sp[r].ctypes.data, Nmeas, 20) / V
        assert s.gS == seq_mean(gs[r]) / V
        assert s.dgS == sm.lib.sm_jackknife_error(gs[r].ctypes.data, Nmeas, 20) / V
        assert abs(s.gS - params[r].beta * (1.0 - s.Ep)) <= 1e-12
        assert s.acceptance == s.accepted / (Nmeas + Nsteps * (Nmeas - 1))
        assert 0 <= s.accepted <= Nmeas + Nsteps * (Nmeas - 1)
        for i in range(Nmeas):  # 28-byte records
            assert os.path.getsize(f"{prefix}_r{r}_{i}.ctxt") == V * 2 * 28
        # the last saved configuration is the replica's field, bitwise on reading back
        last = f"{prefix}_r{r}_{Nmeas - 1}.ctxt"
        U = np.empty((2, V), dtype=np.complex128)
        sm.check(sm.lib.sm_conf_read(last.encode(), N, N, ptr(U[0]), ptr(U[1])))
        assert bits_equal(U.view(np.float64), E.download_gauge(r).view(np.float64))
        # and the series' last entry is its plaquette sum
        spv, act = lone_plaquette(sm, L, U, params[r].beta)
        assert bits(sp[r, -1]) == bits(spv) and bits(gs[r, -1]) == bits(act)
    assert len(list(tmp_path.iterdir())) == R * Nmeas
    E.close()


def test_hot_start_and_draws_are_the_lone_chains(sm, lattices):
    """Nmeas = 1, Ntherm = 0 from a hot start: trajectory 0 of every replica
    against sm_hmc_run's on a lone context with the same seed (r bitwise, the
    rest to the solvers' rounding)."""
    N, R = 16, 3
    L = lattices(N, N)
    params = [prm(sm, i) for i in range(R)]
    E = L.ensemble(R)
    out, sp, gs = E.run(params, 0, 1, 0, hot_start=True)
    for r in range(R):
        s = sm.HMCSummary()
        sp1, gs1 = np.empty(1), np.empty(1)
        sm.check(sm.lib.sm_hmc_run(L.ctx, ctypes.byref(params[r]), 1, 0, 0, 1, 0, None, ctypes.byref(s), ptr(sp1),
                                   ptr(gs1)))
        assert s.accepted == out[r].accepted
        assert abs(s.cg_iterations - out[r].cg_iterations) <= max(1, s.cg_iterations // 100)
        if s.accepted:
            assert rel(E.download_gauge(r), lone_download(sm, L)) <= 1e-8
            assert abs(sp1[0] - sp[r, 0]) <= 1e-8 * abs(sp1[0])
        else:  # both kept the hot start: the same draw, bitwise
            assert bits_equal(E.download_gauge(r).view(np.float64), lone_download(sm, L).view(np.float64))
            assert bits(sp1[0]) == bits(sp[r, 0])
    E.close()


def test_neighbours_undisturbed(sm, lattices):
    """The context's gauge field, an sm_cg_dev solve (through sm_cg) and an
    sm_cg_batch solve are bitwise the same before and after an ensemble
    trajectory on that context; with an ensemble alive, a batched column still
    has the same bits at K = 1 and inside K = 5."""
    Nx, Nt, m0 = 16, 61, 0.1
    L = lattices(Nx, Nt)
    V = Nx * Nt
    U = host_gauge(sm, Nx, Nt, 91, 0.4)
    lone_upload(sm, L, U)
    phi = np.empty((5, 2, V), dtype=np.complex128)
    for b in range(5):
        sm.lib.sm_fill_spinor(40 + b, Nt, 0, Nx, 0, Nt, ptr(phi[b, 0]), ptr(phi[b, 1]))

    def solves():
        x = np.empty((2, V), dtype=np.complex128)
        res = sm.CGResult()
        sm.check(sm.lib.sm_cg(L.ctx, ptr(phi[0, 0]), ptr(phi[0, 1]), ptr(x[0]), ptr(x[1]), m0, TOL, MAXIT,
                              ctypes.byref(res)))
        xb, rb = L.cg_batch(phi, m0, tol=TOL, max_iter=MAXIT)
        return x, res.iterations, xb, [r.iterations for r in rb]

    x0, it0, xb0, itb0 = solves()
    E = L.ensemble(3)
    params = [prm(sm, i) for i in range(3)]
    for r in range(3):
        E.fill_gauge(r, 60 + r, start_sigma(params[r]))
    outs = E.trajectory(params, 0)
    assert all(o.cg_failures == 0 for o in outs)
    x1, it1, xb1, itb1 = solves()
    assert bits_equal(lone_download(sm, L).view(np.float64), U.view(np.float64))
    assert it0 == it1 and itb0 == itb1
    assert bits_equal(x0.view(np.float64), x1.view(np.float64))
    assert bits_equal(xb0.view(np.float64), xb1.view(np.float64))
    xk1, rk1 = L.cg_batch(phi[2:3].copy(), m0, tol=TOL, max_iter=MAXIT)
    assert rk1[0].iterations == itb1[2]
    assert bits_equal(xk1[0].view(np.float64), xb1[2].view(np.float64))
    E.trajectory(params, 1)  # and the ensemble goes on unharmed
    E.close()


def test_refusals(sm, lattices):
    lib = sm.lib
    L = lattices(6, 10)
    h = ctypes.c_void_p()
    cap = lib.sm_ens_max()
    for R in (0, -1, cap + 1):
        assert lib.sm_ens_create(L.ctx, R, ctypes.byref(h)) == SM_ERR_ARG
        assert not h.value
    Lb = sm.Lattice(16, 16, loopback=True)
    assert lib.sm_ens_create(Lb.ctx, 2, ctypes.byref(h)) == SM_ERR_ARG
    assert b"one-shard" in lib.sm_last_error()
    Lb.close()

    E = L.ensemble(2)
    n = ctypes.c_int()
    sm.check(lib.sm_ens_size(E.ens, ctypes.byref(n)))
    assert n.value == 2
    good = (sm.HMCParams * 2)(prm(sm, 0), prm(sm, 1))
    res = (sm.HMCResult * 2)()
    # a replica without a field
    E.fill_gauge(0, 1, -1.0)
    assert lib.sm_ens_hmc_trajectory(E.ens, good, 0, res) == SM_ERR_STATE
    assert b"replica 1" in lib.sm_last_error()
    buf = np.zeros(4 * L.V)
    assert lib.sm_ens_download_gauge(E.ens, 1, ptr(buf), ptr(buf[2 * L.V:])) == SM_ERR_STATE
    assert lib.sm_ens_plaquette(E.ens, ptr(buf), ptr(buf), ptr(buf)) == SM_ERR_STATE
    E.fill_gauge(1, 2, -1.0)
    # r out of range, null pointers
    for r in (-1, 2):
        assert lib.sm_ens_fill_gauge(E.ens, r, 1, -1.0) == SM_ERR_ARG
        assert lib.sm_ens_upload_gauge(E.ens, r, ptr(buf), ptr(buf)) == SM_ERR_ARG
    assert lib.sm_ens_upload_gauge(E.ens, 0, None, ptr(buf)) == SM_ERR_ARG
    assert lib.sm_ens_hmc_trajectory(E.ens, None, 0, res) == SM_ERR_ARG
    assert lib.sm_ens_hmc_trajectory(E.ens, good, 0, None) == SM_ERR_ARG
    # lockstep: the C entry names the field (the Python layer would refuse earlier)
    for field, value in (("md_steps", 7), ("cg_tol", 1e-9), ("cg_max_iter", 77), ("even_odd", 1)):
        bad = (sm.HMCParams * 2)(prm(sm, 0), prm(sm, 1))
        setattr(bad[1], field, value)
        assert lib.sm_ens_hmc_trajectory(E.ens, bad, 0, res) == SM_ERR_ARG
        assert field.encode() in lib.sm_last_error()
        summ = (sm.HMCSummary * 2)()
        assert lib.sm_ens_hmc_run(E.ens, bad, 0, 0, 0, 1, 0, None, summ, None, None) == SM_ERR_ARG
    # and it still runs
    assert lib.sm_ens_hmc_trajectory(E.ens, good, 0, res) == 0
    E.close()
