"""The pion correlator of every replica of an ensemble (sm_ens_pion_correlator,
solver 0 = D D^dag, 1 = even-odd) and the even-odd solve of the lone context's
correlator (sm_pion_solver).

Shapes sit at the edges of the new kernels and of the solvers underneath (the
plain tile is 60 t-columns, the even-odd tile 56 k-columns, a slice block has 64
t-values): 6x10 one partial tile; 16x16; 5x9 odd (solver 0 only); 16x62
half-width 31; 8x122 two slice blocks, a second plain tile and a second
even-odd k-tile. Every shape uses the sources (0,0), (Nx-1,Nt-1), (Nx//2,Nt//3)
and (1,0): both site parities and both t-boundary wraps. Fields are
mixed_model.synthetic's with one gauge_seed per replica, the masses differ per
replica.

Accuracy is held to the bound derived in ens_pion_model.py from the stop test
and sigma_min(D) of the dense model, times 2; everything else is bitwise.

Worst |C - C*| / (2 x bound) measured on an MI355X, tol 1e-10 (test c), solver 0 /
solver 1: 6x10 8.6e-3 / 5.9e-3, 16x16 5.7e-3 / 6.4e-3, 5x9 8.3e-3 / -, 16x62
7.6e-3 / 6.0e-3, 8x122 7.6e-3 / 8.3e-3.
"""
import ctypes

import numpy as np
import pytest

import ens_pion_model as epm
from conftest import bits_equal, ptr

pytestmark = pytest.mark.gpu

SM_ERR_ARG, SM_ERR_STATE = 1, 4
TOL, MAX_ITER = epm.TOL, epm.MAX_ITER
SOLVERS = ("plain", "even_odd")


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def shapes_of(solver):
    return epm.SHAPES_ALL if solver in (0, "plain") else epm.SHAPES_EVEN


CASES = [(solver, shape) for solver in SOLVERS for shape in shapes_of(solver)]
CASE_IDS = [f"{solver}-{epm.shape_id(shape)}" for solver, shape in CASES]


def report(results):
    """[(converged, iterations, residual bits)] of a list of CGResult."""
    return [(r.converged, r.iterations, np.float64(r.residual).view(np.uint64).item()) for r in results]


def lone(sm, Nx, Nt, U):
    L = sm.Lattice(Nx, Nt)
    S = Nx * Nt
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
    return L


def filled(sm, L, Nx, Nt, fields):
    E = L.ensemble(len(fields))
    for r, U in enumerate(fields):
        E.upload_gauge(r, epm.as_complex(U, Nx, Nt))
    return E


_RUNS = {}


def three_replicas(sm, shape, solver):
    """(C, results) of the R = 3 ensemble of epm.SEEDS / epm.MASSES, measured once per (shape, solver)."""
    key = (shape, solver)
    if key not in _RUNS:
        Nx, Nt = shape
        L = sm.Lattice(Nx, Nt)
        try:
            E = filled(sm, L, Nx, Nt, [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS])
            C, res = E.pion_correlator(epm.MASSES, epm.sources(Nx, Nt), solver=solver, tol=TOL, max_iter=MAX_ITER)
            E.close()
        finally:
            L.close()
        C.setflags(write=False)
        _RUNS[key] = (C, [report(r) for r in res])
    return _RUNS[key]


# ---- a. solver 0 against the lone context ---------------------------------------------
@pytest.mark.parametrize("shape", epm.SHAPES_ALL, ids=epm.shape_id)
def test_plain_solver_is_bitwise_the_lone_correlator(sm, shape):
    Nx, Nt = shape
    src = epm.sources(Nx, Nt)
    C, res = three_replicas(sm, shape, "plain")
    assert C.shape == (3, len(src), Nt) and all(len(r) == 2 * len(src) for r in res)
    for r, (seed, m0) in enumerate(zip(epm.SEEDS, epm.MASSES)):
        L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, seed))
        try:
            Cl, rl = L.pion_correlator(m0, src, tol=TOL, max_iter=MAX_ITER)
        finally:
            L.close()
        assert bits_equal(np.ascontiguousarray(C[r]), Cl), f"replica {r}"
        assert res[r] == report(rl), f"replica {r}"


# ---- b. independence -------------------------------------------------------------------
@pytest.mark.parametrize("solver,shape", CASES, ids=CASE_IDS)
def test_a_replica_is_bitwise_independent_of_its_neighbours(sm, solver, shape):
    Nx, Nt = shape
    src = epm.sources(Nx, Nt)
    probe_U, probe_m = epm.as_complex(epm.gauge(sm, Nx, Nt, 4242), Nx, Nt), -0.07
    L = sm.Lattice(Nx, Nt)
    try:
        def measure(R, at, salt):
            E = L.ensemble(R)
            masses = []
            for r in range(R):
                if r in at:
                    E.upload_gauge(r, probe_U)
                    masses.append(probe_m)
                else:
                    E.fill_gauge(r, 7000 + 31 * salt + r, 0.25 + 0.01 * ((salt + r) % 7))
                    masses.append(-0.05 + 0.02 * ((salt + 3 * r) % 6))
            C, res = E.pion_correlator(masses, src, solver=solver, tol=TOL, max_iter=MAX_ITER)
            E.close()
            return {r: (np.ascontiguousarray(C[r]), report(res[r])) for r in at}

        want = measure(1, {0}, 0)[0]
        assert all(c == 1 for c, _, _ in want[1])
        for pos in range(5):
            got = measure(5, {pos}, pos + 1)[pos]
            assert bits_equal(got[0], want[0]) and got[1] == want[1], f"R = 5, position {pos}"
        if shape in ((6, 10), (16, 16)):
            got = measure(64, {37, 63}, 9)
            for pos in (37, 63):
                assert bits_equal(got[pos][0], want[0]) and got[pos][1] == want[1], f"R = 64, position {pos}"
    finally:
        L.close()


# ---- c. accuracy -----------------------------------------------------------------------
@pytest.mark.parametrize("solver,shape", CASES, ids=CASE_IDS)
def test_within_the_derived_bound_of_the_dense_model(sm, solver, shape):
    Nx, Nt = shape
    C, res = three_replicas(sm, shape, solver)
    worst = 0.0
    for r, (seed, m0) in enumerate(zip(epm.SEEDS, epm.MASSES)):
        M = epm.model(sm, Nx, Nt, seed, m0)
        B = epm.MARGIN * epm.bound(M, Nx, Nt, tol=TOL, even_odd=solver == "even_odd")
        dev = np.abs(C[r] - M["C"])
        i = np.unravel_index(np.argmax(dev / B), dev.shape)
        print(f"ENS PION ACCURACY {solver} {Nx}x{Nt} replica {r} (m0 {m0}, sigma_min {M['sigma_min']:.4f}): worst "
              f"slice (source {i[0]}, t {i[1]}) deviation {dev[i]:.3e} allowed {B[i]:.3e} ratio {dev[i] / B[i]:.3e}; "
              f"C there {M['C'][i]:.3e}; iterations {min(k for _, k, _ in res[r])}..{max(k for _, k, _ in res[r])}")
        worst = max(worst, float((dev / B).max()))
        assert all(c == 1 for c, _, _ in res[r]), f"replica {r}"
        assert np.all(dev <= B), f"replica {r}"
    print(f"ENS PION ACCURACY {solver} {Nx}x{Nt}: worst ratio {worst:.3e}")


# ---- d. iteration ratio ----------------------------------------------------------------
@pytest.mark.parametrize("shape", epm.SHAPES_EVEN, ids=epm.shape_id)
def test_even_odd_columns_take_fewer_iterations(sm, shape):
    _, plain = three_replicas(sm, shape, "plain")
    _, eo = three_replicas(sm, shape, "even_odd")
    ratios = []
    for r in range(3):
        for k, ((_, it0, _), (_, it1, _)) in enumerate(zip(plain[r], eo[r])):
            ratios.append(it1 / it0)
            assert it1 < it0, f"replica {r} column {k}: {it1} even-odd iterations, {it0} plain"
    print(f"ENS PION ITERATIONS {shape[0]}x{shape[1]}: even-odd / plain in [{min(ratios):.3f}, {max(ratios):.3f}], "
          f"mean {np.mean(ratios):.3f}")


# ---- e. chains undisturbed -------------------------------------------------------------
@pytest.mark.parametrize("even_odd", [0, 1], ids=["plain-action", "even-odd-action"])
def test_measurements_leave_the_chains_and_the_context_alone(sm, even_odd):
    Nx, Nt = 6, 10
    src = epm.sources(Nx, Nt)
    fields = [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS]
    params = [sm.HMCParams(m0, 2.0 + 0.5 * r, 0.4, 6, 1e-10, 10000, 11 + r, even_odd)
              for r, m0 in enumerate(epm.MASSES)]
    L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, 1234))
    try:
        before = L.pion_correlator(0.03, src, tol=TOL, max_iter=MAX_ITER)
        logs = []
        for measured in (False, True):
            E = filled(sm, L, Nx, Nt, fields)
            log = []
            for t in range(3):
                if measured:
                    for solver in SOLVERS:
                        C, res = E.pion_correlator(epm.MASSES, src, solver=solver, tol=TOL, max_iter=MAX_ITER)
                        assert all(c == 1 for rr in res for c in [x.converged for x in rr])
                out = E.trajectory(params, t)
                log.append([bytes(o) for o in out])
                log.append([E.download_gauge(r).tobytes() for r in range(3)])
            E.close()
            logs.append(log)
        assert logs[0] == logs[1]
        after = L.pion_correlator(0.03, src, tol=TOL, max_iter=MAX_ITER)
        assert bits_equal(before[0], after[0]) and report(before[1]) == report(after[1])
    finally:
        L.close()


# ---- f. repeatability and refusals -------------------------------------------------------
def test_repeatable_and_refusals(sm):
    Nx, Nt = 6, 10
    kmax = sm.lib.sm_cg_batch_max()
    src = epm.sources(Nx, Nt)
    R = 2
    L = sm.Lattice(Nx, Nt)
    O = sm.Lattice(5, 9)
    try:
        E = filled(sm, L, Nx, Nt, [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS[:R]])
        masses = list(epm.MASSES[:R])
        for solver in SOLVERS:
            C1, r1 = E.pion_correlator(masses, src, solver=solver)
            C2, r2 = E.pion_correlator(masses, src, solver=solver)
            assert bits_equal(C1, C2) and [report(r) for r in r1] == [report(r) for r in r2]
        n = kmax // 2 + 1
        sx, st = (ctypes.c_int * n)(), (ctypes.c_int * n)()
        m = np.array(masses)
        C = np.zeros(R * n * Nt)
        res = (sm.CGResult * (R * 2 * n))()

        def call(e=E.ens, m0=ptr(m), solver=0, nsrc=1, x0=0, t0=0, max_iter=10000, px=sx, pt=st, out=ptr(C), rs=res):
            sx[0], st[0] = x0, t0
            return sm.lib.sm_ens_pion_correlator(e, m0, 1e-10, max_iter, solver, nsrc, px, pt, out, rs)

        def works():
            """The ensemble still measures, both solvers, and res may be null."""
            for solver in (0, 1):
                assert call(solver=solver, rs=None) == 0
                want = E.pion_correlator(masses, [(0, 0)], solver=solver)[0]
                assert bits_equal(C[:R * Nt].reshape(R, 1, Nt), want)

        works()
        refused = [dict(e=None), dict(m0=None), dict(px=None), dict(pt=None), dict(out=None), dict(solver=2),
                   dict(solver=-1), dict(nsrc=0), dict(nsrc=-1), dict(nsrc=n), dict(x0=Nx), dict(x0=-1), dict(t0=Nt),
                   dict(t0=-1), dict(max_iter=-1)]
        for kw in refused:
            assert call(**kw) == SM_ERR_ARG, kw
            works()
        assert call(nsrc=kmax // 2) == 0        # 2 nsrc = the cap is accepted
        assert call(nsrc=kmax // 2, solver=1) == 0
        E.close()
        # solver 1 on an odd lattice: refused naming the checkerboard; solver 0 still works
        Eo = filled(sm, O, 5, 9, [epm.gauge(sm, 5, 9, 5)])
        mo, Co = np.array([0.0]), np.zeros(9)
        assert sm.lib.sm_ens_pion_correlator(Eo.ens, ptr(mo), 1e-10, 10000, 1, 1, sx, st, ptr(Co), None) == SM_ERR_ARG
        assert b"checkerboard" in sm.lib.sm_last_error()
        with pytest.raises(sm.SMError, match="checkerboard"):
            Eo.pion_correlator([0.0], [(0, 0)], solver="even_odd")
        Cp, rp = Eo.pion_correlator([0.0], [(0, 0)], solver="plain")
        assert all(x.converged == 1 for x in rp[0]) and np.all(Cp > 0)
        Eo.close()
        # a replica without a gauge field
        Eh = L.ensemble(2)
        Eh.upload_gauge(0, epm.as_complex(epm.gauge(sm, Nx, Nt, 5), Nx, Nt))
        assert call(e=Eh.ens) == SM_ERR_STATE
        Eh.fill_gauge(1, 3, 0.3)
        assert call(e=Eh.ens) == 0
        Eh.close()
    finally:
        L.close()
        O.close()


# ---- g. sm_pion_solver -------------------------------------------------------------------
@pytest.mark.parametrize("shape", epm.SHAPES_EVEN, ids=epm.shape_id)
def test_pion_solver_switch(sm, shape):
    Nx, Nt = shape
    src = epm.sources(Nx, Nt)
    seed, m0 = epm.SEEDS[0], epm.MASSES[0]
    U = epm.gauge(sm, Nx, Nt, seed)
    L = lone(sm, Nx, Nt, U)
    try:
        assert L.pion_solver() == "plain"                       # the default, and its bits
        C0, r0 = L.pion_correlator(m0, src, tol=TOL, max_iter=MAX_ITER)
        Cp, rp = three_replicas(sm, shape, "plain")
        assert bits_equal(C0, np.ascontiguousarray(Cp[0])) and report(r0) == rp[0]
        assert L.pion_solver("even_odd") == "even_odd"
        C1, r1 = L.pion_correlator(m0, src, tol=TOL, max_iter=MAX_ITER)
        assert [x.used for x in L.last_cg_batch_mixed] == [0] * (2 * len(src))
        E = filled(sm, L, Nx, Nt, [U])                          # bitwise the ensemble's solver 1 at R = 1
        Ce, re_ = E.pion_correlator([m0], src, solver="even_odd", tol=TOL, max_iter=MAX_ITER)
        E.close()
        assert bits_equal(C1, np.ascontiguousarray(Ce[0])) and report(r1) == report(re_[0])
        M = epm.model(sm, Nx, Nt, seed, m0)                     # and within the bound of test c
        B = epm.MARGIN * epm.bound(M, Nx, Nt, tol=TOL, even_odd=True)
        dev = np.abs(C1 - M["C"])
        print(f"PION SOLVER 1 {Nx}x{Nt}: worst ratio {(dev / B).max():.3e}; iterations "
              f"{[x.iterations for x in r1]} against {[x.iterations for x in r0]}")
        assert all(x.converged == 1 for x in r1) and np.all(dev <= B)
        # the mode persists across calls and gauge uploads
        S = Nx * Nt
        V2 = epm.gauge(sm, Nx, Nt, epm.SEEDS[1])
        sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(V2[:2 * S]), ptr(V2[2 * S:])))
        assert L.pion_solver() == "even_odd"
        sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
        C2, r2 = L.pion_correlator(m0, src, tol=TOL, max_iter=MAX_ITER)
        assert bits_equal(C1, C2) and report(r1) == report(r2)
        # the batched precision switch does not reach mode 1
        assert L.cg_batch_precision("mixed") == "mixed"
        C3, r3 = L.pion_correlator(m0, src, tol=TOL, max_iter=MAX_ITER)
        assert bits_equal(C1, C3) and report(r1) == report(r3)
        assert L.cg_batch_precision("double") == "double"
        # other values are refused and leave the mode
        mode = ctypes.c_int(-1)
        assert sm.lib.sm_pion_solver(L.ctx, 2, ctypes.byref(mode)) == SM_ERR_ARG and mode.value == 1
        assert sm.lib.sm_pion_solver(L.ctx, -1, ctypes.byref(mode)) == 0 and mode.value == 1
        assert L.pion_solver("plain") == "plain"
        C4, r4 = L.pion_correlator(m0, src, tol=TOL, max_iter=MAX_ITER)
        assert bits_equal(C0, C4) and report(r0) == report(r4)
    finally:
        L.close()


def test_pion_solver_refusals(sm):
    B = sm.Lattice(8, 8, loopback=True)
    try:
        mode = ctypes.c_int(-1)
        assert sm.lib.sm_pion_solver(B.ctx, 1, ctypes.byref(mode)) == SM_ERR_ARG and mode.value == 0
        with pytest.raises(sm.SMError):
            B.pion_solver("even_odd")
        assert B.pion_solver() == "plain"
    finally:
        B.close()
    # an odd lattice: the switch is taken, the correlator call refuses, mode 0 still works
    Nx, Nt = 5, 9
    L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, epm.SEEDS[0]))
    try:
        want = L.pion_correlator(0.0, [(0, 0), (1, 0)], tol=TOL, max_iter=MAX_ITER)
        assert L.pion_solver("even_odd") == "even_odd"
        sx, st = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0)
        C = np.zeros(Nt)
        assert sm.lib.sm_pion_correlator(L.ctx, 0.0, TOL, MAX_ITER, 1, sx, st, ptr(C), None) == SM_ERR_ARG
        assert b"checkerboard" in sm.lib.sm_last_error()
        assert L.pion_solver("plain") == "plain"
        got = L.pion_correlator(0.0, [(0, 0), (1, 0)], tol=TOL, max_iter=MAX_ITER)
        assert bits_equal(want[0], got[0]) and report(want[1]) == report(got[1])
    finally:
        L.close()
