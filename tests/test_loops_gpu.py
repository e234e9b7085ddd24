"""Stochastic quark loops on the GPU (sm_quark_loops, sm_ens_quark_loops; solver
0 = D D^dag, 1 = even-odd).

Shapes are ens_pion_model's, at the edges of the kernels and of the solvers
underneath (the plain tile is 60 t-columns, the even-odd tile 56 k-columns, a
contraction block has 64 t-values and 16 x-groups): 6x10 one partial tile,
fewer rows than x-groups; 16x16; 5x9 odd (solver 0 only); 16x62 half-width 31;
8x122 a second contraction block and a second solver tile. Three replicas with
epm.SEEDS / epm.MASSES and loops_model.NOISE_SEEDS, nnoise = 3; on 6x10 also
nnoise = 70, across the 64-column chunk.

Accuracy is held to the bound derived in loops_model.py from the stop test and
sigma_min(D) of the dense model, times 2; the estimator test to 4 of the
sample's own standard errors; everything else is bitwise.

The pion correlator's even-odd path shares its stage after the sources with
the loops since this feature; no earlier test pins its bits against an earlier
build (test_ens_pion_gpu.py compares the lone context with the ensemble, both
on the shared stage), so test_pion_even_odd_is_bitwise_what_it_was holds it to
tests/golden/pion_eo_before_loops.npz, computed with the library as it was
before the stage was factored out.

Worst |loops - model| / (2 x bound) measured on an MI355X, tol 1e-10 (test a),
solver 0 / solver 1: 6x10 1.1e-2 / 9.3e-3, 16x16 7.7e-3 / 8.9e-3, 5x9 1.3e-2 / -,
16x62 3.8e-3 / 4.5e-3, 8x122 7.4e-3 / 7.3e-3.
"""
import ctypes
import os

import numpy as np
import pytest

import ens_pion_model as epm
import loops_model as lm
from conftest import GOLDEN, bits_equal, ptr

pytestmark = pytest.mark.gpu

SM_ERR_ARG, SM_ERR_STATE = 1, 4
TOL, MAX_ITER = epm.TOL, epm.MAX_ITER
SOLVERS = ("plain", "even_odd")
NN = lm.NNOISE


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def shapes_of(solver):
    return epm.SHAPES_ALL if solver == "plain" else epm.SHAPES_EVEN


CASES = [(solver, shape) for solver in SOLVERS for shape in shapes_of(solver)]
CASE_IDS = [f"{solver}-{epm.shape_id(shape)}" for solver, shape in CASES]


def report(results):
    """[(converged, iterations, residual bits)] of a list of CGResult."""
    return [(r.converged, r.iterations, np.float64(r.residual).view(np.uint64).item()) for r in results]


def cbits(a, b):
    return bits_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


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


_ENS, _LONE = {}, {}


def three_replicas(sm, shape, solver):
    """(loops, reports) of the R = 3 ensemble of epm.SEEDS / epm.MASSES / lm.NOISE_SEEDS, once per case."""
    key = (shape, solver)
    if key not in _ENS:
        Nx, Nt = shape
        L = sm.Lattice(Nx, Nt)
        try:
            E = filled(sm, L, Nx, Nt, [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS])
            loops, res = E.quark_loops(epm.MASSES, NN, lm.NOISE_SEEDS, solver=solver, tol=TOL, max_iter=MAX_ITER)
            E.close()
        finally:
            L.close()
        loops.setflags(write=False)
        _ENS[key] = (loops, [report(r) for r in res])
    return _ENS[key]


def lone_replica(sm, shape, solver, r, nnoise=NN):
    """(loops, report) of a lone context holding replica r's field, once per case."""
    key = (shape, solver, r, nnoise)
    if key not in _LONE:
        Nx, Nt = shape
        L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, epm.SEEDS[r]))
        try:
            loops, res = L.quark_loops(epm.MASSES[r], nnoise, lm.NOISE_SEEDS[r], solver=solver, tol=TOL,
                                       max_iter=MAX_ITER)
        finally:
            L.close()
        loops.setflags(write=False)
        _LONE[key] = (loops, report(res))
    return _LONE[key]


# ---- a. accuracy -----------------------------------------------------------------------
@pytest.mark.parametrize("solver,shape", CASES, ids=CASE_IDS)
def test_within_the_derived_bound_of_the_dense_model(sm, solver, shape):
    Nx, Nt = shape
    loops, res = three_replicas(sm, shape, solver)
    assert loops.shape == (3, NN, Nt, 2) and all(len(r) == NN for r in res)
    worst = 0.0
    for r, (gseed, m0, nseed) in enumerate(zip(epm.SEEDS, epm.MASSES, lm.NOISE_SEEDS)):
        M = lm.model(sm, Nx, Nt, gseed, m0, nseed)
        B = epm.MARGIN * lm.bound(M, Nx, Nt, tol=TOL, even_odd=solver == "even_odd")       # (K,)
        want = lm.loops_array(M["S"], M["P"])
        for who, got in (("ensemble", loops[r]), ("lone", lone_replica(sm, shape, solver, r)[0])):
            dev = np.abs(got - want).max(axis=(1, 2))                                        # worst slice of S and P
            print(f"LOOPS ACCURACY {solver} {Nx}x{Nt} {who} replica {r} (m0 {m0}, sigma_min {M['sigma_min']:.4f}): "
                  f"deviation {dev.max():.3e} allowed {B[np.argmax(dev / B)]:.3e} ratio {(dev / B).max():.3e}; "
                  f"|S| up to {np.abs(want[..., 0]).max():.3e}; iterations {[k for _, k, _ in res[r]]}")
            worst = max(worst, float((dev / B).max()))
            assert np.all(dev <= B), f"{who} replica {r}"
        assert all(c == 1 for c, _, _ in res[r]), f"replica {r}"
    print(f"LOOPS ACCURACY {solver} {Nx}x{Nt}: worst ratio {worst:.3e}")


# ---- b. bitwise ------------------------------------------------------------------------
@pytest.mark.parametrize("solver,shape", CASES, ids=CASE_IDS)
def test_a_replica_is_bitwise_the_lone_context(sm, solver, shape):
    loops, res = three_replicas(sm, shape, solver)
    for r in range(3):
        ll, rl = lone_replica(sm, shape, solver, r)
        assert cbits(loops[r], ll), f"replica {r}"
        assert res[r] == rl, f"replica {r}"


@pytest.mark.parametrize("solver", SOLVERS)
def test_vectors_do_not_depend_on_nnoise_or_the_chunk(sm, solver):
    """nnoise = 70 crosses the 64-column chunk: its vectors 0-2 are the nnoise = 3 call's, vector 64 (first of
    the second chunk) is the same alone as the last of a 65-vector call; repeated calls agree."""
    shape = (6, 10)
    l3, r3 = lone_replica(sm, shape, solver, 0)
    l70, r70 = lone_replica(sm, shape, solver, 0, nnoise=70)
    assert l70.shape == (70, 10, 2) and len(r70) == 70
    assert cbits(l70[:3], l3) and r70[:3] == r3
    assert all(c == 1 for c, _, _ in r70)
    Nx, Nt = shape
    L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, epm.SEEDS[0]))
    try:
        again, ra = L.quark_loops(epm.MASSES[0], 70, lm.NOISE_SEEDS[0], solver=solver, tol=TOL, max_iter=MAX_ITER)
        assert cbits(again, l70) and report(ra) == r70
        l65, r65 = L.quark_loops(epm.MASSES[0], 65, lm.NOISE_SEEDS[0], solver=solver, tol=TOL, max_iter=MAX_ITER)
        assert cbits(l65, l70[:65]) and report(r65) == r70[:65]
        # the ensemble at nnoise = 5 next to the lone context's vectors
        E = filled(sm, L, Nx, Nt, [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS[:2]])
        le, re_ = E.quark_loops(epm.MASSES[:2], 5, lm.NOISE_SEEDS[:2], solver=solver, tol=TOL, max_iter=MAX_ITER)
        le2, re2 = E.quark_loops(epm.MASSES[:2], 5, lm.NOISE_SEEDS[:2], solver=solver, tol=TOL, max_iter=MAX_ITER)
        E.close()
        assert cbits(le, le2) and [report(r) for r in re_] == [report(r) for r in re2]
        assert cbits(le[0], l70[:5]) and report(re_[0]) == r70[:5]
    finally:
        L.close()


@pytest.mark.parametrize("solver,shape", [(s, sh) for s in SOLVERS for sh in ((6, 10), (8, 122))],
                         ids=[f"{s}-{epm.shape_id(sh)}" for s in SOLVERS for sh in ((6, 10), (8, 122))])
def test_permuting_replicas_permutes_results_and_one_replica_is_enough(sm, solver, shape):
    Nx, Nt = shape
    loops, res = three_replicas(sm, shape, solver)
    fields = [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS]
    perm = (2, 0, 1)
    L = sm.Lattice(Nx, Nt)
    try:
        E = filled(sm, L, Nx, Nt, [fields[p] for p in perm])
        lp, rp = E.quark_loops([epm.MASSES[p] for p in perm], NN, [lm.NOISE_SEEDS[p] for p in perm], solver=solver,
                               tol=TOL, max_iter=MAX_ITER)
        E.close()
        for i, p in enumerate(perm):
            assert cbits(lp[i], loops[p]) and report(rp[i]) == res[p], f"position {i} = replica {p}"
        E = filled(sm, L, Nx, Nt, [fields[1]])
        l1, r1 = E.quark_loops([epm.MASSES[1]], NN, [lm.NOISE_SEEDS[1]], solver=solver, tol=TOL, max_iter=MAX_ITER)
        E.close()
        assert cbits(l1[0], loops[1]) and report(r1[0]) == res[1]
    finally:
        L.close()


# ---- c. a measurement ------------------------------------------------------------------
@pytest.mark.parametrize("even_odd", [0, 1], ids=["plain-action", "even-odd-action"])
def test_measurements_leave_the_chains_and_the_context_alone(sm, even_odd):
    Nx, Nt = 6, 10
    S = Nx * Nt
    src = epm.sources(Nx, Nt)
    fields = [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS]
    params = [sm.HMCParams(m0, 2.0 + 0.5 * r, 0.4, 6, 1e-10, 10000, 11 + r, even_odd)
              for r, m0 in enumerate(epm.MASSES)]
    Uc = epm.gauge(sm, Nx, Nt, 1234)
    L = lone(sm, Nx, Nt, Uc)
    phi = np.stack([lm.noise(sm, Nx, Nt, 5, k).reshape(2, S) for k in range(2)])

    def context_state():
        d = np.empty(4 * S)
        sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(d[:2 * S]), ptr(d[2 * S:])))
        x, rx = L.cg_batch(phi, 0.03, tol=TOL, max_iter=MAX_ITER)
        out = [d.tobytes(), x.tobytes(), report(rx)]
        for mode in SOLVERS:
            L.pion_solver(mode)
            C, rc = L.pion_correlator(0.03, src, tol=TOL, max_iter=MAX_ITER)
            out += [C.tobytes(), report(rc)]
        L.pion_solver("plain")
        return out

    try:
        before = context_state()
        logs = []
        for measured in (False, True):
            E = filled(sm, L, Nx, Nt, fields)
            log = []
            for t in range(3):
                if measured:
                    for solver in SOLVERS:
                        _, res = E.quark_loops(epm.MASSES, 2, lm.NOISE_SEEDS, solver=solver, tol=TOL, max_iter=MAX_ITER)
                        assert all(x.converged == 1 for rr in res for x in rr)
                        _, rl = L.quark_loops(0.03, 2, 77, solver=solver, tol=TOL, max_iter=MAX_ITER)
                        assert all(x.converged == 1 for x in rl)
                out = E.trajectory(params, t)
                log.append([bytes(o) for o in out])
                log.append([E.download_gauge(r).tobytes() for r in range(3)])
            E.close()
            logs.append(log)
        assert logs[0] == logs[1]
        assert context_state() == before
        # a lone chain: the trajectory after a measurement is the trajectory without it
        outs = []
        for measured in (False, True):
            sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(Uc[:2 * S]), ptr(Uc[2 * S:])))
            if measured:
                for solver in SOLVERS:
                    L.quark_loops(0.03, 2, 77, solver=solver, tol=TOL, max_iter=MAX_ITER)
            r = sm.HMCResult()
            sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(params[0]), 0, ctypes.byref(r)))
            d = np.empty(4 * S)
            sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(d[:2 * S]), ptr(d[2 * S:])))
            outs.append((bytes(r), d.tobytes()))
        assert outs[0] == outs[1]
    finally:
        L.close()


PION_GOLDEN = os.path.join(GOLDEN, "pion_eo_before_loops.npz")


@pytest.mark.parametrize("shape", [(6, 10), (16, 62), (8, 122)], ids=epm.shape_id)
def test_pion_even_odd_is_bitwise_what_it_was(sm, shape):
    Nx, Nt = shape
    with np.load(PION_GOLDEN, allow_pickle=False) as z:
        C0, R0 = z[f"C_{Nx}x{Nt}"], z[f"res_{Nx}x{Nt}"]
    L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, epm.SEEDS[0]))
    try:
        L.pion_solver("even_odd")
        C, res = L.pion_correlator(epm.MASSES[0], epm.sources(Nx, Nt), tol=TOL, max_iter=MAX_ITER)
        E = filled(sm, L, Nx, Nt, [epm.gauge(sm, Nx, Nt, epm.SEEDS[0])])
        Ce, re_ = E.pion_correlator([epm.MASSES[0]], epm.sources(Nx, Nt), solver="even_odd", tol=TOL,
                                    max_iter=MAX_ITER)
        E.close()
    finally:
        L.close()
    want = [tuple(int(v) for v in row) for row in R0]
    assert bits_equal(C, C0) and report(res) == want
    assert bits_equal(np.ascontiguousarray(Ce[0]), C0) and report(re_[0]) == want


# ---- d. estimator ----------------------------------------------------------------------
def test_device_loops_estimate_the_exact_traces(sm):
    from schwingermodel_amd import loops as est
    Nx, Nt = lm.ESTIMATOR_SHAPE
    N = lm.ESTIMATOR_N
    gseed, m0 = epm.SEEDS[0], -0.10
    L = lone(sm, Nx, Nt, epm.gauge(sm, Nx, Nt, gseed))
    try:
        loops, res = L.quark_loops(m0, N, lm.ESTIMATOR_SEED, tol=TOL, max_iter=MAX_ITER)
    finally:
        L.close()
    assert all(r.converged == 1 for r in res)
    trS, trP = lm.exact_traces(np.linalg.inv(epm.model(sm, Nx, Nt, gseed, m0)["D"]), Nx, Nt)
    worst = 0.0
    for c, exact in ((0, trS), (1, trP)):
        for part in (np.real, np.imag):
            v = part(loops[:, :, c])
            z = np.abs(v.mean(axis=0) - part(exact)) / (v.std(axis=0, ddof=1) / np.sqrt(N))
            worst = max(worst, float(z.max()))
            assert np.all(z <= 4.0), (c, part.__name__, z.max())
    val, err = est.condensate(loops, Nx * Nt, nf=lm.NF)
    exact = lm.NF / (Nx * Nt) * trS.sum().real
    print(f"LOOPS ESTIMATOR {Nx}x{Nt}, {N} vectors: worst {worst:.2f} stderr; condensate {val:.5f} +- {err:.5f}, "
          f"exact {exact:.5f}")
    assert abs(val - exact) <= 4.0 * err
    C_disc = est.disconnected(loops)
    assert C_disc.shape == (Nt,) and np.all(np.isfinite(C_disc))


# ---- e. refusals -----------------------------------------------------------------------
def test_refusals(sm):
    Nx, Nt = 6, 10
    R = 2
    L = sm.Lattice(Nx, Nt)
    O = sm.Lattice(5, 9)
    B = sm.Lattice(8, 8, loopback=True)
    try:
        out = np.zeros(R * 3 * Nt * 4)
        # before a gauge upload
        assert sm.lib.sm_quark_loops(L.ctx, 0.0, TOL, MAX_ITER, 0, 1, 5, ptr(out), None) == SM_ERR_STATE
        E = filled(sm, L, Nx, Nt, [epm.gauge(sm, Nx, Nt, seed) for seed in epm.SEEDS[:R]])
        m = np.array(epm.MASSES[:R])
        sd = np.array(lm.NOISE_SEEDS[:R], dtype=np.uint64)

        def call(e=E.ens, m0=ptr(m), solver=0, nnoise=1, max_iter=MAX_ITER, seed=ptr(sd), o=ptr(out)):
            return sm.lib.sm_ens_quark_loops(e, m0, TOL, max_iter, solver, nnoise, seed, o, None)

        def works():
            for solver in (0, 1):
                assert call(solver=solver) == 0
                want = E.quark_loops(m, 1, sd.tolist(), solver=solver, tol=TOL, max_iter=MAX_ITER)[0]
                assert cbits(out[:R * Nt * 4].reshape(R, 1, Nt, 4), want)

        works()
        for kw in (dict(e=None), dict(m0=None), dict(seed=None), dict(o=None), dict(solver=2), dict(solver=-1),
                   dict(nnoise=0), dict(nnoise=-4), dict(max_iter=-1)):
            assert call(**kw) == SM_ERR_ARG, kw
            works()
        E.close()
        # a replica without a gauge field
        Eh = L.ensemble(2)
        Eh.upload_gauge(0, epm.as_complex(epm.gauge(sm, Nx, Nt, 5), Nx, Nt))
        assert call(e=Eh.ens) == SM_ERR_STATE
        Eh.fill_gauge(1, 3, 0.3)
        assert call(e=Eh.ens) == 0
        Eh.close()
        # the lone context's own refusals
        S = Nx * Nt
        U = epm.gauge(sm, Nx, Nt, 5)
        sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
        for nn in (0, -1):
            assert sm.lib.sm_quark_loops(L.ctx, 0.0, TOL, MAX_ITER, 0, nn, 5, ptr(out), None) == SM_ERR_ARG
            assert b"nnoise" in sm.lib.sm_last_error()
        assert sm.lib.sm_quark_loops(L.ctx, 0.0, TOL, MAX_ITER, 3, 1, 5, ptr(out), None) == SM_ERR_ARG
        assert sm.lib.sm_quark_loops(L.ctx, 0.0, TOL, -1, 0, 1, 5, ptr(out), None) == SM_ERR_ARG
        assert sm.lib.sm_quark_loops(L.ctx, 0.0, TOL, MAX_ITER, 0, 1, 5, None, None) == SM_ERR_ARG
        assert sm.lib.sm_quark_loops(L.ctx, 0.0, TOL, MAX_ITER, 0, 1, 5, ptr(out), None) == 0
        # solver 1 on an odd lattice: refused naming the checkerboard; solver 0 still works
        Uo = epm.gauge(sm, 5, 9, 5)
        sm.check(sm.lib.sm_upload_gauge(O.ctx, ptr(Uo[:90]), ptr(Uo[90:])))
        with pytest.raises(sm.SMError, match="checkerboard"):
            O.quark_loops(0.0, 2, 5, solver="even_odd")
        lo, ro = O.quark_loops(0.0, 2, 5, solver="plain", tol=TOL, max_iter=MAX_ITER)
        assert all(x.converged == 1 for x in ro) and np.all(np.isfinite(lo.view(np.float64)))
        Eo = filled(sm, O, 5, 9, [Uo])
        with pytest.raises(sm.SMError, match="checkerboard"):
            Eo.quark_loops([0.0], 2, [5], solver="even_odd")
        le, reo = Eo.quark_loops([0.0], 2, [5], solver="plain", tol=TOL, max_iter=MAX_ITER)
        Eo.close()
        assert cbits(le[0], lo) and report(reo[0]) == report(ro)
        # a loopback context
        Ub = epm.gauge(sm, 8, 8, 5)
        sm.check(sm.lib.sm_upload_gauge(B.ctx, ptr(Ub[:128]), ptr(Ub[128:])))
        with pytest.raises(sm.SMError, match="one-shard"):
            B.quark_loops(0.0, 2, 5)
    finally:
        L.close()
        O.close()
        B.close()
