"""The lazily allocated workspaces through their whole life on one context and one
ensemble: first use, kept while it fits, regrown for a larger request, used
again for a smaller one, and freed at destruction (csrc/sm_buf.h's BufGroup
owns every one of them).

One context per shape runs every solver and measurement that allocates at first
use, in one sequence with growing and shrinking sizes; every result must be
bitwise that of a fresh context that made only that call. The same for an
ensemble of R = 3 against a fresh ensemble on a fresh context. Then both are
destroyed, and a second pair is created and destroyed without a call in between.

Allocation failures are not provoked here: that would take a shared card's
memory. tools/buf_host_check.cpp (tests/test_capi_host.py) covers those paths.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal, ptr

pytestmark = pytest.mark.gpu

TOL, MAXIT, M0 = 1e-10, 10000, 0.1
R = 3


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def fields_of(s):
    return tuple(getattr(s, name) for name, _ in s._fields_)


def same(a, b):
    """Bitwise: arrays by their bits, ctypes structs field by field, containers element by element."""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and bits_equal(
            np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))
    if isinstance(a, ctypes.Structure):
        return same(fields_of(a), fields_of(b))
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    return a == b


def structs(obj):
    """Every ctypes struct inside a result."""
    if isinstance(obj, ctypes.Structure):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from structs(o)


def gauge(sm, Nx, Nt, seed=4321, sigma=0.3):
    U = np.empty((2, Nx * Nt), dtype=np.complex128)
    sm.lib.sm_fill_gauge(seed, sigma, Nt, 0, Nx, 0, Nt, ptr(U[0]), ptr(U[1]))
    return U


def sources(sm, Nx, Nt, K):
    phi = np.empty((K, 2, Nx * Nt), dtype=np.complex128)
    for k in range(K):
        sm.lib.sm_fill_spinor(100 + k, Nt, 0, Nx, 0, Nt, ptr(phi[k, 0]), ptr(phi[k, 1]))
    return phi


def upload(sm, L, U):
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[0]), ptr(U[1])))


def download(sm, L):
    U = np.empty((2, L.V), dtype=np.complex128)
    sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(U[0]), ptr(U[1])))
    return U


def one_solve(sm, L, fn, phi):
    x = np.empty_like(phi)
    res = sm.CGResult()
    sm.check(fn(L.ctx, ptr(phi[0]), ptr(phi[1]), ptr(x[0]), ptr(x[1]), M0, TOL, MAXIT, ctypes.byref(res)))
    return x, res


def trajectory(sm, L, even_odd):
    prm = sm.HMCParams(M0, 2.0, 0.5, 4, TOL, MAXIT, 11, even_odd)
    res = sm.HMCResult()
    sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(prm), 0, ctypes.byref(res)))
    return res, download(sm, L)


def context_calls(sm, Nx, Nt):
    """(label, call(L)) in the order the sequence context makes them. The calls that
    change the context's gauge field, the two trajectories, come last; before them
    every call sees the uploaded field."""
    phi = sources(sm, Nx, Nt, 5)
    src = [(1, 2), (Nx - 1, Nt - 3)]
    calls = []

    def add(label, fn):
        calls.append((label, fn))

    for K in (2, 5, 3):
        add(f"cg_batch K={K}", lambda L, K=K: L.cg_batch(phi[:K], M0, TOL, MAXIT))
    for K in (2, 5, 3):
        add(f"eo_cg_batch K={K}", lambda L, K=K: L.eo_cg_batch(phi[:K], M0, TOL, MAXIT))

    def mixed_batch(L, K):
        assert L.cg_batch_precision("mixed") == "mixed"
        try:
            out = L.cg_batch(phi[:K], M0, TOL, MAXIT)
            return out, [fields_of(i) for i in L.last_cg_batch_mixed]
        finally:
            L.cg_batch_precision("double")

    for K in (2, 5):
        add(f"mixed cg_batch K={K}", lambda L, K=K: mixed_batch(L, K))

    def mixed_cg(L):
        assert L.cg_precision("mixed") == "mixed"
        try:
            return one_solve(sm, L, sm.lib.sm_cg, phi[0]), fields_of(L.last_cg_mixed)
        finally:
            L.cg_precision("double")

    def mixed_eo(L):
        assert L.eo_cg_precision("mixed") == "mixed"
        try:
            return one_solve(sm, L, sm.lib.sm_eo_cg, phi[1]), fields_of(L.last_eo_cg_mixed)
        finally:
            L.eo_cg_precision("double")

    add("mixed sm_cg", mixed_cg)
    add("mixed sm_eo_cg", mixed_eo)

    def pion(L, solver, n):
        L.pion_solver(solver)
        try:
            return L.pion_correlator(M0, src[:n], TOL, MAXIT)
        finally:
            L.pion_solver("plain")

    for n in (1, 2):
        for solver in ("plain", "even_odd"):
            add(f"pion {solver} nsrc={n}", lambda L, s=solver, n=n: pion(L, s, n))
    for points in (2, 5, 2):
        add(f"flow points={points}", lambda L, p=points: tuple(L.wilson_flow(0.02, p - 1, 1, return_field=True)))
    for nnoise in (2, 5):
        for solver in ("plain", "even_odd"):
            add(f"loops {solver} nnoise={nnoise}", lambda L, s=solver, n=nnoise: L.quark_loops(M0, n, 77, s, TOL, MAXIT))
    return calls


def ensemble_calls(Nx, Nt):
    m0s = [M0, M0 + 0.05, M0 + 0.1]
    src = [(1, 2), (Nx - 1, Nt - 3)]
    calls = []
    for n in (1, 2):
        for solver in ("plain", "even_odd"):
            calls.append((f"ens pion {solver} nsrc={n}",
                          lambda E, s=solver, n=n: E.pion_correlator(m0s, src[:n], s, TOL, MAXIT)))
    for points in (2, 5, 2):
        calls.append((f"ens flow points={points}",
                      lambda E, p=points: tuple(E.wilson_flow(0.02, p - 1, 1, return_field=True))))
    for nnoise in (2, 5):
        for solver in ("plain", "even_odd"):
            calls.append((f"ens loops {solver} nnoise={nnoise}",
                          lambda E, s=solver, n=nnoise: E.quark_loops(m0s, n, [5, 6, 7], s, TOL, MAXIT)))
    return calls, m0s


def new_ensemble(L):
    E = L.ensemble(R)
    for r in range(R):
        E.fill_gauge(r, 900 + r, 0.3)
    return E


def ens_trajectory(sm, E, m0s):
    prm = [sm.HMCParams(m0s[r], 2.0 + 0.5 * r, 0.5, 4, TOL, MAXIT, 21 + r, 1) for r in range(R)]
    return E.trajectory(prm, 0), [E.download_gauge(r) for r in range(R)]


@pytest.mark.parametrize("shape", [(8, 8), (40, 24)], ids=["8x8", "40x24"])
def test_sequence_on_one_context_equals_fresh_contexts(sm, shape):
    Nx, Nt = shape
    U = gauge(sm, Nx, Nt)
    differ = []

    def compare(label, got, want):
        ok = same(got, want)
        for s in structs(got):  # the comparison is of real solves: every one converged, no trajectory lost a solve
            if isinstance(s, sm.CGResult):
                assert s.converged == 1 and s.iterations > 0, (label, fields_of(s))
            if isinstance(s, sm.HMCResult):
                assert s.cg_failures == 0 and s.cg_iterations > 0 and np.isfinite(s.dH), (label, fields_of(s))
        print(f"{Nx}x{Nt} {label}: {'bitwise equal' if ok else 'DIFFERS'}")
        if not ok:
            differ.append(label)

    def fresh(call, field=U):
        L = sm.Lattice(Nx, Nt)
        try:
            upload(sm, L, field)
            return call(L)
        finally:
            L.close()

    def fresh_ens(call):
        L = sm.Lattice(Nx, Nt)
        try:
            E = new_ensemble(L)
            try:
                return call(E)
            finally:
                E.close()
        finally:
            L.close()

    L = sm.Lattice(Nx, Nt)
    E = None
    try:
        upload(sm, L, U)
        for label, call in context_calls(sm, Nx, Nt):
            compare(label, call(L), fresh(call))
        got = trajectory(sm, L, 0)
        compare("HMC trajectory", got, fresh(lambda F: trajectory(sm, F, 0)))
        U1 = got[1]  # the field the even-odd trajectory starts from
        compare("even-odd HMC trajectory", trajectory(sm, L, 1), fresh(lambda F: trajectory(sm, F, 1), U1))

        E = new_ensemble(L)
        calls, m0s = ensemble_calls(Nx, Nt)
        for label, call in calls:
            compare(label, call(E), fresh_ens(call))
        compare("ens even-odd trajectory", ens_trajectory(sm, E, m0s), fresh_ens(lambda F: ens_trajectory(sm, F, m0s)))
    finally:
        if E is not None:
            E.close()
        L.close()
    # a second pair, created and destroyed without a call in between
    L = sm.Lattice(Nx, Nt)
    E = L.ensemble(R)
    E.close()
    L.close()
    assert not differ, differ
