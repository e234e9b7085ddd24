"""Numpy model of the pion correlator from point sources (test helper), built on
the oracle: per source s and spin a, y_a = oracle_cg(unit vector at the source
in plane a), S_a = oracle_dirac(dagger = 1) y_a = D^-1 phi, and
    C[s, t] = sum_x sum_a (|S_a,0(x,t)|^2 + |S_a,1(x,t)|^2).

The end-to-end allowance of the GPU tests is computed here, from the model
alone: the solver is held to 1e-12 relative to the reference's iterates
(test_cg_batch_gpu.py a), so each oracle_cg solution is perturbed by a random
vector of relative norm 1e-12 and the largest change of every slice of C over
16 draws is what such an error may do to C; the tests allow 8x that.

Fields are the library's: 4 S doubles, plane 0 then plane 1, each (Nx, Nt)
row-major (t fastest), interleaved complex.
"""
import ctypes

import numpy as np

import mixed_model as mm
from conftest import ptr

TOL, MAX_ITER = 1e-10, 10000
SOLVER_BAR = 1e-12
DRAWS = 16
MARGIN = 8.0


def point_source(Nx, Nt, x, t, plane):
    p = np.zeros(4 * Nx * Nt)
    p[2 * (plane * Nx * Nt + x * Nt + t)] = 1.0
    return p


def solve(oracle, Nx, Nt, U, phi, m0):
    S = Nx * Nt
    y = np.empty(4 * S)
    it, err = ctypes.c_int(), ctypes.c_double()
    conv = oracle.oracle_cg(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(y[:2 * S]),
                            ptr(y[2 * S:]), m0, TOL, MAX_ITER, ctypes.byref(it), ctypes.byref(err))
    assert conv == 1
    return y


def oracle_ddagger(oracle, Nx, Nt, U, y, m0):
    """D^dagger y through the oracle."""
    S = Nx * Nt
    out = np.empty(4 * S)
    oracle.oracle_dirac(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(y[:2 * S]), ptr(y[2 * S:]), ptr(out[:2 * S]),
                        ptr(out[2 * S:]), m0, 1)
    return out


def numpy_ddagger(Nx, Nt, U, y, m0, antiperiodic=True):
    """D^dagger y with the model's own numpy operator (mixed_model.np_dirac);
    antiperiodic = False drops the t-boundary sign of the apply."""
    links = mm.signed_links(U, Nx, Nt) if antiperiodic else [u.copy() for u in mm.to_planes(U, Nx, Nt)]
    return mm.from_planes(mm.np_dirac(links, mm.to_planes(y, Nx, Nt), m0 + 2.0, 1))


def slice_sums(S_list, Nx, Nt):
    """C[t] = sum_x sum over the given S fields and both planes of |S|^2."""
    C = np.zeros(Nt)
    for S in S_list:
        c = mm.to_planes(S, Nx, Nt)
        C += (c.real ** 2 + c.imag ** 2).sum(axis=(0, 1))
    return C


def solutions(oracle, Nx, Nt, U, m0, sources):
    """[[y_0, y_1] per source]: the oracle's solves of the point sources."""
    return [[solve(oracle, Nx, Nt, U, point_source(Nx, Nt, x, t, a), m0) for a in (0, 1)] for x, t in sources]


def correlator(oracle, Nx, Nt, U, m0, ys, spins=(0, 1), ddagger=None):
    """C[nsrc, Nt] from the solutions ys; spins / ddagger: the damaged variants of the host test."""
    apply = ddagger or (lambda y: oracle_ddagger(oracle, Nx, Nt, U, y, m0))
    return np.stack([slice_sums([apply(y[a]) for a in spins], Nx, Nt) for y in ys])


def allowance(oracle, Nx, Nt, U, m0, ys, seed=20261019):
    """Per source and slice: the largest |change of C| over DRAWS random
    perturbations of relative norm SOLVER_BAR of every solution."""
    rng = np.random.default_rng(seed)
    C0 = correlator(oracle, Nx, Nt, U, m0, ys)
    worst = np.zeros_like(C0)
    for _ in range(DRAWS):
        pert = []
        for y in ys:
            row = []
            for v in y:
                e = rng.standard_normal(v.size)
                row.append(v + e * (SOLVER_BAR * np.linalg.norm(v) / np.linalg.norm(e)))
            pert.append(row)
        worst = np.maximum(worst, np.abs(correlator(oracle, Nx, Nt, U, m0, pert) - C0))
    return worst


def bound(oracle, Nx, Nt, U, m0, ys):
    return MARGIN * allowance(oracle, Nx, Nt, U, m0, ys)
