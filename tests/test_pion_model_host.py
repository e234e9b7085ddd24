"""The pion model (pion_model.py) and its end-to-end bound can tell a wrong
correlator from a right one (CPU only): a dropped spin component and a lost
antiperiodic sign land far outside the bound, and a cold configuration gives
a correlator symmetric about the source time.
"""
import numpy as np
import pytest

import mixed_model as mm
import pion_model as pm

import schwingermodel_amd as sm

M0 = -0.10
SHAPES = [(8, 8), (16, 16)]


def sources(Nx, Nt):
    return [(0, 0), (Nx - 1, Nt - 1), (Nx // 2, Nt // 3)]


_CACHE = {}


@pytest.fixture(scope="module")
def model(oracle):
    def get(shape):
        if shape not in _CACHE:
            Nx, Nt = shape
            U, _ = mm.synthetic(sm, Nx, Nt)
            ys = pm.solutions(oracle, Nx, Nt, U, M0, sources(Nx, Nt))
            C = pm.correlator(oracle, Nx, Nt, U, M0, ys)
            B = pm.bound(oracle, Nx, Nt, U, M0, ys)
            for a in (U, C, B):
                a.setflags(write=False)
            _CACHE[shape] = (U, ys, C, B)
        return _CACHE[shape]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=["8x8", "16x16"])
def test_model_operator_is_the_oracles(oracle, model, shape):
    """The numpy D^dagger the sign variant is built from reproduces the oracle's C within the bound."""
    Nx, Nt = shape
    U, ys, C, B = model(shape)
    Cn = pm.correlator(oracle, Nx, Nt, U, M0, ys, ddagger=lambda y: pm.numpy_ddagger(Nx, Nt, U, y, M0))
    assert np.all(B > 0.0) and np.all(C > 0.0)
    assert np.all(np.abs(Cn - C) <= B)


@pytest.mark.parametrize("shape", SHAPES, ids=["8x8", "16x16"])
def test_dropped_spin_is_far_outside_the_bound(oracle, model, shape):
    Nx, Nt = shape
    U, ys, C, B = model(shape)
    Cv = pm.correlator(oracle, Nx, Nt, U, M0, ys, spins=(0,))
    factor = (np.abs(Cv - C) / B).max()
    print(f"PION MODEL {Nx}x{Nt}: alpha = 1 source dropped: {factor:.3e} x the bound")
    assert factor >= 100.0


@pytest.mark.parametrize("shape", SHAPES, ids=["8x8", "16x16"])
def test_lost_antiperiodic_sign_is_far_outside_the_bound(oracle, model, shape):
    Nx, Nt = shape
    U, ys, C, B = model(shape)
    Cv = pm.correlator(oracle, Nx, Nt, U, M0, ys,
                       ddagger=lambda y: pm.numpy_ddagger(Nx, Nt, U, y, M0, antiperiodic=False))
    factor = (np.abs(Cv - C) / B).max()
    print(f"PION MODEL {Nx}x{Nt}: antiperiodic sign removed from the apply: {factor:.3e} x the bound")
    assert factor >= 100.0


@pytest.mark.parametrize("shape", SHAPES, ids=["8x8", "16x16"])
def test_cold_correlator_is_symmetric_about_the_source_time(oracle, shape):
    Nx, Nt = shape
    S = Nx * Nt
    U = np.zeros(4 * S)
    U[0::2] = 1.0  # cold: every link 1
    src = sources(Nx, Nt)
    ys = pm.solutions(oracle, Nx, Nt, U, M0, src)
    C = pm.correlator(oracle, Nx, Nt, U, M0, ys)
    B = pm.bound(oracle, Nx, Nt, U, M0, ys)
    for s, (_, t0) in enumerate(src):
        fwd = np.array([C[s, (t0 + d) % Nt] for d in range(Nt)])
        bwd = np.array([C[s, (t0 - d) % Nt] for d in range(Nt)])
        allow = np.array([max(B[s, (t0 + d) % Nt], B[s, (t0 - d) % Nt]) for d in range(Nt)])
        assert np.all(np.abs(fwd - bwd) <= allow), (s, np.abs(fwd - bwd).max())
        assert fwd[0] == C[s].max()  # and it peaks at the source
