"""The numpy models behind the fp32 CG pass's iterate tests (mixed_model.py;
no GPU): the np.roll operator is the oracle's, the fp32 model sits under its
own bound, and the bound rejects the stencil errors the GPU test is there to
catch -- each one, applied to the model's fp32 links, lands at least 10x over
it at k = 3."""
import numpy as np
import pytest

import mixed_model as mm

sm = pytest.importorskip("schwingermodel_amd")

M0 = -0.10


@pytest.mark.parametrize("shape", [(5, 9), (8, 8)], ids=["5x9", "8x8"])
def test_numpy_operator_is_the_oracles(oracle, shape):
    Nx, Nt = shape
    U, psi = mm.synthetic(sm, Nx, Nt)
    links = mm.signed_links(U, Nx, Nt)
    p = mm.to_planes(psi, Nx, Nt)
    ref = mm.oracle_ddag(oracle, Nx, Nt, U, psi, M0)
    got = mm.from_planes(mm.np_ddag(links, p, M0 + 2.0))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{Nx}x{Nt}: complex128 np.roll D D^dag against oracle_ddag: {err:.3e}")
    assert err <= 1e-14
    for dag in (0, 1):  # and each factor on its own (D D^dag alone cannot tell D from D^dag's order)
        S = Nx * Nt
        o = np.empty(4 * S)
        oracle.oracle_dirac(Nx, Nt, mm.ptr(U[:2 * S]), mm.ptr(U[2 * S:]), mm.ptr(psi[:2 * S]), mm.ptr(psi[2 * S:]),
                            mm.ptr(o[:2 * S]), mm.ptr(o[2 * S:]), M0, dag)
        g = mm.from_planes(mm.np_dirac(links, p, M0 + 2.0, dag))
        assert np.abs(g - o).max() / np.abs(o).max() <= 1e-14, dag


def flip_t_link(l32):
    l32[0][2, 1] *= -1  # an interior t-link with the boundary's sign


def rotate_x_link(l32):
    l32[1][1, 3] *= np.complex64(np.exp(1e-3j))


def sign_at_t0(l32):
    l32[0][:, -1] *= -1  # off where it belongs ...
    l32[0][:, 0] *= -1   # ... and on the links out of t = 0


MUTANTS = {"t_link_sign": flip_t_link, "x_link_1e-3_rad": rotate_x_link, "sign_at_t0": sign_at_t0}


@pytest.fixture(scope="module", params=[(6, 57), (13, 225)], ids=["6x57", "13x225"])
def case(request, oracle):
    Nx, Nt = request.param
    U, psi = mm.synthetic(sm, Nx, Nt)
    K = 12
    ref = mm.cg_iterates_fp64(oracle, Nx, Nt, U, psi, M0, K)
    model = mm.cg_iterates_fp32_model(Nx, Nt, U, psi, M0, K)
    return Nx, Nt, U, psi, ref, model


def test_model_sits_under_its_bound(case):
    Nx, Nt, U, psi, ref, model = case
    dev = [mm.deviation(m, r, psi) for m, r in zip(model, ref)]
    b = mm.bound(model, ref, psi)
    print(f"{Nx}x{Nt}: model deviation k = 1..12 " + " ".join(f"{d:.2e}" for d in dev) + f"; bound {b:.3e}")
    assert max(dev) <= b / 8


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_bound_rejects_mutant(case, name):
    Nx, Nt, U, psi, ref, model = case
    b = mm.bound(model, ref, psi)
    bad = mm.cg_iterates_fp32_model(Nx, Nt, U, psi, M0, 3, mutate=MUTANTS[name])
    dev = mm.deviation(bad[2], ref[2], psi)
    print(f"{Nx}x{Nt} {name}: deviation at k = 3 {dev:.3e}, bound {b:.3e}, ratio {dev / b:.1f}")
    assert dev >= 10 * b
