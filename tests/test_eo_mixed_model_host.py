"""The numpy models behind the mixed-precision even-odd CG's tests
(eo_mixed_model.py; no GPU): the np.roll Dhat is the oracle-composed one, the
fp32 model sits under its own bound, the bound rejects the stencil errors the
GPU iterate test is there to catch, and a model of the whole reliable-update
scheme on Dhat Dhat^dag gives the iteration cap the GPU tests use."""
import numpy as np
import pytest

import eo_mixed_model as em
import mixed_model as mm
from conftest import load_fixture

sm = pytest.importorskip("schwingermodel_amd")

M0 = -0.10


@pytest.mark.parametrize("shape", [(6, 10), (8, 8), (14, 24)], ids=["6x10", "8x8", "14x24"])
def test_numpy_dhat_is_the_oracle_composed_one(oracle, shape):
    Nx, Nt = shape
    U, psi = em.synthetic(sm, Nx, Nt)
    links = mm.signed_links(U, Nx, Nt)
    p = em.to_planes(em.even_part(psi, Nx, Nt), Nx, Nt)
    for dag in (0, 1):
        ref = em.oracle_dhat(oracle, Nx, Nt, U, psi, M0, dag)
        got = em.from_planes(em.np_dhat(links, p, M0 + 2.0, dag))
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{Nx}x{Nt} dagger {dag}: complex128 np.roll Dhat against the oracle-composed Dhat: {err:.3e}")
        assert err <= 1e-14
        assert np.all(em.to_planes(ref, Nx, Nt)[:, ~em.even_mask(Nx, Nt)] == 0.0)
    ref = em.oracle_dhatdhat(oracle, Nx, Nt, U, psi, M0)
    got = em.from_planes(em.np_dhatdhat(links, p, M0 + 2.0))
    assert np.abs(got - ref).max() / np.abs(ref).max() <= 1e-14


def lost_sign(l32):
    l32[0][:, -1] *= -1  # the antiperiodic sign of the hop out of t = Nt - 1 is gone


def sign_at_t0(l32):
    l32[0][:, -1] *= -1  # off where it belongs ...
    l32[0][:, 0] *= -1   # ... and on the links out of t = 0


def rotate_x_link(l32):
    l32[1][1, 3] *= np.complex64(np.exp(1e-3j))


MUTANTS = {"lost_antiperiodic_sign": lost_sign, "sign_at_t0": sign_at_t0, "x_link_1e-3_rad": rotate_x_link}


@pytest.fixture(scope="module", params=[(6, 10), (14, 24)], ids=["6x10", "14x24"])
def case(request, oracle):
    Nx, Nt = request.param
    U, psi = em.synthetic(sm, Nx, Nt)
    phi = em.even_part(psi, Nx, Nt)
    K = 12
    ref = em.cg_iterates_fp64(oracle, Nx, Nt, U, phi, M0, K)
    model = em.cg_iterates_fp32_model(Nx, Nt, U, phi, M0, K)
    return Nx, Nt, U, phi, ref, model


def test_model_sits_under_its_bound(case):
    Nx, Nt, U, phi, ref, model = case
    dev = [em.deviation(m, r, phi) for m, r in zip(model, ref)]
    b = em.bound(model, ref, phi)
    print(f"{Nx}x{Nt}: model deviation k = 1..12 " + " ".join(f"{d:.2e}" for d in dev) + f"; bound {b:.3e}")
    assert max(dev) <= b / 8


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_bound_rejects_mutant(case, name):
    Nx, Nt, U, phi, ref, model = case
    b = em.bound(model, ref, phi)
    bad = em.cg_iterates_fp32_model(Nx, Nt, U, phi, M0, 3, mutate=MUTANTS[name])
    dev = em.deviation(bad[2], ref[2], phi)
    print(f"{Nx}x{Nt} {name}: deviation at k = 3 {dev:.3e}, bound {b:.3e}, ratio {dev / b:.1f}")
    assert dev >= 10 * b


FIXTURES = ["l16x16_b2_m-0p19", "l32x48_b3_m-0p10", "l64x64_b5_m-0p06"]
CAP = 1.25  # the GPU tests' iteration cap (test_eo_cg_mixed_gpu.py)


def test_reliable_updates_cost_few_iterations():
    """The whole scheme of sm_eomp.cpp in numpy on Dhat Dhat^dag, tol 1e-10:
    iterations over plain fp64 CG, R for the reliable updates that keep the
    search direction (the worst fixture), and the same for a defect correction
    that restarts every segment. R < 1.25 is the cap the GPU tests use."""
    tol = 1e-10
    worst = {True: 0.0, False: 0.0}
    for name in FIXTURES:
        meta, a = load_fixture(name)
        Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
        n64 = em.fp64_cg_count(Nx, Nt, a["U"], a["psi"], m0, tol)
        line = f"{name}: fp64 {n64}"
        for keep in (True, False):
            n, ups, rho = em.solve_model(Nx, Nt, a["U"], a["psi"], m0, tol, keep_direction=keep)
            assert rho < tol
            worst[keep] = max(worst[keep], n / n64)
            line += f"; {'reliable updates' if keep else 'restarted'} {n} ({ups} updates, ratio {n / n64:.3f})"
        print(line)
    print(f"R (reliable updates, worst) {worst[True]:.3f}; restarted defect correction (worst) {worst[False]:.3f}")
    assert worst[True] < CAP
