"""The host model of the pure-gauge trajectory (tests/quenched_model.py), on the CPU.

Two things make the model fit to judge the device by:

* its generator is the library's: against sm_fill_spinor and sm_fill_gauge (the
  host generator of schwingermodel_amd/csrc/sm_fields.h, compiled C with glibc's
  log and sincos) the model's draws agree to 2 ulp;
* it is sharp: changing the momenta's stream, the site index, the trajectory
  key, the number of force evaluations, a half step into a full step or the step
  size each moves U more than 1000 times further than the tolerance the device
  is held to (test_quenched_gpu.py: 32 * delta_ref, delta_ref being the double
  model's distance from the same recurrence in extended precision).
"""
import numpy as np
import pytest

import quenched_model as qm
from conftest import ptr

import schwingermodel_amd as sm

lib = sm.lib
INV_SQRT2 = 0.70710678118654752440084436210485


def start_field(Nx, Nt, sigma=0.4242, seed=4321):
    S = Nx * Nt
    U = np.empty(4 * S)
    lib.sm_fill_gauge(seed, sigma, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
    return U.view(np.complex128).reshape(2, Nx, Nt).copy()


def within_ulps(got, ref, n):
    return np.abs(got - ref) <= n * np.spacing(np.abs(ref))


@pytest.mark.parametrize("Nx,Nt,seed", [(37, 130, 2024), (5, 9, 7), (64, 64, 0xFFFFFFFFFFFFFFF1)])
def test_generator_matches_library_spinor(Nx, Nt, seed):
    """sm_fill_spinor: plane mu = (g1 + i g2) / sqrt(2) of stream 4 + mu at index x*Nt + t."""
    S = Nx * Nt
    p = np.empty(4 * S)
    lib.sm_fill_spinor(seed, Nt, 0, Nx, 0, Nt, ptr(p[:2 * S]), ptr(p[2 * S:]))
    p = p.view(np.complex128).reshape(2, S)
    idx = np.arange(S, dtype=np.uint64)
    same = 0
    for mu in (0, 1):
        g1, g2 = qm.gauss2(seed, 4 + mu, idx)
        for got, ref in ((INV_SQRT2 * g1, p[mu].real), (INV_SQRT2 * g2, p[mu].imag)):
            assert within_ulps(got, ref, 2).all(), float((np.abs(got - ref) / np.spacing(np.abs(ref))).max())
            same += int(np.count_nonzero(got == ref))
    assert same >= 0.99 * 4 * S, same / (4 * S)   # the same draws, not merely close ones


def test_generator_matches_library_on_a_t_window():
    """The index is the GLOBAL site: rows [x0, x0+nx), columns [t0, t0+Wt) of 11 x 40."""
    Nt, x0, nx, t0, Wt = 40, 3, 5, 12, 9
    p = np.empty(4 * nx * Wt)
    lib.sm_fill_spinor(99, Nt, x0, nx, t0, Wt, ptr(p[:2 * nx * Wt]), ptr(p[2 * nx * Wt:]))
    p = p.view(np.complex128).reshape(2, nx, Wt)
    x, t = np.meshgrid(np.arange(x0, x0 + nx), np.arange(t0, t0 + Wt), indexing="ij")
    g1, g2 = qm.gauss2(99, 4, (x * Nt + t).ravel().astype(np.uint64))
    assert within_ulps(INV_SQRT2 * g1, p[0].real.ravel(), 2).all()
    assert within_ulps(INV_SQRT2 * g2, p[0].imag.ravel(), 2).all()


@pytest.mark.parametrize("sigma", [0.4242, -1.0], ids=["gauss", "hot"])
def test_generator_matches_library_gauge(sigma):
    """sm_fill_gauge: theta = sigma * g1 of stream pair mu (Gaussian), or
    pi (2 u - 1) with u of stream 16 + mu (hot); U = (cos theta, sin theta).
    The hot theta involves no transcendental, so the model's is the library's and
    each component is two roundings of one value: 2 ulp. The Gaussian theta
    itself may differ by 2 ulp, which moves a component by up to that much
    (|d cos|, |d sin| <= |d theta|) whatever the component's own size."""
    Nx, Nt, seed = 37, 130, 4321
    S = Nx * Nt
    U = start_field(Nx, Nt, sigma, seed).reshape(2, S)
    idx = np.arange(S, dtype=np.uint64)
    for mu in (0, 1):
        if sigma > 0:
            th = sigma * qm.gauss2(seed, mu, idx)[0]
            slack = 2 * np.spacing(np.abs(th))
        else:
            th = 3.141592653589793238462643383279 * (2.0 * qm.uniform(seed, 16 + mu, idx) - 1.0)
            slack = 0.0
        for got, ref in ((np.cos(th), U[mu].real), (np.sin(th), U[mu].imag)):
            assert (np.abs(got - ref) <= 2 * np.spacing(np.abs(ref)) + slack).all()
        # the angles themselves, where the components determine them well
        assert np.abs(np.angle(U[mu]) - th).max() <= 4 * np.spacing(np.pi)


def test_traj_seed_and_uniform_definition():
    """Scalar restatement in Python integers of the two keyed functions."""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed, traj in ((2024, 3), (0, 0), (M, M - 5)):
        want = mix(seed ^ mix(traj ^ 0x6A09E667F3BCC909))
        assert int(qm.traj_seed(seed, traj)[0]) == want
        k = mix((mix(seed ^ ((0xD1B54A32D192ED03 * (12 + 1)) & M)) + 77) & M)
        assert qm.uniform(seed, 12, 77)[0] == ((k >> 11) + 1) / 9007199254740992.0


DAMAGE = {
    "stream5": dict(stream=5),
    "index_tx": dict(index="tx"),
    "key_seed": dict(key="seed"),
    "force_evals_plus1": dict(force_evals=1),
    "force_evals_minus1": dict(force_evals=-1),
    "first_step_full": dict(first_full=True),
    "last_step_full": dict(last_full=True),
    "eps_tau_over_md_minus1": dict(eps_steps="md_steps-1"),
}


@pytest.fixture(scope="module")
def models(oracle):
    """Per case: the start field, the undamaged double model after the first
    trajectory, and allowed = 32 * delta_ref over the two trajectories (the
    largest tolerance the device comparison grants that case)."""
    force = qm.oracle_force(oracle)
    out = {}
    for case in qm.CASES:
        Nx, Nt, md, tau, beta = case
        U = start_field(Nx, Nt)
        d, fields = qm.delta_ref(U, qm.SEED, qm.TRAJS, md, tau, beta, force)
        out[case] = (U, fields[0], qm.ALLOWED_FACTOR * d[-1], d[-1])
    return out, force


@pytest.mark.parametrize("case", qm.CASES, ids=qm.CASE_IDS)
def test_delta_ref_is_rounding_sized(models, case):
    """delta_ref is the double model's rounding: a few 1e-16, and not zero."""
    d = models[0][case][3]
    print(f"delta_ref {case}: {d:.3e}")
    assert 1e-17 < d < 1e-14, d


@pytest.mark.parametrize("what", sorted(DAMAGE))
@pytest.mark.parametrize("case", qm.CASES, ids=qm.CASE_IDS)
def test_damaged_model_is_far_from_the_model(models, case, what):
    (U, good, allowed, _), force = models[0][case], models[1]
    Nx, Nt, md, tau, beta = case
    kw = dict(DAMAGE[what])
    if kw.get("eps_steps"):
        kw["eps_steps"] = md - 1
    bad = qm.trajectory(U, qm.SEED, qm.TRAJS[0], md, tau, beta, np.float64, force, **kw)
    dev = qm.max_component_deviation(bad, good)
    assert dev > 1000 * allowed, (dev, allowed)


def test_long_double_force_is_the_oracles_force(oracle):
    """The numpy force of the extended-precision run is Force_G: in double it
    meets the oracle's to rounding (three-link products, |F| <= 2 beta)."""
    U = start_field(37, 130)
    F = qm.gauge_force(U, 5.0)
    Fo = qm.oracle_force(oracle)(U, 5.0)
    assert np.abs(F - Fo).max() <= 64 * np.finfo(float).eps * 5.0
