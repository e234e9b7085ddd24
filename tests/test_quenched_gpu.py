"""sm_quenched_trajectory against the host model of tests/quenched_model.py.

The pure-gauge trajectory makes the evolved field bench.py --full times the CG
on. Its momenta are drawn on the device (draw_momenta_kernel: stream 6, keyed by
sm_traj_seed(seed, traj), indexed by the global site x*Nt + t) and its leapfrog
is the host's loop in sm_md.cpp; until now only the ensemble was compared with
the lone chain, and both share that device code.

Against the model. Each case runs two consecutive trajectories from one start
field; after each, every component of the downloaded U must be within
    allowed = 32 * delta_ref
of the double model's, delta_ref being the largest component deviation between
the model in double and the same recurrence in numpy.longdouble up to that
trajectory: computed here on the CPU, the code under test has no part in it. The
device's log and sincos and the C library's may each be 1-2 ulp off the exact
value, there are md_steps + 1 link updates and one Box-Muller draw per link, and
delta_ref already carries what the force feeds back, hence 32. delta_ref is
3e-16 to 7e-15 for these cases, allowed 1e-14 to 2e-13; a wrong stream, index,
key, step count or step size moves links by 1e-3 and more
(test_quenched_model_host.py).

Measured on an MI355X (ROCm 7.2), deviation / allowed after the first and the
second trajectory (deviation, delta_ref):
    6x10   md 10: 0.0080 (1.1e-16, 4.3e-16)   0.0175 (4.4e-16, 7.9e-16)
    5x9    md 3:  0.0028 (2.8e-17, 3.1e-16)   0.0077 (1.1e-16, 4.5e-16)
    16x16  md 2:  0.0176 (1.7e-16, 3.0e-16)  0.0171 (2.2e-16, 4.1e-16)
    37x130 md 10: 0.0190 (8.6e-16, 1.4e-15)   0.0060 (1.3e-15, 6.8e-15)
The worst ratio, 0.019, is recorded in DESIGN.md section 6: the device is closer
to the double model than the double model is to the extended-precision one.

Bitwise: the same (seed, trajectory) on a fresh context reproduces the field, a
different trajectory number does not, and an RCCL loopback context (ghost links
re-exchanged after every link update, draws keyed by the global site) gives the
one-shard context's bits. And the link codes the recompute-Ad CG caches are
rebuilt after a quenched trajectory.
"""
import ctypes

import numpy as np
import pytest

import quenched_model as qm
from conftest import bits_equal, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def start_field(sm, Nx, Nt, sigma=0.4242, seed=4321):
    S = Nx * Nt
    U = np.empty(4 * S)
    sm.lib.sm_fill_gauge(seed, sigma, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
    return U.view(np.complex128).reshape(2, Nx, Nt).copy()


def params(sm, md, tau, beta, seed=qm.SEED):
    return sm.HMCParams(m0=0.0, beta=beta, tau=tau, md_steps=md, cg_tol=1e-10, cg_max_iter=10000, seed=seed,
                        even_odd=0)


def upload(sm, L, U):
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[0]), ptr(U[1])))


def download(sm, L, Nx, Nt):
    U = np.empty((2, Nx, Nt), dtype=np.complex128)
    sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(U[0]), ptr(U[1])))
    return U


def evolve(sm, Nx, Nt, U, p, trajs, loopback=False):
    """The fields after each of the consecutive trajectories on a fresh context."""
    L = sm.Lattice(Nx, Nt, loopback=loopback)
    out = []
    try:
        upload(sm, L, U)
        for traj in trajs:
            sm.check(sm.lib.sm_quenched_trajectory(L.ctx, ctypes.byref(p), traj))
            out.append(download(sm, L, Nx, Nt))
    finally:
        L.close()
    return out


@pytest.mark.parametrize("case", qm.CASES, ids=qm.CASE_IDS)
def test_quenched_trajectory_matches_host_model(sm, oracle, case):
    Nx, Nt, md, tau, beta = case
    S = Nx * Nt
    U = start_field(sm, Nx, Nt)
    deltas, model = qm.delta_ref(U, qm.SEED, qm.TRAJS, md, tau, beta, qm.oracle_force(oracle))
    p = params(sm, md, tau, beta)
    L = sm.Lattice(Nx, Nt)
    ratios, sums = [], []
    try:
        upload(sm, L, U)
        for i, traj in enumerate(qm.TRAJS):
            sm.check(sm.lib.sm_quenched_trajectory(L.ctx, ctypes.byref(p), traj))
            got = download(sm, L, Nx, Nt)
            allowed = qm.ALLOWED_FACTOR * deltas[i]
            dev = qm.max_component_deviation(got, model[i])
            ratios.append(dev / allowed)
            print(f"quenched {Nx}x{Nt} md {md} traj {traj}: deviation {dev:.3e}, delta_ref {deltas[i]:.3e}, "
                  f"allowed {allowed:.3e}, ratio {dev / allowed:.4f}")
            sp, act = ctypes.c_double(), ctypes.c_double()
            sm.check(sm.lib.sm_plaquette(L.ctx, beta, ctypes.byref(sp), ctypes.byref(act), None))
            rsp, ract = ctypes.c_double(), ctypes.c_double()
            oracle.oracle_plaquette_sums(Nx, Nt, ptr(got[0]), ptr(got[1]), beta, ctypes.byref(rsp),
                                         ctypes.byref(ract))
            sums.append(((sp.value, rsp.value), (act.value, ract.value)))
    finally:
        L.close()
    assert max(ratios) <= 1.0, ratios
    # the trajectory did move the field, by far more than the tolerance
    assert qm.max_component_deviation(model[0], U) > 1e-3
    for pair in sums:
        for got, ref in pair:
            assert abs(got - ref) <= 1e-13 * max(1.0, abs(ref)) + 1e-13 * S, (got, ref)


@pytest.mark.parametrize("case", [qm.CASES[1], qm.CASES[3]], ids=[qm.CASE_IDS[1], qm.CASE_IDS[3]])
def test_quenched_trajectory_bitwise_properties(sm, case):
    Nx, Nt, md, tau, beta = case
    U = start_field(sm, Nx, Nt)
    p = params(sm, md, tau, beta)
    first = evolve(sm, Nx, Nt, U, p, qm.TRAJS)
    again = evolve(sm, Nx, Nt, U, p, qm.TRAJS)
    loop = evolve(sm, Nx, Nt, U, p, qm.TRAJS, loopback=True)
    other = evolve(sm, Nx, Nt, U, p, (qm.TRAJS[0] + 1,))
    other_seed = evolve(sm, Nx, Nt, U, params(sm, md, tau, beta, seed=qm.SEED + 1), qm.TRAJS[:1])
    for i in range(len(qm.TRAJS)):
        assert bits_equal(first[i].view(np.float64), again[i].view(np.float64)), i
        assert bits_equal(first[i].view(np.float64), loop[i].view(np.float64)), i
    assert qm.max_component_deviation(first[0], other[0]) > 1e-3
    assert qm.max_component_deviation(first[0], other_seed[0]) > 1e-3


def test_link_codes_rebuilt_after_quenched_trajectory(sm, oracle):
    """The pattern of test_link_codes_after_hmc_trajectories: the recompute-Ad CG
    caches link codes of U; a solve on the start field builds them, the quenched
    trajectory must invalidate them, and the next solve (no upload in between) is
    bitwise the complex-link solve and meets oracle_cg on the downloaded field."""
    Nx, Nt, m0 = 96, 64, -0.05
    S = Nx * Nt
    U = start_field(sm, Nx, Nt)
    psi = np.empty(4 * S)
    sm.lib.sm_fill_spinor(13, Nt, 0, Nx, 0, Nt, ptr(psi[:2 * S]), ptr(psi[2 * S:]))
    L = sm.Lattice(Nx, Nt)
    c = L.ctx

    def solve(on):
        sm.check(sm.lib.sm_cg_link_codes(c, on, None))
        x, res = np.empty(4 * S), sm.CGResult()
        sm.check(sm.lib.sm_cg(c, ptr(psi[:2 * S]), ptr(psi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, 1e-10,
                              10000, ctypes.byref(res)))
        use = ctypes.c_int(-1)
        sm.check(sm.lib.sm_cg_link_codes(c, -1, ctypes.byref(use)))
        return x, res, use.value

    try:
        upload(sm, L, U)
        sm.check(sm.lib.sm_tune_cg(c, 5, 0))
        x_start, _, use = solve(1)
        assert use == 1
        p = params(sm, 10, 1.0, 2.0)
        sm.check(sm.lib.sm_quenched_trajectory(c, ctypes.byref(p), 0))
        x_on, res_on, use = solve(1)     # stale codes would solve on the start field
        assert use == 1 and res_on.converged == 1
        err, bad = ctypes.c_double(-1.0), ctypes.c_long(-1)
        sm.check(sm.lib.sm_link_code_check(c, None, ctypes.byref(err), ctypes.byref(bad)))
        assert bad.value == 0 and err.value == 0.0, (bad.value, err.value)
        x_off, res_off, use_off = solve(0)
        assert use_off == 0
        cur = download(sm, L, Nx, Nt)
    finally:
        sm.check(sm.lib.sm_cg_link_codes(c, 1, None))
        L.close()
    assert res_on.iterations == res_off.iterations
    assert bits_equal(x_on, x_off)
    assert np.linalg.norm(x_on - x_start) / np.linalg.norm(x_start) > 1e-3
    xr = np.empty(4 * S)
    it, e = ctypes.c_int(), ctypes.c_double()
    assert oracle.oracle_cg(Nx, Nt, ptr(cur[0]), ptr(cur[1]), ptr(psi[:2 * S]), ptr(psi[2 * S:]), ptr(xr[:2 * S]),
                            ptr(xr[2 * S:]), m0, 1e-10, 10000, ctypes.byref(it), ctypes.byref(e)) == 1
    assert abs(res_on.iterations - it.value) <= max(1, it.value // 100), (res_on.iterations, it.value)
    assert np.linalg.norm(x_on - xr) / np.linalg.norm(xr) <= 1e-12
