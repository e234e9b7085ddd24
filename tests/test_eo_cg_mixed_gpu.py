"""Mixed-precision even-odd CG (sm_eo_cg_precision = 1): fp32 inner iterations
of the one-pass even-odd kernel held to the fp64 stop test by reliable updates
(schwingermodel_amd/csrc/sm_eomp.cpp, sm_eosp.hip).

The reference of every check is Dhat = m - (1/m) D_eo D_oe composed from the
CPU oracle's oracle_dirac and parity masks (eo_mixed_model.py), never the
GPU's own fp64 even-odd path. The mixed solution is not the fp64 iterate
sequence, so nothing compares x to 1e-12. What a mixed solve owes is the stop
test itself, rho = ||phi_e - Dhat Dhat^dag x|| / ||phi_e|| < tol in fp64. Two
vectors x, x' that both pass it satisfy, by the triangle inequality,
    ||Dhat Dhat^dag (x - x')|| <= (rho + rho') ||phi_e||,
which is the comparison against the fp64 even-odd solve of the same context;
the 1 % on top covers the fp64 rounding of the check itself. Iteration totals
are bounded by 1.25 x the fp64 even-odd count + 20: the reliable-update scheme
stays within 1.09 in a numpy model of this operator, a restarted defect
correction (which the cap is there to reject) needs 1.48-1.99
(test_eo_mixed_model_host.py).
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import eo_mixed_model as em
from conftest import REPO, bits_equal, load_fixture, opts_env, ptr

pytestmark = pytest.mark.gpu

TOL, MAXIT = 1e-10, 10000
CAP = 1.25
SM_ERR_ARG = 1


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def eo_cg(sm, L, phi, m0, tol=TOL, max_iter=MAXIT):
    S = L.V
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_eo_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, tol,
                             max_iter, ctypes.byref(res)))
    return res, L.last_eo_cg_mixed, x


def cg(sm, L, phi, m0, tol=TOL, max_iter=MAXIT):
    S = L.V
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, tol,
                          max_iter, ctypes.byref(res)))
    return res, x


def upload(sm, L, U):
    S = L.V
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))


def relres(oracle, Nx, Nt, U, phi, x, m0):
    return np.linalg.norm(phi - em.oracle_dhatdhat(oracle, Nx, Nt, U, x, m0)) / np.linalg.norm(phi)


def check_solution(oracle, Nx, Nt, U, phi, m0, x, x_other, label):
    """The true-residual bound on x, and the triangle inequality against x_other
    (a vector that passes the same stop test). Returns (rho, rho_other)."""
    rho = relres(oracle, Nx, Nt, U, phi, x, m0)
    rho_o = relres(oracle, Nx, Nt, U, phi, x_other, m0)
    gap = np.linalg.norm(em.oracle_dhatdhat(oracle, Nx, Nt, U, x - x_other, m0))
    lim = 1.01 * (rho + rho_o) * np.linalg.norm(phi)
    print(f"{label}: rho_mixed {rho:.3e} rho_fp64 {rho_o:.3e} ||A(x - x')|| {gap:.3e} <= {lim:.3e}")
    assert rho < TOL, rho
    assert gap <= lim, (gap, lim)
    return rho, rho_o


def fp64_then_mixed(sm, oracle, Nx, Nt, U, phi, m0, label):
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        r64, i64, x64 = eo_cg(sm, L, phi, m0)
        assert L.eo_cg_precision("mixed") == "mixed"
        res, info, x = eo_cg(sm, L, phi, m0)
    finally:
        L.close()
    print(f"{label}: mixed total {res.iterations} (inner {info.inner_iterations}, updates {info.reliable_updates}, "
          f"fp64 {info.fp64_iterations}) against the fp64 even-odd solve's {r64.iterations}")
    assert r64.converged == 1 and i64.used == 0
    assert res.converged == 1 and info.used == 1 and info.fell_back == 0
    assert res.iterations == info.inner_iterations + info.fp64_iterations
    rho, _ = check_solution(oracle, Nx, Nt, U, phi, m0, x, x64, label)
    assert abs(info.true_residual - rho) <= 1e-3 * rho + 1e-15, (info.true_residual, rho)
    assert res.iterations <= CAP * r64.iterations + 20, (res.iterations, r64.iterations)


# ---- 1. golden fixtures ---------------------------------------------------------
FIXTURES = ["l8x8_hot_m0p2", "l16x16_b2_m-0p19", "l32x48_b3_m-0p10", "l64x64_b5_m-0p06"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_meets_stop_test_and_iteration_bound(sm, oracle, name):
    meta, a = load_fixture(name)
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    fp64_then_mixed(sm, oracle, Nx, Nt, a["U"], em.even_part(a["psi"], Nx, Nt), m0, name)


# ---- 2. several tiles in both directions, uneven edges -----------------------------
@pytest.mark.parametrize("shape", [(96, 200), (130, 72)], ids=["96x200", "130x72"])
def test_multi_tile_shapes(sm, oracle, shape):
    Nx, Nt = shape
    U, psi = em.synthetic(sm, Nx, Nt)
    fp64_then_mixed(sm, oracle, Nx, Nt, U, em.even_part(psi, Nx, Nt), -0.10, f"{Nx}x{Nt}")


# ---- 3. separation --------------------------------------------------------------------
def _case(sm, name):
    if name == "gen:256x120":
        Nx, Nt, m0 = 256, 120, -0.06
        U, psi = em.synthetic(sm, Nx, Nt, sigma=0.2374)
    else:
        meta, a = load_fixture(name)
        Nx, Nt, m0, U, psi = meta["Nx"], meta["Nt"], meta["m0"], a["U"], a["psi"]
    return Nx, Nt, m0, U, psi, em.even_part(psi, Nx, Nt)


@pytest.mark.parametrize("name", ["l64x64_b5_m-0p06", "gen:256x120"])
def test_fp64_solves_unchanged_by_a_mixed_even_odd_solve(sm, name):
    """fp64, mixed, fp64 sm_eo_cg on one context: the two fp64 solves are
    bitwise equal in x and iteration count. The same bracket with sm_cg in
    fp64 and in mixed precision around a mixed even-odd solve. Either switch
    alone leaves the other solver's *_mixed_last.used at 0."""
    Nx, Nt, m0, U, psi, phi = _case(sm, name)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        assert L.last_eo_cg_mixed.used == 0 and L.eo_cg_precision() == "double"
        ra, ia, xa = eo_cg(sm, L, phi, m0)
        assert ia.used == 0
        fa, ya = cg(sm, L, psi, m0)                       # full operator, fp64
        assert L.last_cg_mixed.used == 0
        L.eo_cg_precision("mixed")                        # only the even-odd switch
        assert L.cg_precision() == "double"
        rm, im, xm = eo_cg(sm, L, phi, m0)
        assert im.used == 1 and rm.converged == 1
        fb, yb = cg(sm, L, psi, m0)                       # still fp64, after a mixed even-odd solve
        assert L.last_cg_mixed.used == 0
        L.eo_cg_precision("double")
        rb, ib, xb = eo_cg(sm, L, phi, m0)
        assert ib.used == 0
        L.cg_precision("mixed")                           # only the full operator's switch
        assert L.eo_cg_precision() == "double"
        fc, yc = cg(sm, L, psi, m0)
        assert L.last_cg_mixed.used == 1
        rc, ic, xc = eo_cg(sm, L, phi, m0)                # fp64 even-odd under cg_precision = mixed
        assert ic.used == 0
        L.eo_cg_precision("mixed")                        # both
        rd, idd, xd = eo_cg(sm, L, phi, m0)
        assert idd.used == 1
        fd, yd = cg(sm, L, psi, m0)                       # mixed full solve after a mixed even-odd one
        assert L.last_cg_mixed.used == 1 and L.last_eo_cg_mixed.used == 1
    finally:
        L.close()
    for r in (ra, rb, rc):
        assert r.converged == 1
    assert ra.iterations == rb.iterations == rc.iterations and ra.residual == rb.residual == rc.residual
    assert bits_equal(xa, xb) and bits_equal(xa, xc)
    assert not np.array_equal(xa, xm)                     # the mixed solve did run something else
    assert rm.iterations == rd.iterations and bits_equal(xm, xd)
    assert fa.iterations == fb.iterations and fa.residual == fb.residual and bits_equal(ya, yb)
    assert fc.iterations == fd.iterations and fc.residual == fd.residual and bits_equal(yc, yd)


# ---- 4. max_iter cut-off -----------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [16, 17], ids=["stop_even", "stop_odd"])
def test_max_iter_cutoff(sm, oracle, max_iter):
    """Cut off after an even / odd number of fp32 passes: the count is exact,
    and x holds everything iterated so far (the fp32 correction folded in, the
    alpha d pending after an odd pass included): its fp64 residual is the
    reported one."""
    meta, a = load_fixture("l64x64_b5_m-0p06")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    phi = em.even_part(a["psi"], Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        L.eo_cg_precision("mixed")
        res, info, x = eo_cg(sm, L, phi, m0, max_iter=max_iter)
    finally:
        L.close()
    assert res.converged == 0 and res.iterations == max_iter and info.used == 1
    assert info.inner_iterations == max_iter and info.fell_back == 0
    assert np.all(np.isfinite(x))
    rho = relres(oracle, Nx, Nt, a["U"], phi, x, m0)
    print(f"max_iter {max_iter}: true relres {rho:.6e} (reported {info.true_residual:.6e})")
    assert abs(rho - info.true_residual) <= 1e-6 * rho
    assert abs(res.residual - rho * res.phi_norm) <= 1e-6 * res.residual


# ---- 5. fallback ----------------------------------------------------------------------------
def test_forced_fallback_finishes_in_fp64(sm, oracle):
    meta, a = load_fixture("l32x48_b3_m-0p10")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    phi = em.even_part(a["psi"], Nx, Nt)
    with opts_env(mp_force_fallback=1):
        L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        L.eo_cg_precision("mixed")
        res, info, x = eo_cg(sm, L, phi, m0)
    finally:
        L.close()
    rho = relres(oracle, Nx, Nt, a["U"], phi, x, m0)
    print(f"fallback: inner {info.inner_iterations} updates {info.reliable_updates} fp64 {info.fp64_iterations} "
          f"rho {rho:.3e}")
    assert res.converged == 1 and info.used == 1 and info.fell_back == 1
    assert info.reliable_updates == 1 and info.inner_iterations > 0 and info.fp64_iterations > 0
    assert res.iterations == info.inner_iterations + info.fp64_iterations
    assert rho < TOL


@pytest.mark.parametrize("s", [127, -160], ids=["overflow", "flush_to_zero"])
def test_fp32_range_exit_finishes_in_fp64(sm, oracle, s):
    """(float) r overflows (phi 2^127) or is zero (2^-160): the first pass's
    scalars are not finite, the driver discards y and the fp64 even-odd solver
    finishes."""
    meta, a = load_fixture("l32x48_b3_m-0p10")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    phi = np.ldexp(em.even_part(a["psi"], Nx, Nt), s)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        L.eo_cg_precision("mixed")
        res, info, x = eo_cg(sm, L, phi, m0)
    finally:
        L.close()
    assert np.all(np.isfinite(x))
    rho = relres(oracle, Nx, Nt, a["U"], phi, x, m0)
    print(f"2^{s}: converged {res.converged} iterations {res.iterations} inner {info.inner_iterations} "
          f"fp64 {info.fp64_iterations} relres {rho:.3e}")
    assert res.converged == 1 and info.used == 1 and info.fell_back == 1
    assert info.inner_iterations <= 1
    assert rho < TOL


class _Hip:
    """hipMalloc / hipMemcpy through the HIP runtime the library itself links."""

    def __init__(self):
        self.rt = ctypes.CDLL("libamdhip64.so.7")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), nbytes) == 0
        return p

    def upload(self, a):
        p = self.alloc(a.nbytes)
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p

    def download(self, p, a):
        assert self.rt.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost

    def free(self, p):
        self.rt.hipFree(p)


@pytest.mark.parametrize("mode", ["double", "mixed"])
def test_device_entry_point_equals_the_host_one(sm, mode):
    """sm_eo_cg_dev on device-resident fields is sm_eo_cg without the transfers: bitwise the same x and counts."""
    meta, a = load_fixture("l32x48_b3_m-0p10")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    phi = a["psi"]  # the odd sites are ignored
    hip = _Hip()
    L = sm.Lattice(Nx, Nt)
    dphi = dx = None
    try:
        upload(sm, L, a["U"])
        L.eo_cg_precision(mode)
        res, info, x = eo_cg(sm, L, phi, m0)
        dphi, dx = hip.upload(phi), hip.alloc(phi.nbytes)
        rd = sm.CGResult()
        sm.check(sm.lib.sm_eo_cg_dev(L.ctx, dphi, dx, m0, TOL, MAXIT, ctypes.byref(rd)))
        infod = L.last_eo_cg_mixed
        xd = np.empty_like(x)
        hip.download(dx, xd)
    finally:
        L.close()
        for p in (dphi, dx):
            if p is not None:
                hip.free(p)
    assert res.converged == 1 and rd.converged == 1
    assert (rd.iterations, rd.residual, infod.used, infod.reliable_updates) == \
        (res.iterations, res.residual, info.used, info.reliable_updates)
    assert info.used == (1 if mode == "mixed" else 0)
    assert bits_equal(x, xd)
    assert np.all(em.to_planes(xd, Nx, Nt)[:, ~em.even_mask(Nx, Nt)] == 0.0)


# ---- 6. sharded contexts refuse ------------------------------------------------------------------
def test_loopback_context_refuses_and_stays_fp64(sm):
    meta, a = load_fixture("l32x48_b3_m-0p10")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    phi = em.even_part(a["psi"], Nx, Nt)
    L = sm.Lattice(Nx, Nt, loopback=True)
    O = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        upload(sm, O, a["U"])
        mode = ctypes.c_int(-1)
        assert sm.lib.sm_eo_cg_precision(L.ctx, 1, ctypes.byref(mode)) == SM_ERR_ARG
        assert mode.value == 0
        assert sm.lib.sm_eo_cg_precision(L.ctx, 2, None) == SM_ERR_ARG
        assert sm.lib.sm_eo_cg_precision(O.ctx, 2, ctypes.byref(mode)) == SM_ERR_ARG and mode.value == 0
        res, info, x = eo_cg(sm, L, phi, m0)
        ro, io, xo = eo_cg(sm, O, phi, m0)
    finally:
        L.close()
        O.close()
    assert res.converged == 1 and info.used == 0 and ro.converged == 1 and io.used == 0
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) <= 1e-10


# ---- 7. the fp32 links follow the gauge field --------------------------------------------------------
def test_fp32_links_follow_an_uploaded_gauge_field(sm):
    """Mixed solve on U_a, upload U_b, mixed solve: bitwise the solve of a
    fresh context given U_b (stale fp32 links would still converge -- every
    reliable update is fp64 -- but along other iterates)."""
    Nx, Nt, m0 = 32, 48, -0.10
    Ua, psi = em.synthetic(sm, Nx, Nt)
    Ub, _ = em.synthetic(sm, Nx, Nt, sigma=0.41, gauge_seed=1234)
    phi = em.even_part(psi, Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    F = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, Ua)
        L.eo_cg_precision("mixed")
        r1, i1, x1 = eo_cg(sm, L, phi, m0)
        upload(sm, L, Ub)
        r2, i2, x2 = eo_cg(sm, L, phi, m0)
        upload(sm, F, Ub)
        F.eo_cg_precision("mixed")
        rf, jf, xf = eo_cg(sm, F, phi, m0)
    finally:
        L.close()
        F.close()
    assert r1.converged == 1 and r2.converged == 1 and i1.used == 1 and i2.used == 1 and jf.used == 1
    assert (r2.iterations, i2.reliable_updates, i2.fell_back) == (rf.iterations, jf.reliable_updates, jf.fell_back)
    assert bits_equal(x2, xf), np.abs(x2 - xf).max()
    assert not np.array_equal(x1, x2)


# ---- 8. HMC ---------------------------------------------------------------------------------------------
def test_hmc_trajectories_mixed_against_fp64(sm):
    """Three even-odd trajectories (32^2, beta 2, m0 0, 10 MD steps, tau 0.5)
    from the same start and seed, fp64 against mixed: no CG failure, the same
    accept / reject decisions, and per trajectory |dH_mixed - dH_fp64| <= B,
    where B follows from the solves' residuals as in
    test_cg_mixed_gpu.py::test_hmc_trajectories_mixed_against_fp64, with Dhat
    in place of D. With A = Dhat Dhat^dag, every solve of either mode returns x
    with ||phi - A x|| <= tol ||phi||, so dx = x - A^-1 phi has
    ||dx|| <= tol ||phi|| / lmin(A), and:
      (a) the fermion action <x, phi> is off by |<r, A^-1 phi>| <= tol ||phi||
          ||x||; H_old and H_new, two modes: 4 tol ||phi|| ||x||;
      (b) a force error dF_k at MD step k moves H_new, to first order, by
          eps P_k . dF_k. The force is the bilinear -2 Re(l^dag dD r) with
          l = (X, -(1/m) (D^dag)_oe X), r = (Y, -(1/m) D_oe Y), Y = Dhat^dag X:
          the hopping blocks have norm <= 2, so ||l|| <= (1 + 2/m) ||X|| and
          ||r|| <= (1 + 2/m) ||Dhat|| ||X||, and with ||dD/domega|| <= 1
          ||dF|| <= 4 (1 + 2/m)^2 ||Dhat|| ||x|| ||dx||; over the trajectory
          and two modes: 8 tau ||P|| (1 + 2/m)^2 ||Dhat|| ||x|| tol ||phi|| / lmin.
    So B = tol ||phi|| ||x|| (4 + 8 tau ||P|| (1 + 2/m)^2 ||Dhat|| / lmin), with
    ||Dhat|| <= m + 4/m, ||P|| <= 1.5 sqrt(2 V) (unit Gaussian momenta, with
    room for the exchange with the potential), and ||phi||, ||x||, 1 / lmin
    measured in fp64 on the trajectory's starting configuration: phi = Dhat
    chi_e for a Gaussian chi, x = A^-1 phi, 1 / lmin from three inverse
    iterations (a lower estimate, doubled). Worst case at every step, so B is
    loose; it is derived, not fitted."""
    N, m0, beta, tau, steps = 32, 0.0, 2.0, 0.5, 10
    S, m = N * N, m0 + 2.0
    ctx = {}
    for mode in ("double", "mixed"):
        ctx[mode] = sm.Lattice(N, N)
        sm.check(sm.lib.sm_fill_gauge_dev(ctx[mode].ctx, 77, 0.4242))
        ctx[mode].eo_cg_precision(mode)
    H = sm.Lattice(N, N)  # helper: fp64 norms on the starting configurations
    rng = np.random.default_rng(5)
    try:
        p = sm.HMCParams(m0, beta, tau, steps, TOL, MAXIT, 2024, 1)
        for traj in range(3):
            U = np.empty(4 * S)
            sm.check(sm.lib.sm_download_gauge(ctx["double"].ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
            upload(sm, H, U)
            chi = em.even_part(rng.standard_normal(4 * S) / math.sqrt(2.0), N, N)
            phi = np.empty(4 * S)
            sm.check(sm.lib.sm_eo_dhat(H.ctx, 0, ptr(chi[:2 * S]), ptr(chi[2 * S:]), ptr(phi[:2 * S]),
                                       ptr(phi[2 * S:]), m0))
            _, _, x = eo_cg(sm, H, phi, m0, tol=1e-12)
            n_phi, n_x = np.linalg.norm(phi), np.linalg.norm(x)
            v, inv_l = x / n_x, 0.0
            for _ in range(3):
                _, _, w = eo_cg(sm, H, v, m0, tol=1e-8)
                inv_l = max(inv_l, np.linalg.norm(w))
                v = w / np.linalg.norm(w)
            inv_l *= 2.0
            B = TOL * n_phi * n_x * (4 + 8 * tau * 1.5 * math.sqrt(2 * S) * (1 + 2 / m) ** 2 * (m + 4 / m) * inv_l)
            out = {}
            for mode in ("double", "mixed"):
                r = sm.HMCResult()
                sm.check(sm.lib.sm_hmc_trajectory(ctx[mode].ctx, ctypes.byref(p), traj, ctypes.byref(r)))
                out[mode] = r
                assert r.cg_failures == 0, mode
                assert ctx[mode].last_eo_cg_mixed.used == (1 if mode == "mixed" else 0)
                assert ctx[mode].last_cg_mixed.used == 0
            d = abs(out["mixed"].dH - out["double"].dH)
            print(f"traj {traj}: dH fp64 {out['double'].dH:.9e} mixed {out['mixed'].dH:.9e} |diff| {d:.3e} "
                  f"B {B:.3e} (||phi|| {n_phi:.3e} ||x|| {n_x:.3e} 1/lmin {inv_l:.3e}); CG iterations "
                  f"{out['double'].cg_iterations} / {out['mixed'].cg_iterations}")
            assert d <= B, (d, B)
            assert out["mixed"].accepted == out["double"].accepted
    finally:
        for L in list(ctx.values()) + [H]:
            L.close()


# ---- 9. Python -----------------------------------------------------------------------------------------------
def test_python_eo_cg_precision_attribute(sm):
    L = sm.Lattice(16, 16)
    try:
        assert L.eo_cg_precision() == "double" and L.last_eo_cg_mixed.used == 0
        assert L.eo_cg_precision("mixed") == "mixed" and L.eo_cg_precision() == "mixed"
        assert L.cg_precision() == "double"
        assert L.eo_cg_precision(0) == "double"
        assert L.eo_cg_precision(1) == "mixed"
        with pytest.raises(sm.SMError):
            L.eo_cg_precision(7)
        assert L.eo_cg_precision() == "mixed"  # a refused mode changes nothing
        with pytest.raises(ValueError):
            L.eo_cg_precision("single")
        assert L.eo_cg_precision("double") == "double"
    finally:
        L.close()


# ---- 10. sm_hmc ---------------------------------------------------------------------------------------------------
def test_sm_hmc_eo_cg_precision(tmp_path):
    exe = os.path.join(REPO, "schwingermodel_amd", "sm_hmc")
    if not os.path.exists(exe):
        pytest.skip("schwingermodel_amd/sm_hmc not built (build_cli needs an MPI)")
    params = "1\n1\n0.1\n6\n0.5\n2\n2\n3\n1\n0\n"
    env = dict(os.environ, HOSTNAME="box", SM_HMC_EO_CG_PRECISION="mixed")
    r = subprocess.run([exe, "16", "16", "77", "--even-odd"], input=params, capture_output=True, text=True,
                       cwd=tmp_path, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Acceptance rate:" in r.stdout
    r = subprocess.run([exe, "16", "16", "77"], input=params, capture_output=True, text=True, cwd=tmp_path, env=env,
                       timeout=300)
    assert r.returncode != 0
    assert "SM_HMC_EO_CG_PRECISION=mixed needs --even-odd" in r.stderr, r.stderr[-2000:]
