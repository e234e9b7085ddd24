"""Mixed-precision CG (sm_cg_precision = 1): fp32 inner iterations held to the
fp64 stop test by reliable updates (schwingermodel_amd/csrc/sm_cgmp.cpp,
sm_cgsp.hip).

The mixed solution is not the reference's iterate sequence, so nothing here
compares x to 1e-12. What a mixed solve owes is the stop test itself, checked
with the CPU oracle in fp64: rho = ||phi - D D^dag x|| / ||phi|| < tol. Two
vectors x, x' that both pass it satisfy, by the triangle inequality,
    ||D D^dag (x - x')|| <= (rho + rho') ||phi||,
which is the comparison against the reference's ref_cgx (and against the fp64
solve of the same context); the 1 % on top covers the fp64 rounding of the
check itself. Iteration totals are printed beside the reference's cg_iters
and bounded by 1.25 cg_iters + 20: the reliable-update scheme stays within
1.10 in a numpy model of this operator, a restarted defect correction (which
the bound is there to reject) needs 1.23-1.70.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, fixture_names, load_fixture, opts_env, ptr

pytestmark = pytest.mark.gpu

TOL, MAXIT = 1e-10, 10000


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def ddag(oracle, Nx, Nt, U, v, m0):
    S = Nx * Nt
    tmp, out = np.empty(4 * S), np.empty(4 * S)
    oracle.oracle_ddag(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(v[:2 * S]), ptr(v[2 * S:]), ptr(tmp[:2 * S]),
                       ptr(tmp[2 * S:]), ptr(out[:2 * S]), ptr(out[2 * S:]), m0)
    return out


def relres(oracle, Nx, Nt, U, phi, x, m0):
    return np.linalg.norm(phi - ddag(oracle, Nx, Nt, U, x, m0)) / np.linalg.norm(phi)


def cg(sm, L, phi, m0, tol=TOL, max_iter=MAXIT):
    S = L.V
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, tol,
                          max_iter, ctypes.byref(res)))
    return res, L.last_cg_mixed, x


def upload(sm, L, U):
    S = L.V
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))


def synthetic(sm, Nx, Nt, sigma):
    S = Nx * Nt
    U, psi = np.empty(4 * S), np.empty(4 * S)
    sm.lib.sm_fill_gauge(4321, sigma, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
    sm.lib.sm_fill_spinor(5678, Nt, 0, Nx, 0, Nt, ptr(psi[:2 * S]), ptr(psi[2 * S:]))
    return U, psi


def check_solution(oracle, Nx, Nt, U, phi, m0, x, x_other, label):
    """The true-residual bound on x, and the triangle inequality against x_other
    (a vector that passes the same stop test). Returns (rho, rho_other)."""
    rho = relres(oracle, Nx, Nt, U, phi, x, m0)
    rho_o = relres(oracle, Nx, Nt, U, phi, x_other, m0)
    gap = np.linalg.norm(ddag(oracle, Nx, Nt, U, x - x_other, m0))
    lim = 1.01 * (rho + rho_o) * np.linalg.norm(phi)
    print(f"{label}: rho_mixed {rho:.3e} rho_other {rho_o:.3e} ||A(x - x')|| {gap:.3e} <= {lim:.3e}")
    assert rho < TOL, rho
    assert gap <= lim, (gap, lim)
    return rho, rho_o


# ---- 1. every golden fixture ------------------------------------------------
@pytest.mark.parametrize("name", fixture_names())
def test_fixture_meets_stop_test_and_iteration_bound(sm, oracle, name):
    meta, a = load_fixture(name)
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        assert L.cg_precision("mixed") == "mixed"
        res, info, x = cg(sm, L, a["psi"], m0)
    finally:
        L.close()
    print(f"{name}: mixed total {res.iterations} (inner {info.inner_iterations}, updates {info.reliable_updates}, "
          f"fp64 {info.fp64_iterations}) against cg_iters {meta['cg_iters']}")
    assert res.converged == 1 and info.used == 1 and info.fell_back == 0
    assert res.iterations == info.inner_iterations + info.fp64_iterations
    rho, rho_ref = check_solution(oracle, Nx, Nt, a["U"], a["psi"], m0, x, a["ref_cgx"], name)
    # the manifest's figure for the reference's x is the cross-check of this recomputation
    assert abs(rho_ref - meta["cg_true_relres"]) <= 1e-3 * meta["cg_true_relres"] + 1e-15
    assert abs(info.true_residual - rho) <= 1e-3 * rho + 1e-15
    assert res.iterations <= 1.25 * meta["cg_iters"] + 20, (res.iterations, meta["cg_iters"])


# ---- 2. several tiles in both directions, uneven edges -----------------------
@pytest.mark.parametrize("shape", [(96, 200), (130, 72)], ids=["96x200", "130x72"])
def test_multi_tile_shapes_against_fp64(sm, oracle, shape):
    Nx, Nt = shape
    m0 = -0.10
    U, psi = synthetic(sm, Nx, Nt, 0.3246)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        r64, i64, x64 = cg(sm, L, psi, m0)
        L.cg_precision("mixed")
        res, info, x = cg(sm, L, psi, m0)
    finally:
        L.close()
    print(f"{Nx}x{Nt}: mixed total {res.iterations} (updates {info.reliable_updates}) against fp64 {r64.iterations}")
    assert r64.converged == 1 and i64.used == 0
    assert res.converged == 1 and info.used == 1 and info.fell_back == 0
    check_solution(oracle, Nx, Nt, U, psi, m0, x, x64, f"{Nx}x{Nt}")
    assert res.iterations <= 1.25 * r64.iterations + 20, (res.iterations, r64.iterations)


# ---- 3. the default path is untouched ----------------------------------------
@pytest.mark.parametrize("name", ["l64x64_b5_m-0p06", "gen:256x256"])
def test_fp64_solve_unchanged_by_a_mixed_solve(sm, name):
    """fp64, mixed, fp64 on one context: the two fp64 solves are bitwise equal
    in x and iteration count (64^2: the stored-Ad pass; 256^2: the
    recompute-Ad pass), so no scalar, partial or direction buffer leaks."""
    if name.startswith("gen:"):
        Nx = Nt = 256
        m0 = -0.06
        U, psi = synthetic(sm, Nx, Nt, 0.2374)
    else:
        meta, a = load_fixture(name)
        Nx, Nt, m0, U, psi = meta["Nx"], meta["Nt"], meta["m0"], a["U"], a["psi"]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        assert L.last_cg_mixed.used == 0
        ra, ia, xa = cg(sm, L, psi, m0)
        assert ia.used == 0 and L.cg_precision() == "double"
        L.cg_precision("mixed")
        rm, im, xm = cg(sm, L, psi, m0)
        assert im.used == 1 and rm.converged == 1
        L.cg_precision("double")
        rb, ib, xb = cg(sm, L, psi, m0)
    finally:
        L.close()
    assert ib.used == 0
    assert ra.iterations == rb.iterations and ra.residual == rb.residual
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64))
    assert not np.array_equal(xa, xm)  # the mixed solve did run something else


# ---- 4. max_iter cut-off -------------------------------------------------------
@pytest.mark.parametrize("max_iter", [16, 17], ids=["stop_even", "stop_odd"])
def test_max_iter_cutoff(sm, oracle, max_iter):
    """Cut off after an even / odd number of fp32 passes: the count is exact,
    and x holds everything iterated so far (the fp32 correction folded in, its
    pending rows included), i.e. its fp64 residual is the reported one."""
    meta, a = load_fixture("l64x64_b5_m-0p06")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        L.cg_precision("mixed")
        res, info, x = cg(sm, L, a["psi"], m0, max_iter=max_iter)
        L.cg_precision("double")
        r64, _, x64 = cg(sm, L, a["psi"], m0, max_iter=max_iter)
    finally:
        L.close()
    assert res.converged == 0 and res.iterations == max_iter and info.used == 1
    assert np.all(np.isfinite(x))
    rho = relres(oracle, Nx, Nt, a["U"], a["psi"], x, m0)
    rho64 = relres(oracle, Nx, Nt, a["U"], a["psi"], x64, m0)
    print(f"max_iter {max_iter}: true relres mixed {rho:.6e} (reported {info.true_residual:.6e}), fp64 {rho64:.6e}")
    assert abs(rho - info.true_residual) <= 1e-6 * rho
    assert abs(res.residual - rho * res.phi_norm) <= 1e-6 * res.residual


# ---- 5. fallback ----------------------------------------------------------------
def test_forced_fallback_finishes_in_fp64(sm, oracle):
    meta, a = load_fixture("l32x48_b3_m-0p10")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    with opts_env(mp_force_fallback=1):
        L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, a["U"])
        L.cg_precision("mixed")
        res, info, x = cg(sm, L, a["psi"], m0)
    finally:
        L.close()
    print(f"fallback: inner {info.inner_iterations} updates {info.reliable_updates} fp64 {info.fp64_iterations}")
    assert res.converged == 1 and info.used == 1 and info.fell_back == 1
    assert info.reliable_updates == 1 and info.inner_iterations > 0 and info.fp64_iterations > 0
    assert res.iterations == info.inner_iterations + info.fp64_iterations
    check_solution(oracle, Nx, Nt, a["U"], a["psi"], m0, x, a["ref_cgx"], "fallback")


# ---- 6. sharded contexts refuse ---------------------------------------------------
def test_loopback_context_refuses_and_stays_fp64(sm):
    meta, a = load_fixture("l32x48_b3_m-0p10")
    L = sm.Lattice(meta["Nx"], meta["Nt"], loopback=True)
    try:
        upload(sm, L, a["U"])
        mode = ctypes.c_int(-1)
        assert sm.lib.sm_cg_precision(L.ctx, 1, ctypes.byref(mode)) == 1  # SM_ERR_ARG
        assert mode.value == 0
        assert sm.lib.sm_cg_precision(L.ctx, 2, None) == 1
        res, info, x = cg(sm, L, a["psi"], meta["m0"])
    finally:
        L.close()
    assert res.converged == 1 and info.used == 0
    assert abs(res.iterations - meta["cg_iters"]) <= max(1, meta["cg_iters"] // 100)
    assert np.linalg.norm(x - a["ref_cgx"]) / np.linalg.norm(a["ref_cgx"]) <= 1e-12


# ---- 7. HMC -----------------------------------------------------------------------
def test_hmc_trajectories_mixed_against_fp64(sm):
    """Three trajectories (32^2, beta 2, m0 0, 10 MD steps, tau 0.5) from the
    same start and seed in both modes: no CG failure, the same accept / reject
    decisions, and per trajectory |dH_mixed - dH_fp64| <= B, where B follows
    from the solves' residuals. With A = D D^dag, every solve of either mode
    returns x with ||phi - A x|| <= tol ||phi||, so dx = x - A^-1 phi has
    ||dx|| <= tol ||phi|| / lmin(A), and:
      (a) the fermion action <x, phi> is off by |<dx, phi>| = |<r, A^-1 phi>|
          <= tol ||phi|| ||x||; H_old and H_new, two modes: 4 tol ||phi|| ||x||;
      (b) a force error dF_k at MD step k moves H_new, to first order, by
          eps P_k . dF_k (H is conserved along the flow, so the tangent map
          drops out), and the bilinear force has ||dF|| <= 4 ||D|| ||x|| ||dx||
          (||dD/domega|| <= 1, two factors, real part of two terms); over the
          trajectory and two modes: 8 tau ||P|| ||D|| ||x|| tol ||phi|| / lmin.
    So B = tol ||phi|| ||x|| (4 + 8 tau ||P|| ||D|| / lmin), with ||D|| <= m0 + 4
    (Wilson's disc), ||P|| <= 1.5 sqrt(2 V) (unit Gaussian momenta, with room
    for the exchange with the potential), and ||phi||, ||x||, 1 / lmin measured
    in fp64 on the trajectory's starting configuration: phi = D chi for a
    Gaussian chi as the trajectory draws it, x = A^-1 phi, and 1 / lmin from
    three inverse iterations (a lower estimate, doubled). Worst case at every
    step, so B is loose; it is derived, not fitted.
    With p.even_odd = 1 the mode is ignored (the even-odd solver stays fp64)."""
    N, m0, beta, tau, steps = 32, 0.0, 2.0, 0.5, 10
    S = N * N
    ctx = {}
    for mode in ("double", "mixed"):
        ctx[mode] = sm.Lattice(N, N)
        sm.check(sm.lib.sm_fill_gauge_dev(ctx[mode].ctx, 77, 0.4242))
        ctx[mode].cg_precision(mode)
    H = sm.Lattice(N, N)  # helper: fp64 norms on the starting configurations
    rng = np.random.default_rng(5)
    try:
        p = sm.HMCParams(m0, beta, tau, steps, TOL, MAXIT, 2024, 0)
        for traj in range(3):
            U = np.empty(4 * S)
            sm.check(sm.lib.sm_download_gauge(ctx["double"].ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
            upload(sm, H, U)
            chi = rng.standard_normal(4 * S) / math.sqrt(2.0)
            phi = np.empty(4 * S)
            sm.check(sm.lib.sm_dirac(H.ctx, ptr(chi[:2 * S]), ptr(chi[2 * S:]), ptr(phi[:2 * S]), ptr(phi[2 * S:]),
                                     m0, 0))
            _, _, x = cg(sm, H, phi, m0, tol=1e-12)
            n_phi, n_x = np.linalg.norm(phi), np.linalg.norm(x)
            v, inv_l = x / n_x, 0.0
            for _ in range(3):
                _, _, w = cg(sm, H, v, m0, tol=1e-8)
                inv_l = max(inv_l, np.linalg.norm(w))
                v = w / np.linalg.norm(w)
            inv_l *= 2.0
            B = TOL * n_phi * n_x * (4 + 8 * tau * 1.5 * math.sqrt(2 * S) * (m0 + 4) * inv_l)
            out = {}
            for mode in ("double", "mixed"):
                r = sm.HMCResult()
                sm.check(sm.lib.sm_hmc_trajectory(ctx[mode].ctx, ctypes.byref(p), traj, ctypes.byref(r)))
                out[mode] = r
                assert r.cg_failures == 0, mode
                assert ctx[mode].last_cg_mixed.used == (1 if mode == "mixed" else 0)
            d = abs(out["mixed"].dH - out["double"].dH)
            print(f"traj {traj}: dH fp64 {out['double'].dH:.9e} mixed {out['mixed'].dH:.9e} |diff| {d:.3e} "
                  f"B {B:.3e} (||phi|| {n_phi:.3e} ||x|| {n_x:.3e} 1/lmin {inv_l:.3e}); CG iterations "
                  f"{out['double'].cg_iterations} / {out['mixed'].cg_iterations}")
            assert d <= B, (d, B)
            assert out["mixed"].accepted == out["double"].accepted
        # even-odd action: its own solver, fp64 whatever the mode
        E = sm.Lattice(N, N)
        try:
            sm.check(sm.lib.sm_fill_gauge_dev(E.ctx, 77, 0.4242))
            E.cg_precision("mixed")
            pe = sm.HMCParams(m0, beta, tau, steps, TOL, MAXIT, 2024, 1)
            r = sm.HMCResult()
            sm.check(sm.lib.sm_hmc_trajectory(E.ctx, ctypes.byref(pe), 0, ctypes.byref(r)))
            assert r.cg_failures == 0 and E.last_cg_mixed.used == 0
        finally:
            E.close()
    finally:
        for L in list(ctx.values()) + [H]:
            L.close()


# ---- 8. Python and shim --------------------------------------------------------------
def test_python_cg_precision_attribute(sm, oracle):
    meta, a = load_fixture("l32x48_b3_m-0p10")
    Nx, Nt, m0 = meta["Nx"], meta["Nt"], meta["m0"]
    S = Nx * Nt
    L = sm.init(Nx, Nt)
    cplx = lambda v: (v[:2 * S].view(np.complex128).copy(), v[2 * S:].view(np.complex128).copy())  # noqa: E731
    U, phi, x = sm.spinor.from_arrays(*cplx(a["U"])), sm.spinor.from_arrays(*cplx(a["psi"])), sm.spinor(S)
    old = sm.CG.precision
    try:
        sm.CG.precision = "mixed"
        assert sm.conjugate_gradient(U, phi, x, m0) == 1
        info = L.last_cg_mixed
        assert info.used == 1 and info.fell_back == 0 and L.cg_precision() == "mixed"
        xm = np.concatenate([x.mu0.view(np.float64), x.mu1.view(np.float64)])
        check_solution(oracle, Nx, Nt, a["U"], a["psi"], m0, xm, a["ref_cgx"], "python")
        assert L.last_cg.iterations <= 1.25 * meta["cg_iters"] + 20
        sm.CG.precision = "double"
        assert sm.conjugate_gradient(U, phi, x, m0) == 1
        assert L.last_cg_mixed.used == 0 and L.cg_precision() == "double"
        with pytest.raises(sm.SMError):
            L.cg_precision(7)
    finally:
        sm.CG.precision = old
        L.close()


def test_dropin_shim_mixed(tmp_path, oracle):
    """The reference's own fixture driver over the shim with
    SM_DROPIN_CG_PRECISION=mixed on one rank: its x meets the stop test."""
    exe = os.path.join(REPO, "oracle", "_ref", "sm_dropin_32x48")
    if not os.path.exists(exe):
        pytest.skip("drop-in binary not built (needs the reference sources at build time)")
    meta, a = load_fixture("l32x48_b3_m-0p10")
    for k in ("U", "psi", "chi"):
        a[k].tofile(tmp_path / f"{k}.bin")
    env = dict(os.environ, HOSTNAME=os.environ.get("HOSTNAME", "gpu-box"), SM_DROPIN_CG_PRECISION="mixed")
    r = subprocess.run([exe, "fixture", str(tmp_path), "1", "1", repr(meta["m0"]), "1e-10", "10000"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert '"cg_converged": 1' in r.stdout
    x = np.fromfile(tmp_path / "ref_cgx.bin", dtype=np.float64)
    assert not np.array_equal(x, a["ref_cgx"])  # the mixed solve ran, not the fp64 one
    check_solution(oracle, meta["Nx"], meta["Nt"], a["U"], a["psi"], meta["m0"], x, a["ref_cgx"], "shim")
