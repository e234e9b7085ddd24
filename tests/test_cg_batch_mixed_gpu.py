"""The mixed-precision batched CG (sm_cg_batch_precision = 1: sm_cgbatchsp.hip,
sm_cgbatchmp.cpp): fp32 passes for K columns per launch, fp64 reliable updates
per column.

a. iterates against textbook fp64 CG on the oracle's operator, within 8x the
   numpy fp32 model's own deviation, at the batch's tile edges;  b. whole
   solves whose columns stop at different counts (idling);  c. a column's bits
   do not depend on K, its position, its neighbours or the tile height;
d. the fp64 batch, the other solvers and the ensemble do not notice;
e. gauge changes need no call;  f. the cut-off;  g. the forced fallback;
h. host and device entry points;  i. refusals;  j. Python;  k. the correlator.
The reference is the CPU oracle and the numpy models, never the GPU's own fp64
batch except where b, d and k say so.
"""
import ctypes
import math

import numpy as np
import pytest

import mixed_model as mm
from conftest import bits_equal, load_fixture, opts_env, ptr

pytestmark = pytest.mark.gpu

M0 = -0.10
TOL, MAXIT = 1e-10, 10000
KS = (1, 2, 3, 4, 5, 6, 7, 12)
KMAX = max(KS)
SM_ERR_ARG = 1


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def upload(sm, L, U):
    S = L.V
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))


def spinor(sm, Nx, Nt, seed):
    S = Nx * Nt
    p = np.empty(4 * S)
    sm.lib.sm_fill_spinor(seed, Nt, 0, Nx, 0, Nt, ptr(p[:2 * S]), ptr(p[2 * S:]))
    return p


def point(Nx, Nt, x, t, plane):
    p = np.zeros(4 * Nx * Nt)
    p[2 * (plane * Nx * Nt + x * Nt + t)] = 1.0
    return p


def infos(sm, L, K):
    out = (sm.CGMixedInfo * K)()
    sm.check(sm.lib.sm_cg_batch_mixed_last(L.ctx, K, out))
    return list(out)


def batch(sm, L, cols, tol=TOL, max_iter=MAXIT, m0=M0):
    """sm_cg_batch on the columns (4 S doubles each): (x[K, 4S], results, infos)."""
    K = len(cols)
    phi = np.ascontiguousarray(np.stack(cols))
    x = np.full_like(phi, np.nan)
    res = (sm.CGResult * K)()
    sm.check(sm.lib.sm_cg_batch(L.ctx, K, ptr(phi), ptr(x), m0, tol, max_iter, res))
    return x, list(res), infos(sm, L, K)


def rtuple(r):
    return (r.converged, r.iterations, np.float64(r.residual).view(np.uint64), np.float64(r.phi_norm).view(np.uint64))


def ituple(i):
    return (i.used, i.inner_iterations, i.reliable_updates, i.fp64_iterations, i.fell_back,
            np.float64(i.true_residual).view(np.uint64))


def same(a, b, ia, ib):
    """Column ia of batch result a is bitwise column ib of b: x, sm_cg_result and sm_cg_mixed_info."""
    return (bits_equal(a[0][ia], b[0][ib]) and rtuple(a[1][ia]) == rtuple(b[1][ib])
            and ituple(a[2][ia]) == ituple(b[2][ib]))


def relres(oracle, Nx, Nt, U, phi, x, m0=M0):
    return np.linalg.norm(phi - mm.oracle_ddag(oracle, Nx, Nt, U, x, m0)) / np.linalg.norm(phi)


def oracle_inverse(oracle, Nx, Nt, U, v):
    S = Nx * Nt
    x = np.empty(4 * S)
    it, err = ctypes.c_int(), ctypes.c_double()
    assert oracle.oracle_cg(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(v[:2 * S]), ptr(v[2 * S:]), ptr(x[:2 * S]),
                            ptr(x[2 * S:]), M0, 1e-12, MAXIT, ctypes.byref(it), ctypes.byref(err)) == 1
    return x


def columns_a(sm, Nx, Nt):
    return [spinor(sm, Nx, Nt, 5678), spinor(sm, Nx, Nt, 91011), point(Nx, Nt, Nx // 2, Nt - 1, 1)]


def columns_b(sm, oracle, Nx, Nt, U):
    """Five unlike columns: a random one, a point source, a random one scaled by
    2^40, (D D^dag)^-1 r and (D D^dag)^-2 r (heavy on the low modes: they stop
    at other counts)."""
    inv = oracle_inverse(oracle, Nx, Nt, U, spinor(sm, Nx, Nt, 31))
    return [spinor(sm, Nx, Nt, 5709), point(Nx, Nt, 3 % Nx, 6 % Nt, 1), spinor(sm, Nx, Nt, 808) * 2.0 ** 40, inv,
            oracle_inverse(oracle, Nx, Nt, U, inv)]


# ---- a. iterates -------------------------------------------------------------
# The fp64 batch's tile edges (test_cg_batch_gpu.py lists what each shape is for);
# the fp32 pass keeps that geometry.
SHAPES = [(4, 2), (5, 9), (3, 60), (6, 61), (7, 62), (7, 121), (130, 72), (130, 241), (515, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_iterates_match_fp64_cg(sm, oracle, shape):
    """A mixed batched solve cut off at max_iter = k (tol 0) returns per column
    x_k = phi + (the fp32 correction, folded): compared per site with textbook
    fp64 CG on the oracle's operator within mm.bound() of that column's own
    numpy fp32 model, which is computed from the model and never the kernel."""
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    refs = [mm.cg_iterates_fp64(oracle, Nx, Nt, U, phi, M0, KMAX) for phi in cols]
    bounds = [mm.bound(mm.cg_iterates_fp32_model(Nx, Nt, U, phi, M0, KMAX), ref, phi) for phi, ref in zip(cols, refs)]
    L = sm.Lattice(Nx, Nt)
    worst = [0.0] * len(cols)
    try:
        upload(sm, L, U)
        assert L.cg_batch_precision("mixed") == "mixed"
        for k in KS:
            x, res, info = batch(sm, L, cols, 0.0, k)
            for b, phi in enumerate(cols):
                assert res[b].iterations == k and res[b].converged == 0, (k, b, res[b].iterations, res[b].converged)
                assert info[b].used == 1 and info[b].fell_back == 0, (k, b, info[b].used, info[b].fell_back)
                assert np.all(np.isfinite(x[b])), (k, b)
                dev = mm.deviation(x[b], refs[b][k - 1], phi)
                worst[b] = max(worst[b], dev)
                print(f"BATCH MIXED ITERATES {Nx}x{Nt} k {k} column {b}: deviation {dev:.3e} bound {bounds[b]:.3e}")
                assert dev <= bounds[b], (k, b, dev, bounds[b])
    finally:
        L.close()
    print(f"BATCH MIXED ITERATES {Nx}x{Nt}: worst {[f'{w:.2e}' for w in worst]} bounds {[f'{w:.2e}' for w in bounds]}")


# ---- b. whole solves ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16), (32, 48), (96, 200), (130, 72)], ids=["16x16", "32x48", "96x200", "130x72"])
def test_whole_solves(sm, oracle, shape):
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    five = Nx * Nt <= 32 * 48
    cols = columns_b(sm, oracle, Nx, Nt, U) if five else columns_a(sm, Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        x64, r64, i64 = batch(sm, L, cols)
        assert all(i.used == 0 for i in i64)
        L.cg_batch_precision("mixed")
        x, res, info = batch(sm, L, cols)
    finally:
        L.close()
    its = []
    for b, phi in enumerate(cols):
        rho, rho64 = relres(oracle, Nx, Nt, U, phi, x[b]), relres(oracle, Nx, Nt, U, phi, x64[b])
        gap = np.linalg.norm(mm.oracle_ddag(oracle, Nx, Nt, U, x[b] - x64[b], M0))
        lim = 1.01 * (rho + rho64) * np.linalg.norm(phi)
        print(f"BATCH MIXED SOLVE {Nx}x{Nt} column {b}: iterations {res[b].iterations} (inner "
              f"{info[b].inner_iterations}, updates {info[b].reliable_updates}, fp64 {info[b].fp64_iterations}) against "
              f"{r64[b].iterations}; rho {rho:.3e} rho64 {rho64:.3e} gap {gap:.3e} <= {lim:.3e}")
        assert res[b].converged == 1 and r64[b].converged == 1, b
        assert info[b].used == 1 and info[b].fell_back == 0, b
        assert rho < TOL, (b, rho)
        assert gap <= lim, (b, gap, lim)
        assert abs(info[b].true_residual - rho) <= 1e-3 * rho, (b, info[b].true_residual, rho)
        assert abs(res[b].residual - rho * res[b].phi_norm) <= 1e-3 * res[b].residual, b
        assert info[b].reliable_updates >= 1, b
        assert res[b].iterations == info[b].inner_iterations + info[b].fp64_iterations
        assert res[b].iterations <= 1.25 * r64[b].iterations + 20, (b, res[b].iterations, r64[b].iterations)
        its.append(res[b].iterations)
    if five:  # columns that end their segments and their solves at different passes: idling is exercised
        assert len(set(its)) >= 3, its


# ---- c. column independence, bitwise -----------------------------------------
def test_column_bits_do_not_depend_on_the_batch(sm, oracle):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_b(sm, oracle, Nx, Nt, U)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        L.cg_batch_precision("mixed")
        alone = [batch(sm, L, [c]) for c in cols]
        b5 = batch(sm, L, cols)
        again = batch(sm, L, cols)
        for b in range(5):
            assert b5[1][b].converged == 1 and b5[2][b].used == 1
            assert same(b5, again, b, b), b
            assert same(b5, alone[b], b, 0), b
        for shift in range(1, 5):  # every column in every position
            perm = [(b + shift) % 5 for b in range(5)]
            bp = batch(sm, L, [cols[p] for p in perm])
            for pos, p in enumerate(perm):
                assert same(bp, b5, pos, p), (shift, pos)
        # beside an all-zero column: alpha = 0 / 0 there, the column is handed to a finish that has nothing to do
        z = np.zeros_like(cols[0])
        bz = batch(sm, L, [cols[0], z, cols[1]])
        za = batch(sm, L, [z])
        assert same(bz, b5, 0, 0) and same(bz, b5, 2, 1)
        assert same(bz, za, 1, 0)
        assert np.all(np.isfinite(bz[0][1])) and np.all(bz[0][1] == 0.0)
        assert bz[1][1].converged == 0 and bz[1][1].phi_norm == 0.0
        # beside a column outside fp32's range: it leaves the fp32 passes alone and finishes in fp64
        big = spinor(sm, Nx, Nt, 4242) * 2.0 ** 127
        bb = batch(sm, L, [cols[0], big, cols[4]])
        ba = batch(sm, L, [big])
        assert same(bb, b5, 0, 0) and same(bb, b5, 2, 4)
        assert same(bb, ba, 1, 0)
        assert bb[2][1].fell_back == 1 and bb[1][1].converged == 1 and bb[2][1].fp64_iterations > 0
        rho = relres(oracle, Nx, Nt, U, big, bb[0][1])
        print(f"BATCH MIXED 2^127 column: rho {rho:.3e} fp64 iterations {bb[2][1].fp64_iterations}")
        assert rho < TOL
    finally:
        L.close()


def test_column_bits_at_the_largest_batch(sm):
    Nx, Nt = 6, 10
    U, _ = mm.synthetic(sm, Nx, Nt)
    kmax = sm.lib.sm_cg_batch_max()
    cols = [spinor(sm, Nx, Nt, 100 + b) for b in range(kmax)]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        L.cg_batch_precision("mixed")
        full = batch(sm, L, cols)
        assert all(r.converged == 1 for r in full[1]) and all(i.used == 1 for i in full[2])
        for b in (0, 1, kmax // 2, kmax - 1):
            assert same(full, batch(sm, L, [cols[b]]), b, 0), b
    finally:
        L.close()


@pytest.mark.parametrize("shape", [(130, 72), (515, 8), (130, 241)], ids=["130x72", "515x8", "130x241"])
def test_column_bits_do_not_depend_on_the_tile_height(sm, shape):
    """The tile height follows K and the tile target; the partial sums are kept
    per granule, so neither moves a bit. mp_delta_pct = 50 puts reliable
    updates (fold, true residual, injection) inside the 40 iterations compared."""
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    out = []
    for tiles in (0, 8, 40):
        with opts_env(mp_delta_pct=50, **({"batch_tiles": tiles} if tiles else {})):
            L = sm.Lattice(Nx, Nt)
        try:
            upload(sm, L, U)
            L.cg_batch_precision("mixed")
            out.append(batch(sm, L, cols, TOL, 40))
        finally:
            L.close()
    for b in range(len(cols)):
        assert out[0][1][b].iterations == 40 and out[0][2][b].reliable_updates >= 2, (b, out[0][2][b].reliable_updates)
        for o in out[1:]:
            assert same(o, out[0], b, b), b


# ---- d. separation -----------------------------------------------------------
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

    def download(self, p, like):
        out = np.empty_like(like)
        assert self.rt.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self, p):
        self.rt.hipFree(p)


def test_fp64_batch_unchanged_by_a_mixed_batch(sm):
    Nx, Nt = 32, 48
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        a = batch(sm, L, cols)
        assert L.cg_batch_precision("mixed") == "mixed"
        m = batch(sm, L, cols)
        assert L.cg_batch_precision("double") == "double"
        b = batch(sm, L, cols)
    finally:
        L.close()
    assert all(i.used == 0 for i in a[2] + b[2]) and all(i.used == 1 for i in m[2])
    for k in range(len(cols)):
        assert same(a, b, k, k), k
        assert not bits_equal(a[0][k], m[0][k]), k  # the mixed solve did run something else


def test_other_solvers_do_not_notice(sm):
    """sm_cg (fp64 and mixed), sm_eo_cg (fp64 and mixed) and a stepwise solve
    return the bits they return without mixed batched solves in between."""
    Nx, Nt = 32, 48
    S = Nx * Nt
    U, phi = mm.synthetic(sm, Nx, Nt)
    cols = [spinor(sm, Nx, Nt, 1), spinor(sm, Nx, Nt, 2), point(Nx, Nt, 3, 4, 1)]

    def sm_cg(L):
        x = np.empty(4 * S)
        res = sm.CGResult()
        sm.check(sm.lib.sm_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), M0, TOL, MAXIT,
                              ctypes.byref(res)))
        return x, rtuple(res), ituple(L.last_cg_mixed)

    def eo_cg(L):
        even = phi.copy().reshape(2, Nx, Nt, 2)
        xx, tt = np.meshgrid(np.arange(Nx), np.arange(Nt), indexing="ij")
        even[:, (xx + tt) % 2 == 1] = 0.0
        even = even.reshape(-1)
        x = np.empty(4 * S)
        res = sm.CGResult()
        sm.check(sm.lib.sm_eo_cg(L.ctx, ptr(even[:2 * S]), ptr(even[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), M0, TOL,
                                 MAXIT, ctypes.byref(res)))
        return x, rtuple(res), ituple(L.last_eo_cg_mixed)

    def run(with_batch):
        def between(L):
            if with_batch:
                _, res, info = batch(sm, L, cols)
                assert all(r.converged == 1 for r in res) and all(i.used == 1 for i in info)

        def stepwise(L):
            hip = _Hip()
            dphi, dx = hip.upload(phi), hip.alloc(phi.nbytes)
            res = sm.CGResult()
            sm.check(sm.lib.sm_cg_begin(L.ctx, dphi, dx, M0, TOL))
            sm.check(sm.lib.sm_cg_iterate(L.ctx, 9))
            between(L)
            sm.check(sm.lib.sm_cg_iterate(L.ctx, 4))
            between(L)
            sm.check(sm.lib.sm_cg_finish(L.ctx, ctypes.byref(res)))
            x = hip.download(dx, phi)
            hip.free(dphi)
            hip.free(dx)
            return x, rtuple(res), ()

        L = sm.Lattice(Nx, Nt)
        out = []
        try:
            upload(sm, L, U)
            L.cg_batch_precision("mixed")
            assert L.cg_precision() == "double" and L.eo_cg_precision() == "double"
            out.append(sm_cg(L))
            between(L)
            out.append(sm_cg(L))
            out.append(stepwise(L))
            L.cg_precision("mixed")
            assert L.cg_batch_precision() == "mixed" and L.eo_cg_precision() == "double"
            out.append(sm_cg(L))
            between(L)
            out.append(sm_cg(L))
            L.cg_precision("double")
            out.append(eo_cg(L))
            between(L)
            out.append(eo_cg(L))
            L.eo_cg_precision("mixed")
            assert L.cg_batch_precision() == "mixed" and L.cg_precision() == "double"
            out.append(eo_cg(L))
            between(L)
            out.append(eo_cg(L))
        finally:
            L.close()
        return out

    plain, mixed_in = run(False), run(True)
    assert len(plain) == len(mixed_in) == 9
    for i, (p, q) in enumerate(zip(plain, mixed_in)):
        assert bits_equal(p[0], q[0]) and p[1:] == q[1:], i
    assert plain[3][2][0] == 1 and plain[7][2][0] == 1  # the mixed sm_cg and sm_eo_cg did run mixed


def test_the_ensemble_stays_fp64(sm):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = [spinor(sm, Nx, Nt, 1), point(Nx, Nt, 0, 0, 0)]
    prm = [sm.HMCParams(M0, 2.0, 0.3, 6, TOL, MAXIT, 11, 0), sm.HMCParams(0.0, 3.0, 0.2, 6, TOL, MAXIT, 12, 0)]
    out = []
    for mode in ("double", "mixed"):
        L = sm.Lattice(Nx, Nt)
        try:
            upload(sm, L, U)
            L.cg_batch_precision("mixed")
            before = batch(sm, L, cols)
            L.cg_batch_precision(mode)
            E = L.ensemble(2)
            try:
                E.fill_gauge(0, 5, 0.3)
                E.fill_gauge(1, 6, 0.2)
                res = [E.trajectory(prm, t) for t in range(2)]
                fields = [E.download_gauge(r) for r in range(2)]
            finally:
                E.close()
            after = infos(sm, L, 2)  # still the two columns of the solve before the trajectories
            assert [ituple(i) for i in after] == [ituple(i) for i in before[2]]
            out.append((res, fields))
        finally:
            L.close()
    (ra, fa), (rb, fb) = out
    for t in range(2):
        for r in range(2):
            a, b = ra[t][r], rb[t][r]
            assert (a.H_old, a.H_new, a.dH, a.r, a.accepted, a.sp, a.cg_iterations) == \
                (b.H_old, b.H_new, b.dH, b.r, b.accepted, b.sp, b.cg_iterations), (t, r)
    for r in range(2):
        assert bits_equal(fa[r].view(np.float64), fb[r].view(np.float64)), r


# ---- e. gauge changes ----------------------------------------------------------
def test_gauge_changes_need_no_call(sm):
    Nx, Nt = 16, 16
    Ua, _ = mm.synthetic(sm, Nx, Nt)
    Ub, _ = mm.synthetic(sm, Nx, Nt, gauge_seed=99)
    cols = [spinor(sm, Nx, Nt, 1), point(Nx, Nt, 0, 0, 0), spinor(sm, Nx, Nt, 2)]
    L, F = sm.Lattice(Nx, Nt), sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, Ua)
        L.cg_batch_precision("mixed")
        first = batch(sm, L, cols)
        upload(sm, L, Ub)
        second = batch(sm, L, cols)
        upload(sm, F, Ub)
        F.cg_batch_precision("mixed")
        fresh = batch(sm, F, cols)
    finally:
        L.close()
        F.close()
    for b in range(3):
        assert same(second, fresh, b, b), b
        assert not bits_equal(first[0][b], second[0][b]), b


# ---- f. cut-off --------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [16, 17], ids=["stop_even", "stop_odd"])
def test_max_iter_cutoff(sm, oracle, max_iter):
    """Cut off after an even / odd number of fp32 passes: the count is exact and
    x holds everything iterated so far (the pending alpha d included), i.e. its
    fp64 residual by the oracle is the reported one."""
    meta, a = load_fixture("l64x64_b5_m-0p06")
    Nx, Nt, m0, U = meta["Nx"], meta["Nt"], meta["m0"], a["U"]
    cols = [a["psi"], spinor(sm, Nx, Nt, 77), point(Nx, Nt, 5, 63, 0)]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        L.cg_batch_precision("mixed")
        x, res, info = batch(sm, L, cols, TOL, max_iter, m0)
    finally:
        L.close()
    for b, phi in enumerate(cols):
        assert res[b].converged == 0 and res[b].iterations == max_iter and info[b].used == 1, b
        assert info[b].inner_iterations == max_iter and info[b].fell_back == 0, b
        assert np.all(np.isfinite(x[b]))
        rho = relres(oracle, Nx, Nt, U, phi, x[b], m0)
        print(f"BATCH MIXED max_iter {max_iter} column {b}: true relres {rho:.6e} (reported {info[b].true_residual:.6e})")
        assert abs(rho - info[b].true_residual) <= 1e-6 * rho, b
        assert abs(res[b].residual - rho * res[b].phi_norm) <= 1e-6 * res[b].residual, b


# ---- g. forced fallback ------------------------------------------------------------
def test_forced_fallback_finishes_in_fp64(sm, oracle):
    Nx, Nt = 32, 48
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    with opts_env(mp_force_fallback=1):
        L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        L.cg_batch_precision("mixed")
        full = batch(sm, L, cols)
        alone = [batch(sm, L, [c]) for c in cols]
    finally:
        L.close()
    x, res, info = full
    for b, phi in enumerate(cols):
        assert info[b].fell_back == 1 and info[b].reliable_updates == 1 and info[b].fp64_iterations > 0, b
        assert res[b].converged == 1 and res[b].iterations == info[b].inner_iterations + info[b].fp64_iterations
        rho = relres(oracle, Nx, Nt, U, phi, x[b])
        print(f"BATCH MIXED forced fallback column {b}: inner {info[b].inner_iterations} fp64 "
              f"{info[b].fp64_iterations} rho {rho:.3e}")
        assert rho < TOL, (b, rho)
        assert same(full, alone[b], b, 0), b


# ---- h. entry points -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["double", "mixed"])
def test_host_and_device_entry_points_agree(sm, mode):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = [spinor(sm, Nx, Nt, 1), point(Nx, Nt, 5, 6, 1), spinor(sm, Nx, Nt, 2)]
    L = sm.Lattice(Nx, Nt)
    hip = _Hip()
    try:
        upload(sm, L, U)
        assert L.cg_batch_precision(mode) == mode
        host = batch(sm, L, cols)
        hphi = np.ascontiguousarray(np.stack(cols))
        dphi, dx = hip.upload(hphi), hip.alloc(hphi.nbytes)
        res = (sm.CGResult * 3)()
        sm.check(sm.lib.sm_cg_batch_dev(L.ctx, 3, dphi, dx, M0, TOL, MAXIT, res))
        dev = (hip.download(dx, hphi), list(res), infos(sm, L, 3))
        hip.free(dphi)
        hip.free(dx)
        for b in range(3):
            assert same(host, dev, b, b), b
            assert host[2][b].used == (1 if mode == "mixed" else 0)
        # a K that is not the last solve's
        out = (sm.CGMixedInfo * 4)()
        assert sm.lib.sm_cg_batch_mixed_last(L.ctx, 2, out) == SM_ERR_ARG
        assert sm.lib.sm_cg_batch_mixed_last(L.ctx, 4, out) == SM_ERR_ARG
        assert sm.lib.sm_cg_batch_mixed_last(L.ctx, 3, None) == SM_ERR_ARG
    finally:
        L.close()


# ---- i. refusals ---------------------------------------------------------------------
def test_loopback_contexts_refuse_and_stay_fp64(sm):
    Nx, Nt = 8, 8
    for kind in (True, "peer"):
        B = sm.Lattice(Nx, Nt, loopback=kind)
        try:
            mode = ctypes.c_int(-1)
            assert sm.lib.sm_cg_batch_precision(B.ctx, 1, ctypes.byref(mode)) == SM_ERR_ARG
            assert mode.value == 0
            with pytest.raises(sm.SMError):
                B.cg_batch_precision("mixed")
            assert B.cg_batch_precision() == "double"
            assert B.cg_batch_precision("double") == "double"
        finally:
            B.close()


# ---- j. Python --------------------------------------------------------------------------
def test_python_cg_batch_precision_attribute(sm):
    Nx = Nt = 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    try:
        assert L.cg_batch_precision() == "double" and L.last_cg_batch_mixed == []
        assert L.cg_batch_precision("mixed") == "mixed" and L.cg_batch_precision() == "mixed"
        assert L.cg_precision() == "double" and L.eo_cg_precision() == "double"
        assert L.cg_batch_precision(0) == "double"
        assert L.cg_batch_precision(1) == "mixed"
        with pytest.raises(sm.SMError):
            L.cg_batch_precision(7)
        assert L.cg_batch_precision() == "mixed"  # a refused mode changes nothing
        with pytest.raises(ValueError):
            L.cg_batch_precision("single")
        upload(sm, L, U)
        phi = np.stack([spinor(sm, Nx, Nt, 1), spinor(sm, Nx, Nt, 2)]).view(np.complex128).reshape(2, 2, L.V)
        _, res = L.cg_batch(phi, M0, tol=TOL, max_iter=MAXIT)
        info = L.last_cg_batch_mixed
        assert len(info) == 2 and all(i.used == 1 for i in info) and all(r.converged == 1 for r in res)
        assert [r.iterations for r in res] == [i.inner_iterations + i.fp64_iterations for i in info]
        assert L.cg_batch_precision("double") == "double"
        L.cg_batch(phi[:1], M0, tol=TOL, max_iter=MAXIT)
        info = L.last_cg_batch_mixed
        assert len(info) == 1 and info[0].used == 0
    finally:
        L.close()


# ---- k. pion correlator ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 10), (16, 16)], ids=["6x10", "16x16"])
def test_pion_correlator_mixed_against_fp64(sm, shape):
    """Both modes return y with ||phi - D D^dag y|| <= tol (||phi|| = 1), so
    ||D D^dag (y - y')|| <= 2 tol and, with S = D^dag y = D^-1 D D^dag y,
    ||S - S'|| <= e = 2 tol sqrt(1 / lmin(D D^dag)). A slice of C is the squared
    norm of the slices of two such columns: | |a|^2 - |b|^2 | <= 2 |a| |a - b| +
    |a - b|^2 per column with |a| <= sqrt(C(t)), so
    |C(t) - C'(t)| <= 2 (2 sqrt(C64(t)) e + e^2). 1 / lmin: three inverse
    iterations through the fp64 sm_cg (a lower estimate, doubled). Derived, not
    fitted; 1 % of room for the estimate of C by C64."""
    Nx, Nt = shape
    S = Nx * Nt
    U, _ = mm.synthetic(sm, Nx, Nt)
    sources = [(0, 0), (Nx // 2, Nt - 1), (Nx - 1, 3)]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        C64, r64 = L.pion_correlator(M0, sources, tol=TOL, max_iter=MAXIT)
        assert all(i.used == 0 for i in L.last_cg_batch_mixed) and len(L.last_cg_batch_mixed) == 6
        L.cg_batch_precision("mixed")
        C, res = L.pion_correlator(M0, sources, tol=TOL, max_iter=MAXIT)
        info = L.last_cg_batch_mixed
        v, inv_l = spinor(sm, Nx, Nt, 9), 0.0
        v /= np.linalg.norm(v)
        for _ in range(3):
            w = np.empty(4 * S)
            r = sm.CGResult()
            sm.check(sm.lib.sm_cg(L.ctx, ptr(v[:2 * S]), ptr(v[2 * S:]), ptr(w[:2 * S]), ptr(w[2 * S:]), M0, 1e-8, MAXIT,
                                  ctypes.byref(r)))
            inv_l = max(inv_l, np.linalg.norm(w))
            v = w / np.linalg.norm(w)
        inv_l *= 2.0
    finally:
        L.close()
    assert len(info) == 6 and all(i.used == 1 for i in info)
    assert all(r.converged == 1 for r in res) and all(r.converged == 1 for r in r64)
    e = 2.0 * TOL * math.sqrt(inv_l)
    lim = 1.01 * 2.0 * (2.0 * np.sqrt(C64) * e + e * e)
    worst = float(np.max(np.abs(C - C64) / lim))
    print(f"BATCH MIXED PION {Nx}x{Nt}: 1/lmin {inv_l:.3e} e {e:.3e} worst |dC| / bound {worst:.3e}")
    assert np.all(np.abs(C - C64) <= lim)
    assert not bits_equal(C, C64)
