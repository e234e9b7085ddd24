"""The batched multi-source CG (sm_cgbatch.hip, sm_cgbatch.cpp): K right-hand
sides on one gauge field, one launch per iteration, every column with its own
scalars and stop test.

a. iterates against the reference's CG (oracle_cg cut off at max_iter = k),
   column by column, to the 1e-12 every fp64 path is held to, at the kernel's
   own tile edges;  b. whole solves whose columns stop at different counts;
c. a column's bits do not depend on K, its position, its neighbours or the
   tile height;  d. the other solvers do not notice a batched solve;
e. gauge changes need no call;  f. regrowth;  g. host and device entry
   points;  h. refusals.
"""
import ctypes

import numpy as np
import pytest

import mixed_model as mm
from conftest import bits_equal, opts_env, ptr

pytestmark = pytest.mark.gpu

M0 = -0.10
KS = (1, 2, 3, 4, 5, 6, 7, 12)
SM_ERR_ARG, SM_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def upload(sm, L, U):
    S = L.V
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))


def download(sm, L):
    S = L.V
    U = np.empty(4 * S)
    sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
    return U


def spinor(sm, Nx, Nt, seed):
    S = Nx * Nt
    p = np.empty(4 * S)
    sm.lib.sm_fill_spinor(seed, Nt, 0, Nx, 0, Nt, ptr(p[:2 * S]), ptr(p[2 * S:]))
    return p


def point(Nx, Nt, x, t, plane):
    p = np.zeros(4 * Nx * Nt)
    p[2 * (plane * Nx * Nt + x * Nt + t)] = 1.0
    return p


def batch(sm, L, cols, tol, max_iter, m0=M0, expect=0):
    """sm_cg_batch on the columns (4 S doubles each); returns (x[K, 4S], results)."""
    K = len(cols)
    phi = np.ascontiguousarray(np.stack(cols))
    x = np.full_like(phi, np.nan)
    res = (sm.CGResult * K)()
    rc = sm.lib.sm_cg_batch(L.ctx, K, ptr(phi), ptr(x), m0, tol, max_iter, res)
    assert rc == expect, (rc, sm.lib.sm_last_error())
    return x, list(res)


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


def rtuple(r):
    return (r.converged, r.iterations, np.float64(r.residual).view(np.uint64), np.float64(r.phi_norm).view(np.uint64))


def same(xa, ra, xb, rb):
    return bits_equal(xa, xb) and rtuple(ra) == rtuple(rb)


def oracle_cg(oracle, Nx, Nt, U, phi, m0, tol, max_iter):
    S = Nx * Nt
    x = np.empty(4 * S)
    it, err = ctypes.c_int(), ctypes.c_double()
    conv = oracle.oracle_cg(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]),
                            ptr(x[2 * S:]), m0, tol, max_iter, ctypes.byref(it), ctypes.byref(err))
    return x, conv, it.value


def sm_cg(sm, L, phi, tol, max_iter, m0=M0):
    S = L.V
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, tol, max_iter,
                          ctypes.byref(res)))
    return x, res


# ---- a. iterates against the reference ----------------------------------------
# A tile is one wave: 60 owned t-columns (2 halo lanes per side) times xchunk
# rows; partial sums per granule of G rows (G = 1 below Nx = 512, 8 from there);
# P = ceil(Nt / 60) * ceil(Nx / G) slots per column, redundant scalars up to
# P = 512 and a scalar kernel above. A block is one wave, so "a second wave"
# and "a second block" are the same edge here; 7x121 puts one column into a
# third.
#   4x2      narrower than the t-halo: lanes wrap onto themselves
#   5x9      odd both ways
#   3x60     exactly one wave's owned columns; fewer rows than the 5-row prologue
#   6x61     one column spills into a second wave (= block)
#   7x62     the second wave owns exactly a halo's width
#   7x121    one column in a third wave
#   130x72   several x-chunks (one row per tile at K = 3: 130 chunks, 2 t-tiles)
#   130x241  P = 650 > 512: the scalar-kernel path instead of redundant scalars
#   515x8    G = 8: 8-row granules, the last one 3 rows
SHAPES = [(4, 2), (5, 9), (3, 60), (6, 61), (7, 62), (7, 121), (130, 72), (130, 241), (515, 8)]


def columns_a(sm, Nx, Nt):
    return [spinor(sm, Nx, Nt, 5678), spinor(sm, Nx, Nt, 91011), point(Nx, Nt, Nx // 2, Nt - 1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_iterates_match_reference(sm, oracle, shape):
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    worst = 0.0
    try:
        upload(sm, L, U)
        for k in KS:
            x, res = batch(sm, L, cols, 0.0, k)
            for b, phi in enumerate(cols):
                assert res[b].iterations == k and res[b].converged == 0, (k, b, res[b].iterations, res[b].converged)
                ref, _, it = oracle_cg(oracle, Nx, Nt, U, phi, M0, 0.0, k)
                assert it == k
                rel = np.linalg.norm(x[b] - ref) / np.linalg.norm(ref)
                worst = max(worst, rel)
                assert rel <= 1e-12, (k, b, rel)
    finally:
        L.close()
    print(f"BATCH ITERATES {Nx}x{Nt}: worst relative deviation {worst:.3e}")


# ---- b. whole solves -------------------------------------------------------------
# A whole solve is compared with the reference's to 1e-12 in x, which presumes
# both stop at the same iteration. The stop is a threshold on |r|, and the bar
# on the iterates itself leaves |r| undetermined to about bar / tol = 1e-12 /
# 1e-10 = 1 %: an x that differs by 1e-12 |x| has a residual that differs by
# about that fraction of tol |phi|. A source whose REFERENCE residual passes
# within 1 % of the threshold at the stopping iteration or the one before is a
# coin flip between two correct solvers, not a test of one. So every kind of
# column takes the first of its candidates that the reference alone decides:
# |r_it| <= 0.99 tol |phi| and |r_{it-1}| >= 1.01 tol |phi| in oracle_cg. The
# choice never looks at the library's result.
def decided_by_the_reference(oracle, Nx, Nt, U, phi, tol=1e-10):
    S = Nx * Nt
    x = np.empty(4 * S)
    it, err = ctypes.c_int(), ctypes.c_double()
    thr = tol * np.linalg.norm(phi)
    args = (Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), M0)
    assert oracle.oracle_cg(*args, tol, 10000, ctypes.byref(it), ctypes.byref(err)) == 1
    last, n = err.value, it.value
    oracle.oracle_cg(*args, 0.0, n - 1, ctypes.byref(it), ctypes.byref(err))
    return last <= 0.99 * thr and err.value >= 1.01 * thr


_COLS_B = {}


def columns_b(sm, oracle, Nx, Nt, U):
    """The columns of (b) and (c), chosen once per shape and left unchanged."""
    if (Nx, Nt) not in _COLS_B:
        cols = _choose_columns_b(sm, oracle, Nx, Nt, U)
        for c in cols:
            c.setflags(write=False)
        _COLS_B[(Nx, Nt)] = cols
    return _COLS_B[(Nx, Nt)]


def _choose_columns_b(sm, oracle, Nx, Nt, U):
    """A random source, a point source, a random one scaled by 2^40, and two
    heavy on the low modes, which stop at other counts: (D D^dag)^-2 r (about
    10 % earlier) and (D D^dag)^-1 r. Not D D^dag r: with x0 = phi that source
    has |phi| = 6.7 |x|, the iterates x_k = phi + corrections cancel most of
    phi, and the library's default fp64 path itself (sm_cg) then ends 1.2e-11
    from the reference on 32x48 and 1.6e-11 on 16x16, the batch with the very
    same figures: the 1e-12 bar of the fp64 paths is a bar for sources whose
    solution is not much smaller than they are."""
    def first(candidates):
        for phi in candidates:
            if decided_by_the_reference(oracle, Nx, Nt, U, phi):
                return phi
        raise AssertionError("no candidate whose stop the reference decides")

    def inverse(v):
        return oracle_cg(oracle, Nx, Nt, U, v, M0, 1e-12, 10000)[0]

    seeds = range(31, 47)
    return [first(spinor(sm, Nx, Nt, 5678 + s) for s in seeds),
            first(point(Nx, Nt, s % Nx, (2 * s) % Nt, s & 1) for s in seeds),
            first(spinor(sm, Nx, Nt, 777 + s) * 2.0 ** 40 for s in seeds),
            first(inverse(inverse(spinor(sm, Nx, Nt, s))) for s in seeds),
            first(inverse(spinor(sm, Nx, Nt, s)) for s in seeds)]


@pytest.mark.parametrize("shape", [(32, 48), (16, 16)], ids=["32x48", "16x16"])
def test_whole_solves_stop_per_column(sm, oracle, shape):
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_b(sm, oracle, Nx, Nt, U)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        x, res = batch(sm, L, cols, 1e-10, 10000)
    finally:
        L.close()
    its = []
    for b, phi in enumerate(cols):
        ref, conv, it = oracle_cg(oracle, Nx, Nt, U, phi, M0, 1e-10, 10000)
        rel = np.linalg.norm(x[b] - ref) / np.linalg.norm(ref)
        print(f"BATCH SOLVE {Nx}x{Nt} column {b}: iterations {res[b].iterations} (reference {it}) deviation {rel:.3e}")
        assert conv == 1 and res[b].converged == 1, b
        assert abs(res[b].iterations - it) <= max(1, it // 100), (b, res[b].iterations, it)
        assert rel <= 1e-12, (b, rel)
        assert res[b].residual < 1e-10 * res[b].phi_norm
        assert res[b].phi_norm == pytest.approx(np.linalg.norm(phi), rel=1e-13)
        its.append(res[b].iterations)
    # the random sources, (D D^dag)^-2 r and (D D^dag)^-1 r stop at different counts
    assert len(set(its)) >= 3, its


# ---- c. column independence, bitwise ------------------------------------------------
def test_column_bits_do_not_depend_on_the_batch(sm, oracle):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_b(sm, oracle, Nx, Nt, U)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        alone = [batch(sm, L, [c], 1e-10, 10000) for c in cols]
        x5, r5 = batch(sm, L, cols, 1e-10, 10000)
        again = batch(sm, L, cols, 1e-10, 10000)
        assert bits_equal(x5, again[0]) and [rtuple(r) for r in r5] == [rtuple(r) for r in again[1]]
        for b in range(5):
            assert same(x5[b], r5[b], alone[b][0][0], alone[b][1][0]), b
        for shift in range(1, 5):  # every column in every position
            perm = [(b + shift) % 5 for b in range(5)]
            xp, rp = batch(sm, L, [cols[p] for p in perm], 1e-10, 10000)
            for pos, p in enumerate(perm):
                assert same(xp[pos], rp[pos], x5[p], r5[p]), (shift, pos)
        # next to an all-zero column (alpha = 0 / 0 there, as in a lone sm_cg_dev: it runs to max_iter)
        z = np.zeros_like(cols[0])
        lone40 = [batch(sm, L, [c], 1e-10, 40) for c in cols[:2]]
        xz, rz = batch(sm, L, [cols[0], z, cols[1]], 1e-10, 40)
        assert same(xz[0], rz[0], lone40[0][0][0], lone40[0][1][0])
        assert same(xz[2], rz[2], lone40[1][0][0], lone40[1][1][0])
        assert rz[1].converged == 0 and rz[1].phi_norm == 0.0
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
        x, res = batch(sm, L, cols, 1e-10, 10000)
        assert all(r.converged == 1 for r in res)
        for b in (0, 1, kmax // 2, kmax - 1):
            xa, ra = batch(sm, L, [cols[b]], 1e-10, 10000)
            assert same(x[b], res[b], xa[0], ra[0]), b
    finally:
        L.close()


@pytest.mark.parametrize("shape", [(130, 72), (515, 8), (130, 241)], ids=["130x72", "515x8", "130x241"])
def test_column_bits_do_not_depend_on_the_tile_height(sm, shape):
    """The tile height follows K and the tile target; the partial sums are kept
    per granule, so neither moves a bit."""
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    out = []
    for tiles in (0, 8, 40):
        with opts_env(**({"batch_tiles": tiles} if tiles else {})):
            L = sm.Lattice(Nx, Nt)
        try:
            upload(sm, L, U)
            out.append(batch(sm, L, cols, 0.0, 12))
        finally:
            L.close()
    for x, res in out[1:]:
        assert bits_equal(x, out[0][0])
        assert [rtuple(r) for r in res] == [rtuple(r) for r in out[0][1]]


# ---- d. separation -----------------------------------------------------------------
def test_other_solvers_do_not_notice(sm):
    Nx, Nt = 32, 48
    S = Nx * Nt
    U, phi = mm.synthetic(sm, Nx, Nt)
    cols = [spinor(sm, Nx, Nt, 1), spinor(sm, Nx, Nt, 2), point(Nx, Nt, 3, 4, 1)]

    def eo_cg(L):
        even = phi.copy().reshape(2, Nx, Nt, 2)
        xx, tt = np.meshgrid(np.arange(Nx), np.arange(Nt), indexing="ij")
        even[:, (xx + tt) % 2 == 1] = 0.0
        even = even.reshape(-1)
        x = np.empty(4 * S)
        res = sm.CGResult()
        sm.check(sm.lib.sm_eo_cg(L.ctx, ptr(even[:2 * S]), ptr(even[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), M0, 1e-10,
                                 10000, ctypes.byref(res)))
        return x, res

    def stepwise(L, with_batch):
        hip = _Hip()
        dphi, dx = hip.upload(phi), hip.alloc(phi.nbytes)
        res = sm.CGResult()
        sm.check(sm.lib.sm_cg_begin(L.ctx, dphi, dx, M0, 1e-10))
        sm.check(sm.lib.sm_cg_iterate(L.ctx, 9))
        if with_batch:
            batch(sm, L, cols, 1e-10, 10000)
        sm.check(sm.lib.sm_cg_iterate(L.ctx, 4))
        if with_batch:
            batch(sm, L, cols, 1e-10, 10000)
        sm.check(sm.lib.sm_cg_finish(L.ctx, ctypes.byref(res)))
        x = hip.download(dx, phi)
        hip.free(dphi)
        hip.free(dx)
        return x, res

    def run(with_batch):
        L = sm.Lattice(Nx, Nt)
        out = []
        try:
            upload(sm, L, U)
            out.append(sm_cg(sm, L, phi, 1e-10, 10000))
            if with_batch:
                batch(sm, L, cols, 1e-10, 10000)
            out.append(sm_cg(sm, L, phi, 1e-10, 10000))
            out.append(stepwise(L, with_batch))
            L.cg_precision("mixed")
            out.append(sm_cg(sm, L, phi, 1e-10, 10000))
            if with_batch:
                batch(sm, L, cols, 1e-10, 10000)
            out.append(sm_cg(sm, L, phi, 1e-10, 10000))
            L.cg_precision("double")
            out.append(eo_cg(L))
            if with_batch:
                batch(sm, L, cols, 1e-10, 10000)
            out.append(eo_cg(L))
            L.eo_cg_precision("mixed")
            out.append(eo_cg(L))
            if with_batch:
                batch(sm, L, cols, 1e-10, 10000)
            out.append(eo_cg(L))
        finally:
            L.close()
        return out

    plain, mixed_in = run(False), run(True)
    assert len(plain) == len(mixed_in) == 9
    for i, ((xa, ra), (xb, rb)) in enumerate(zip(plain, mixed_in)):
        assert same(xa, ra, xb, rb), i


# ---- e. gauge changes -----------------------------------------------------------------
def test_gauge_changes_need_no_call(sm):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    U2, _ = mm.synthetic(sm, Nx, Nt, gauge_seed=99)
    cols = [spinor(sm, Nx, Nt, 1), point(Nx, Nt, 0, 0, 0), spinor(sm, Nx, Nt, 2)]

    def fresh(Unow):
        F = sm.Lattice(Nx, Nt)
        try:
            upload(sm, F, Unow)
            return batch(sm, F, cols, 1e-10, 10000)
        finally:
            F.close()

    def check_against_fresh(L, what):
        x, res = batch(sm, L, cols, 1e-10, 10000)
        xf, rf = fresh(download(sm, L))
        assert bits_equal(x, xf) and [rtuple(r) for r in res] == [rtuple(r) for r in rf], what

    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        first = batch(sm, L, cols, 1e-10, 10000)
        upload(sm, L, U2)
        check_against_fresh(L, "upload")
        assert not bits_equal(first[0], batch(sm, L, cols, 1e-10, 10000)[0])
        r = sm.HMCResult()
        # a short, finely stepped trajectory is accepted (dH ~ 1e-4) ...
        p = sm.HMCParams(M0, 2.0, 0.1, 20, 1e-10, 10000, 2024, 0)
        sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(p), 0, ctypes.byref(r)))
        assert r.accepted == 1, (r.dH, r.r)
        check_against_fresh(L, "accepted trajectory")
        # ... one coarse step over a long trajectory is rejected (dH >> 1)
        before = download(sm, L)
        p = sm.HMCParams(M0, 2.0, 6.0, 2, 1e-10, 10000, 2024, 0)
        sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(p), 1, ctypes.byref(r)))
        assert r.accepted == 0, (r.dH, r.r)
        assert bits_equal(before, download(sm, L))
        check_against_fresh(L, "rejected trajectory")
    finally:
        L.close()


# ---- f. regrowth ---------------------------------------------------------------------------
def test_regrowth_keeps_the_bits(sm):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = [spinor(sm, Nx, Nt, 10 + b) for b in range(9)]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        x2, r2 = batch(sm, L, cols[:2], 1e-10, 10000)
        x9, r9 = batch(sm, L, cols, 1e-10, 10000)
        x2b, r2b = batch(sm, L, cols[:2], 1e-10, 10000)
    finally:
        L.close()
    assert bits_equal(x2, x2b) and [rtuple(r) for r in r2] == [rtuple(r) for r in r2b]
    assert bits_equal(x9[:2], x2) and all(r.converged == 1 for r in r9)


# ---- g. host and device entry points -----------------------------------------------------------
def test_host_and_device_entry_points_agree(sm):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = [spinor(sm, Nx, Nt, 1), point(Nx, Nt, 5, 6, 1), spinor(sm, Nx, Nt, 2)]
    L = sm.Lattice(Nx, Nt)
    hip = _Hip()
    try:
        upload(sm, L, U)
        xh, rh = batch(sm, L, cols, 1e-10, 10000)
        hphi = np.ascontiguousarray(np.stack(cols))
        dphi, dx = hip.upload(hphi), hip.alloc(hphi.nbytes)
        res = (sm.CGResult * 3)()
        sm.check(sm.lib.sm_cg_batch_dev(L.ctx, 3, dphi, dx, M0, 1e-10, 10000, res))
        assert bits_equal(hip.download(dx, hphi), xh)
        assert [rtuple(r) for r in res] == [rtuple(r) for r in rh]
        # x must not alias phi
        assert sm.lib.sm_cg_batch_dev(L.ctx, 3, dphi, dphi, M0, 1e-10, 10000, res) == SM_ERR_ARG
        hip.free(dphi)
        hip.free(dx)
        # through the package
        xp, rp = L.cg_batch(np.stack(cols).view(np.complex128).reshape(3, 2, L.V), M0, tol=1e-10, max_iter=10000)
        assert bits_equal(xp.view(np.float64).reshape(3, -1), xh)
        assert [rtuple(r) for r in rp] == [rtuple(r) for r in rh]
    finally:
        L.close()


# ---- h. refusals -------------------------------------------------------------------------------
def test_refusals(sm):
    Nx, Nt = 8, 8
    U, phi = mm.synthetic(sm, Nx, Nt)
    kmax = sm.lib.sm_cg_batch_max()
    L = sm.Lattice(Nx, Nt)
    try:
        batch(sm, L, [phi], 1e-10, 100, expect=SM_ERR_STATE)  # no gauge field yet
        upload(sm, L, U)
        res = (sm.CGResult * (kmax + 1))()
        big = np.zeros((kmax + 1, 4 * L.V))
        out = np.zeros_like(big)
        assert sm.lib.sm_cg_batch(L.ctx, 0, ptr(big), ptr(out), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert sm.lib.sm_cg_batch(L.ctx, kmax + 1, ptr(big), ptr(out), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert sm.lib.sm_cg_batch(L.ctx, 1, None, ptr(out), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert sm.lib.sm_cg_batch(L.ctx, 1, ptr(big), None, M0, 1e-10, 100, res) == SM_ERR_ARG
        assert sm.lib.sm_cg_batch(L.ctx, 1, ptr(big), ptr(out), M0, 1e-10, 100, None) == SM_ERR_ARG
        want = sm_cg(sm, L, phi, 1e-10, 10000)
        _, r = batch(sm, L, [phi], 1e-10, 10000)  # still usable after the refusals
        assert r[0].converged == 1
    finally:
        L.close()
    for kind in (True, "peer"):
        B = sm.Lattice(Nx, Nt, loopback=kind)
        try:
            upload(sm, B, U)
            batch(sm, B, [phi], 1e-10, 100, expect=SM_ERR_ARG)
            got = sm_cg(sm, B, phi, 1e-10, 10000)
            assert got[1].converged == 1 and got[1].iterations == want[1].iterations
            assert np.linalg.norm(got[0] - want[0]) <= 1e-12 * np.linalg.norm(want[0])
        finally:
            B.close()
