"""The batched one-pass even-odd CG (sm_eobatch.hip, sm_eobatch.cpp): K even
right-hand sides of Dhat Dhat^dag on one gauge field, one launch per iteration,
every column with its own scalars and stop test.

a. iterates against textbook CG on the oracle-composed Dhat Dhat^dag
   (eo_mixed_model.cg_iterates_fp64), column by column; the bar is what the
   lone sm_eo_cg_dev deviates from the same model on the same column and k,
   times 4, and never below 1e-12;  b. whole solves whose columns stop at
   different counts, against the lone solver and the true residual;
c. a column's bits do not depend on K, its position, its neighbours, regrowth
   or the tile height;  d. the other solvers do not notice;  e. gauge changes
   need no call;  f. refusals.

The kernel's tile is one wave of 56 owned k-columns (k = t / 2; 4 halo lanes
per side) times xchunk rows, as sm_eotd.hip's wave, so the issue's t-edges
hold as given. Two shapes are moved to this kernel's own edges: partial sums
are kept per granule of G = 2 rows below Nx = 512 (G is even: the march's row
parities are static), so 130x482 has only 5 * 65 = 325 slots, under the
redundant-scalar cap of 512; 130x962 (9 waves x 65 granules = 585 slots) takes
the scalar-kernel path instead. 516x8 has G = 8 and a last granule of 4 rows.
"""
import ctypes

import numpy as np
import pytest

import eo_mixed_model as em
import mixed_model as mm
from conftest import bits_equal, opts_env, ptr
from test_cg_batch_gpu import _Hip, batch as full_batch, download, rtuple, same, sm_cg, spinor, upload

pytestmark = pytest.mark.gpu

M0 = -0.10
KS = (1, 2, 3, 4, 5, 6, 7, 12)
SM_ERR_ARG, SM_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


@pytest.fixture(scope="module")
def hip():
    return _Hip()


def even(v, Nx, Nt):
    return em.even_part(v, Nx, Nt)


def point_even(Nx, Nt, x, t, plane):
    """A unit vector at an even site (t moved down by one if (x + t) is odd)."""
    if (x + t) % 2:
        t = (t - 1) % Nt
    p = np.zeros(4 * Nx * Nt)
    p[2 * (plane * Nx * Nt + x * Nt + t)] = 1.0
    return p


def batch(sm, L, cols, tol, max_iter, m0=M0, expect=0):
    """sm_eo_cg_batch on the columns (4 S doubles each); returns (x[K, 4S], results)."""
    K = len(cols)
    phi = np.ascontiguousarray(np.stack(cols))
    x = np.full_like(phi, np.nan)
    res = (sm.CGResult * K)()
    rc = sm.lib.sm_eo_cg_batch(L.ctx, K, ptr(phi), ptr(x), m0, tol, max_iter, res)
    assert rc == expect, (rc, sm.lib.sm_last_error())
    return x, list(res)


def lone(sm, hip, L, phi, tol, max_iter, m0=M0):
    """The lone sm_eo_cg_dev on one column; (x, result), or (None, None) where it refuses."""
    dphi, dx = hip.upload(phi), hip.alloc(phi.nbytes)
    res = sm.CGResult()
    rc = sm.lib.sm_eo_cg_dev(L.ctx, dphi, dx, m0, tol, max_iter, ctypes.byref(res))
    x = hip.download(dx, phi) if rc == 0 else None
    hip.free(dphi)
    hip.free(dx)
    return (x, res) if rc == 0 else (None, None)


# ---- a. iterates -------------------------------------------------------------------
#   4x4      half-width 2, narrower than the 4-lane halo: lanes wrap more than once
#   6x10     odd half-width
#   4x112    exactly one wave's owned columns; fewer rows than the 8-row prologue
#   6x114    one column spills into a second wave
#   8x120    the second wave owns exactly a halo's width
#   130x72   many x-chunks (one granule per tile at K = 3)
#   130x962  585 partial slots > 512: the scalar-kernel path
#   516x8    8-row granules, the last one 4 rows
SHAPES = [(4, 4), (6, 10), (4, 112), (6, 114), (8, 120), (130, 72), (130, 962), (516, 8)]


def columns_a(sm, Nx, Nt):
    return [even(spinor(sm, Nx, Nt, 5678), Nx, Nt), even(spinor(sm, Nx, Nt, 91011), Nx, Nt),
            point_even(Nx, Nt, Nx // 2, Nt - 1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_iterates_match_the_model_as_the_lone_solver_does(sm, hip, oracle, shape):
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    model = [em.cg_iterates_fp64(oracle, Nx, Nt, U, phi, M0, max(KS)) for phi in cols]
    L = sm.Lattice(Nx, Nt)
    worst_b = worst_l = 0.0
    try:
        upload(sm, L, U)
        for k in KS:
            x, res = batch(sm, L, cols, 0.0, k)
            for b, phi in enumerate(cols):
                assert res[b].iterations == k and res[b].converged == 0, (k, b, res[b].iterations, res[b].converged)
                ref = model[b][k - 1]
                nr = np.linalg.norm(ref)
                xl, rl = lone(sm, hip, L, phi, 0.0, k)
                bar = 1e-12
                if xl is not None:
                    assert rl.iterations == k
                    dev_l = np.linalg.norm(xl - ref) / nr
                    worst_l = max(worst_l, dev_l)
                    bar = max(1e-12, 4 * dev_l)
                dev_b = np.linalg.norm(x[b] - ref) / nr
                worst_b = max(worst_b, dev_b)
                assert dev_b <= bar, (k, b, dev_b, bar)
    finally:
        L.close()
    print(f"EO BATCH ITERATES {Nx}x{Nt}: worst relative deviation from the model: batch {worst_b:.3e}, "
          f"lone sm_eo_cg_dev {worst_l:.3e}")


# ---- b. whole solves ---------------------------------------------------------------
# test_cg_batch_gpu.py's rule, with the lone fp64 even-odd solver as the judge:
# a source counts only if that solver's residual passes the threshold by 1 % on
# both sides (|r_it| <= 0.99 tol |phi|, |r_{it-1}| >= 1.01 tol |phi|), so the
# stopping iteration is not a coin flip between two correct solvers. The choice
# never looks at the batch's result.
_COLS_B = {}


def decided_by_the_lone_solver(sm, hip, L, phi, tol=1e-10):
    thr = tol * np.linalg.norm(phi)
    _, r = lone(sm, hip, L, phi, tol, 10000)
    assert r.converged == 1
    _, q = lone(sm, hip, L, phi, 0.0, r.iterations - 1)
    return r.residual <= 0.99 * thr and q.residual >= 1.01 * thr


def columns_b(sm, hip, Nx, Nt, U):
    """A random source, a point source, a random one scaled by 2^40 and two
    heavy on the low modes ((Dhat Dhat^dag)^-2 r and (Dhat Dhat^dag)^-1 r),
    chosen once per shape and left unchanged."""
    if (Nx, Nt) in _COLS_B:
        return _COLS_B[(Nx, Nt)]
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)

        def first(candidates):
            for phi in candidates:
                if decided_by_the_lone_solver(sm, hip, L, phi):
                    return phi
            raise AssertionError("no candidate whose stop the lone solver decides")

        def inverse(v):
            return lone(sm, hip, L, v, 1e-12, 10000)[0]

        def rnd(seed):
            return even(spinor(sm, Nx, Nt, seed), Nx, Nt)

        seeds = range(31, 47)
        cols = [first(rnd(5678 + s) for s in seeds),
                first(point_even(Nx, Nt, s % Nx, (2 * s) % Nt, s & 1) for s in seeds),
                first(rnd(777 + s) * 2.0 ** 40 for s in seeds),
                first(inverse(inverse(rnd(s))) for s in seeds),
                first(inverse(rnd(s)) for s in seeds)]
    finally:
        L.close()
    for c in cols:
        c.setflags(write=False)
    _COLS_B[(Nx, Nt)] = cols
    return cols


def eo_dhat(sm, L, v, dag, m0=M0):
    S = L.V
    out = np.empty(4 * S)
    sm.check(sm.lib.sm_eo_dhat(L.ctx, dag, ptr(v[:2 * S]), ptr(v[2 * S:]), ptr(out[:2 * S]), ptr(out[2 * S:]), m0))
    return out


@pytest.mark.parametrize("shape", [(32, 48), (16, 16)], ids=["32x48", "16x16"])
def test_whole_solves_stop_per_column(sm, hip, shape):
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_b(sm, hip, Nx, Nt, U)
    L = sm.Lattice(Nx, Nt)
    its = []
    try:
        upload(sm, L, U)
        x, res = batch(sm, L, [np.array(c) for c in cols], 1e-10, 10000)
        for b, phi in enumerate(cols):
            phi = np.array(phi)
            xl, rl = lone(sm, hip, L, phi, 1e-10, 10000)
            rel = np.linalg.norm(x[b] - xl) / np.linalg.norm(xl)
            true_r = np.linalg.norm(phi - eo_dhat(sm, L, eo_dhat(sm, L, x[b], 1), 0)) / np.linalg.norm(phi)
            print(f"EO BATCH SOLVE {Nx}x{Nt} column {b}: iterations {res[b].iterations} (lone {rl.iterations}) "
                  f"deviation {rel:.3e} true residual {true_r:.3e}")
            assert rl.converged == 1 and res[b].converged == 1, b
            assert abs(res[b].iterations - rl.iterations) <= max(1, rl.iterations // 100), (b, res[b].iterations,
                                                                                          rl.iterations)
            assert rel <= 1e-10, (b, rel)
            assert true_r < 1e-10, (b, true_r)
            assert np.all(x[b] - even(x[b], Nx, Nt) == 0.0)  # exactly zero on the odd sites
            assert res[b].residual < 1e-10 * res[b].phi_norm
            assert res[b].phi_norm == pytest.approx(np.linalg.norm(phi), rel=1e-13)
            its.append(res[b].iterations)
    finally:
        L.close()
    # the (Dhat Dhat^dag)^-2 source stops earlier than the random ones (16x16: 64 against 69 for all others)
    assert len(set(its)) >= 2, its


# ---- c. column independence, bitwise -----------------------------------------------
def test_column_bits_do_not_depend_on_the_batch(sm, hip):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = [np.array(c) for c in columns_b(sm, hip, Nx, Nt, U)]
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
        perm = [3, 0, 4, 2, 1]  # a permutation that is no rotation
        xp, rp = batch(sm, L, [cols[p] for p in perm], 1e-10, 10000)
        for pos, p in enumerate(perm):
            assert same(xp[pos], rp[pos], x5[p], r5[p]), pos
        # next to an all-zero column (alpha = 0 / 0 there: it runs to max_iter) and a column that hits
        # max_iter while its neighbour converges
        its = [r.iterations for r in r5]
        fast, slow = int(np.argmin(its)), int(np.argmax(its))
        cap = its[fast] + 1
        assert its[slow] > cap, its
        z = np.zeros_like(cols[0])
        lone_cap = [batch(sm, L, [cols[b]], 1e-10, cap) for b in (fast, slow)]
        xz, rz = batch(sm, L, [cols[fast], z, cols[slow]], 1e-10, cap)
        assert same(xz[0], rz[0], lone_cap[0][0][0], lone_cap[0][1][0])
        assert same(xz[2], rz[2], lone_cap[1][0][0], lone_cap[1][1][0])
        assert rz[0].converged == 1 and same(xz[0], rz[0], x5[fast], r5[fast])
        assert rz[2].converged == 0 and rz[2].iterations == cap
        assert rz[1].converged == 0 and rz[1].phi_norm == 0.0
        # the zero column's NaNs stay in its own slot: the next batch has the first one's bits
        x5c, r5c = batch(sm, L, cols, 1e-10, 10000)
        assert bits_equal(x5, x5c) and [rtuple(r) for r in r5] == [rtuple(r) for r in r5c]
    finally:
        L.close()


def test_column_bits_at_the_largest_batch(sm):
    Nx, Nt = 6, 10
    U, _ = mm.synthetic(sm, Nx, Nt)
    kmax = sm.lib.sm_cg_batch_max()
    assert kmax == 64
    cols = [even(spinor(sm, Nx, Nt, 100 + b), Nx, Nt) for b in range(kmax)]
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


def test_regrowth_keeps_the_bits(sm):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = [even(spinor(sm, Nx, Nt, 10 + b), Nx, Nt) for b in range(9)]
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


@pytest.mark.parametrize("shape", [(130, 72), (516, 8), (130, 962)], ids=["130x72", "516x8", "130x962"])
def test_column_bits_do_not_depend_on_the_tile_height(sm, shape):
    """The tile height follows K and the tile target (SM_TEST_OPTS
    eo_batch_tiles); the partial sums are kept per granule, so neither moves a bit."""
    Nx, Nt = shape
    U, _ = mm.synthetic(sm, Nx, Nt)
    cols = columns_a(sm, Nx, Nt)
    out = []
    for tiles in (0, 8, 40):
        with opts_env(**({"eo_batch_tiles": tiles} if tiles else {})):
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
def test_other_solvers_do_not_notice(sm, hip):
    Nx, Nt = 32, 48
    S = Nx * Nt
    U, phi = mm.synthetic(sm, Nx, Nt)
    cols = [even(spinor(sm, Nx, Nt, 1), Nx, Nt), even(spinor(sm, Nx, Nt, 2), Nx, Nt), point_even(Nx, Nt, 3, 5, 1)]
    fcols = [spinor(sm, Nx, Nt, 3), spinor(sm, Nx, Nt, 4)]
    phie = even(phi, Nx, Nt)

    def eo_cg(L):
        x = np.empty(4 * S)
        res = sm.CGResult()
        sm.check(sm.lib.sm_eo_cg(L.ctx, ptr(phie[:2 * S]), ptr(phie[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), M0, 1e-10,
                                 10000, ctypes.byref(res)))
        return x, res

    def stepwise(L, with_batch):
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

        def between():
            if with_batch:
                batch(sm, L, cols, 1e-10, 10000)

        try:
            upload(sm, L, U)
            for solver in (lambda: sm_cg(sm, L, phi, 1e-10, 10000), lambda: eo_cg(L)):
                out.append(solver())
                between()
                out.append(solver())
            L.eo_cg_precision("mixed")
            out.append(eo_cg(L))
            between()
            out.append(eo_cg(L))
            L.eo_cg_precision("double")
            xb, rb = full_batch(sm, L, fcols, 1e-10, 10000)
            out.append((xb, rb[0]))
            between()
            xb, rb = full_batch(sm, L, fcols, 1e-10, 10000)
            out.append((xb, rb[0]))
            out.append(stepwise(L, with_batch))
        finally:
            L.close()
        return out

    plain, with_eob = run(False), run(True)
    assert len(plain) == len(with_eob) == 9
    for i, ((xa, ra), (xb, rb)) in enumerate(zip(plain, with_eob)):
        assert same(xa, ra, xb, rb), i


# ---- e. gauge changes ----------------------------------------------------------------
def test_gauge_changes_need_no_call(sm):
    Nx, Nt = 16, 16
    U, _ = mm.synthetic(sm, Nx, Nt)
    U2, _ = mm.synthetic(sm, Nx, Nt, gauge_seed=99)
    cols = [even(spinor(sm, Nx, Nt, 1), Nx, Nt), point_even(Nx, Nt, 0, 0, 0), even(spinor(sm, Nx, Nt, 2), Nx, Nt)]

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
        for eo in (0, 1):  # a short, finely stepped trajectory is accepted (dH ~ 1e-4)
            p = sm.HMCParams(M0, 2.0, 0.1, 20, 1e-10, 10000, 2024, eo)
            sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(p), eo, ctypes.byref(r)))
            assert r.accepted == 1, (r.dH, r.r)
            check_against_fresh(L, f"accepted trajectory, even_odd = {eo}")
    finally:
        L.close()


# ---- f. refusals ---------------------------------------------------------------------
def test_refusals(sm, hip):
    Nx, Nt = 8, 8
    U, phi = mm.synthetic(sm, Nx, Nt)
    phi = even(phi, Nx, Nt)
    kmax = sm.lib.sm_cg_batch_max()
    L = sm.Lattice(Nx, Nt)
    try:
        batch(sm, L, [phi], 1e-10, 100, expect=SM_ERR_STATE)  # no gauge field yet
        upload(sm, L, U)
        res = (sm.CGResult * (kmax + 1))()
        big = np.zeros((kmax + 1, 4 * L.V))
        out = np.zeros_like(big)
        f = sm.lib.sm_eo_cg_batch
        assert f(L.ctx, 0, ptr(big), ptr(out), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert f(L.ctx, kmax + 1, ptr(big), ptr(out), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert f(L.ctx, 1, None, ptr(out), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert f(L.ctx, 1, ptr(big), None, M0, 1e-10, 100, res) == SM_ERR_ARG
        assert f(L.ctx, 1, ptr(big), ptr(out), M0, 1e-10, 100, None) == SM_ERR_ARG
        assert f(L.ctx, 1, ptr(big), ptr(big), M0, 1e-10, 100, res) == SM_ERR_ARG
        assert f(L.ctx, 1, ptr(big), ptr(out), M0, 1e-10, -1, res) == SM_ERR_ARG
        dphi = hip.upload(phi)
        assert sm.lib.sm_eo_cg_batch_dev(L.ctx, 1, dphi, dphi, M0, 1e-10, 100, res) == SM_ERR_ARG
        assert b"alias" in sm.lib.sm_last_error()
        # still usable; host entry, device entry and the package agree bitwise
        xh, rh = batch(sm, L, [phi], 1e-10, 10000)
        assert rh[0].converged == 1
        dx = hip.alloc(phi.nbytes)
        sm.check(sm.lib.sm_eo_cg_batch_dev(L.ctx, 1, dphi, dx, M0, 1e-10, 10000, res))
        assert same(hip.download(dx, phi), res[0], xh[0], rh[0])
        hip.free(dphi)
        hip.free(dx)
        xp, rp = L.eo_cg_batch(phi.view(np.complex128).reshape(1, 2, L.V), M0, tol=1e-10, max_iter=10000)
        assert same(xp.view(np.float64).reshape(-1), rp[0], xh[0], rh[0])
    finally:
        L.close()
    for shape in ((7, 8), (8, 7)):  # no checkerboard on an odd periodic lattice
        O = sm.Lattice(*shape)
        try:
            Uo, po = mm.synthetic(sm, *shape)
            upload(sm, O, Uo)
            batch(sm, O, [po], 1e-10, 100, expect=SM_ERR_ARG)
            assert b"even" in sm.lib.sm_last_error()
            assert sm_cg(sm, O, po, 1e-10, 10000)[1].converged == 1
        finally:
            O.close()
    B = sm.Lattice(Nx, Nt, loopback=True)
    try:
        upload(sm, B, U)
        batch(sm, B, [phi], 1e-10, 100, expect=SM_ERR_ARG)
        assert sm_cg(sm, B, phi, 1e-10, 10000)[1].converged == 1
    finally:
        B.close()
