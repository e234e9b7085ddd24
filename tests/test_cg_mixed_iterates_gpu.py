"""The fp32 CG pass (sm_cgsp.hip) and its driver (sm_cgmp.cpp) looked at
directly: iterate by iterate, at the pass's geometry edges, under every launch
geometry, across changes of U and at the ends of fp32's range.

A mixed solve cut off at max_iter = k returns x_k = phi + (the fp32 correction,
folded), the k-th CG iterate from x0 = phi -- before any reliable update or
fp64 finish can repair a wrong stencil, sign, row parity or buffer rotation.
It is compared per site with a plain fp64 CG on the oracle's D D^dag
(mixed_model.py) in the max norm relative to the correction,
    deviation <= bound = 8 max(max_k deviation(fp32 numpy model_k), 2^-23),
the bound computed per shape from the numpy model, never from the kernel;
test_mixed_model_host.py shows that a lost boundary sign, a misplaced one and
a 1e-3 rad link error each land 10x or more over it. Every case prints its
deviation, the bound and the ratio to the model's own deviation.
"""
import ctypes
import math

import numpy as np
import pytest

import mixed_model as mm
from conftest import bits_equal, opts_env, ptr

pytestmark = pytest.mark.gpu

M0 = -0.10
KS = (1, 2, 3, 4, 5, 6, 7, 12)
KMAX = max(KS)
COUNTERS = ("used", "inner_iterations", "reliable_updates", "fp64_iterations", "fell_back")


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def cg(sm, L, phi, tol, max_iter, m0=M0):
    S = L.V
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, tol,
                          max_iter, ctypes.byref(res)))
    return res, L.last_cg_mixed, x


def upload(sm, L, U):
    S = L.V
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))


def download(sm, L):
    S = L.V
    U = np.empty(4 * S)
    sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
    return U


def counters(info):
    return tuple(getattr(info, f) for f in COUNTERS)


def relres(oracle, Nx, Nt, U, phi, x):
    return np.linalg.norm(phi - mm.oracle_ddag(oracle, Nx, Nt, U, x, M0)) / np.linalg.norm(phi)


_REFS = {}


@pytest.fixture(scope="module")
def refs(sm, oracle):
    """shape -> (U, phi, fp64 iterates x_1..x_12, bound, model deviation), computed once per shape."""
    def get(shape):
        if shape not in _REFS:
            Nx, Nt = shape
            U, phi = mm.synthetic(sm, Nx, Nt)
            ref = mm.cg_iterates_fp64(oracle, Nx, Nt, U, phi, M0, KMAX)
            model = mm.cg_iterates_fp32_model(Nx, Nt, U, phi, M0, KMAX)
            for a in [U, phi] + ref:
                a.setflags(write=False)
            _REFS[shape] = (U, phi, ref, mm.bound(model, ref, phi), mm.model_deviation(model, ref, phi))
        return _REFS[shape]
    return get


def mixed_iterate(sm, L, phi, k):
    """x_k of a mixed solve cut off at max_iter = k, with everything such a solve owes checked."""
    res, info, x = cg(sm, L, phi, 0.0, k)
    assert res.iterations == k and res.converged == 0, (k, res.iterations, res.converged)
    assert info.used == 1 and info.fell_back == 0 and info.inner_iterations == k, (k, counters(info))
    assert np.all(np.isfinite(x)), k
    return x, info


# ---- a. iterates against the fp64 reference -----------------------------------
#   4x2     narrower than the halo: lanes wrap onto themselves
#   5x9     odd in both directions
#   3x56    exactly one wave; fewer rows than the prologue and the row halo
#   6x57    one column spills into a second wave
#   7x60    the second wave owns exactly a halo's width
#   13x225  4*56 + 1: a second 4-wave t-block owning one column
#   130x72  several x-chunks at the default chunk length
# mp_delta_pct 1: no reliable update inside 12 iterations (an operator error
# shows undamped); 10: the default; 99: an update after almost every pass (the
# injection with beta != 0, the fold with J = 1, 2, 3, the buffer rotation).
ALL_MODES = [(6, 57), (13, 225), (130, 72)]
CASES = [(s, 1) for s in [(4, 2), (5, 9), (3, 56), (6, 57), (7, 60), (13, 225), (130, 72)]]
CASES += [(s, m) for s in ALL_MODES for m in (10, 99)]


@pytest.mark.parametrize("shape,mode", CASES, ids=[f"{s[0]}x{s[1]}-delta{m}" for s, m in CASES])
def test_iterates_match_fp64_cg(sm, refs, shape, mode):
    Nx, Nt = shape
    U, phi, ref, bound, mdev = refs(shape)
    with opts_env(mp_delta_pct=mode):
        L = sm.Lattice(Nx, Nt)
    dev, ups, x64 = {}, {}, {}
    try:
        upload(sm, L, U)
        L.cg_precision("mixed")
        for k in KS:
            x, info = mixed_iterate(sm, L, phi, k)
            dev[k] = mm.deviation(x, ref[k - 1], phi)
            ups[k] = info.reliable_updates
        L.cg_precision("double")  # the reference itself: the library's fp64 path follows it
        for k in KS:
            r64, i64, x64[k] = cg(sm, L, phi, 0.0, k)
            assert r64.iterations == k and r64.converged == 0 and i64.used == 0
    finally:
        L.close()
    worst = max(dev.values())
    print(f"ITERATES {Nx}x{Nt} delta {mode}%: deviation " + " ".join(f"k{k}={d:.2e}" for k, d in dev.items())
          + f"; updates {list(ups.values())}; max {worst:.3e} bound {bound:.3e} model {mdev:.3e} "
          f"ratio {worst / mdev:.2f}")
    for k in KS:
        rel = np.linalg.norm(x64[k] - ref[k - 1]) / np.linalg.norm(ref[k - 1])
        assert rel <= 1e-12, (k, rel)
    for k in KS:
        assert dev[k] <= bound, (k, dev[k], bound)
        if mode == 99:
            assert ups[k] >= k // 2, (k, ups[k])


# ---- b. launch geometries of the fp32 pass --------------------------------------
# The pass takes its tile shape from the fp64 recompute-Ad pass's configuration
# (cg_sp_config), so everything that reshapes that one reshapes this one.
def geometries(Nx):
    g = {f"wpb{w}_xchunk{xc}": ({}, [("sm_tune_cg_geometry", w, xc)])
         for w, xc in [(1, 0), (2, 0), (4, 0), (1, 1), (1, 5), (4, 300)]}
    g["wpb2_xchunkNx"] = ({}, [("sm_tune_cg_geometry", 2, Nx)])
    # balanced chunks, 7 rows asked for: 13 -> 2 chunks of 6 / 7, 130 -> 19 of 6 / 7
    g["balanced_xchunk7"] = ({}, [("sm_tune_cg_geometry", 0, 7), ("sm_tune_cg_strip", -1, 1)])
    g["strip_on"] = ({}, [("sm_tune_cg_strip", 1, -1)])
    # tiles: default 14 (13x225) / 65 (130x72), neither a multiple of 8; one chunk of 4-wave blocks: 2 / 1
    for r in (0, 1):
        g[f"remap{r}_default_tiles"] = ({"ra_remap": r}, [])
        g[f"remap{r}_few_tiles"] = ({"ra_remap": r}, [("sm_tune_cg_geometry", 4, 300)])
    return g


GEOM_SHAPES = [(13, 225), (130, 72)]
GEOM_KS = (2, 3, 7)
_DEFAULT_X7 = {}


@pytest.fixture(scope="module")
def default_x7(sm, refs):
    def get(shape):
        if shape not in _DEFAULT_X7:
            U, phi = refs(shape)[:2]
            with opts_env(mp_delta_pct=1):
                L = sm.Lattice(*shape)
            try:
                upload(sm, L, U)
                L.cg_precision("mixed")
                _DEFAULT_X7[shape] = mixed_iterate(sm, L, phi, 7)[0]
            finally:
                L.close()
        return _DEFAULT_X7[shape]
    return get


@pytest.mark.parametrize("name", sorted(geometries(0)))
@pytest.mark.parametrize("shape", GEOM_SHAPES, ids=["13x225", "130x72"])
def test_launch_geometries(sm, refs, default_x7, shape, name):
    Nx, Nt = shape
    U, phi, ref, bound, mdev = refs(shape)
    opts, calls = geometries(Nx)[name]
    with opts_env(mp_delta_pct=1, **opts):
        L = sm.Lattice(Nx, Nt)
    xs = {}
    try:
        upload(sm, L, U)
        for fn, a, b in calls:
            sm.check(getattr(sm.lib, fn)(L.ctx, a, b))
        L.cg_precision("mixed")
        for k in GEOM_KS:
            xs[k] = mixed_iterate(sm, L, phi, k)[0]
    finally:
        L.close()
    dev = {k: mm.deviation(xs[k], ref[k - 1], phi) for k in GEOM_KS}
    x7 = default_x7(shape)
    gap = mm.deviation(xs[7], x7, phi)
    worst = max(dev.values())
    print(f"GEOMETRY {Nx}x{Nt} {name}: deviation " + " ".join(f"k{k}={d:.2e}" for k, d in dev.items())
          + f"; against the default geometry at k7 {gap:.2e}; bound {bound:.3e} ratio {worst / mdev:.2f}")
    for k in GEOM_KS:
        assert dev[k] <= bound, (k, dev[k], bound)
    assert gap <= bound, (gap, bound)  # the tile shape may change only the rounding order of the sums
    if name == "strip_on":  # cg_sp_config clears the strip: the very same launches
        assert bits_equal(xs[7], x7)


# ---- c. state and links -----------------------------------------------------------
TOL, MAXIT = 1e-10, 10000


def full_solve(sm, L, phi):
    res, info, x = cg(sm, L, phi, TOL, MAXIT)
    return x, res.iterations, res.converged, counters(info)


def same_solve(a, b):
    (xa, ia, ca, na), (xb, ib, cb, nb) = a, b
    assert (ia, ca, na) == (ib, cb, nb), ((ia, ca, na), (ib, cb, nb))
    assert bits_equal(xa, xb), np.abs(xa - xb).max()


@pytest.fixture(scope="module")
def base3248(sm):
    """32x48 at tol 1e-10 on a fresh context: (U, phi, solve)."""
    Nx, Nt = 32, 48
    U, phi = mm.synthetic(sm, Nx, Nt)
    L = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, U)
        L.cg_precision("mixed")
        out = full_solve(sm, L, phi)
    finally:
        L.close()
    assert out[2] == 1 and out[3][0] == 1 and out[3][4] == 0 and out[3][2] >= 1, out[1:]
    for a in (U, phi, out[0]):
        a.setflags(write=False)
    return U, phi, out


def test_repeated_mixed_solve_is_bitwise(sm, base3248):
    """Nothing of one mixed solve (y, the direction buffers and their rotation,
    the scalars) reaches the next one on the same context."""
    U, phi, fresh = base3248
    L = sm.Lattice(32, 48)
    try:
        upload(sm, L, U)
        L.cg_precision("mixed")
        a = full_solve(sm, L, phi)
        b = full_solve(sm, L, phi)
        mixed_iterate(sm, L, phi, 5)  # a cut-off solve in between leaves pending rows and a rotation behind
        c = full_solve(sm, L, phi)
    finally:
        L.close()
    print(f"repeat: iterations {a[1]} counters {a[3]}")
    same_solve(a, fresh)
    same_solve(b, a)
    same_solve(c, a)


class _Hip:
    """hipMalloc / hipMemcpy through the HIP runtime the library itself links."""

    def __init__(self):
        self.rt = ctypes.CDLL("libamdhip64.so.7")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]

    def upload(self, a):
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p

    def free(self, p):
        self.rt.hipFree(p)


def _change_by_upload(sm, L, Ub):
    upload(sm, L, Ub)


def _change_by_upload_dev(sm, L, Ub):
    hip = _Hip()
    d = hip.upload(Ub)
    try:
        sm.check(sm.lib.sm_upload_gauge_dev(L.ctx, d))
        sm.check(sm.lib.sm_synchronize(L.ctx))
    finally:
        hip.free(d)


def _change_by_fill_dev(sm, L, Ub):
    sm.check(sm.lib.sm_fill_gauge_dev(L.ctx, 99, 0.41))


# tau 4 in 2 steps: far outside the leapfrog's stable range, dH is huge
REJECT = dict(m0=0.2, beta=2.0, tau=4.0, steps=2, seed=31)


def _change_by_rejected_trajectory(sm, L, Ub):
    """The trajectory's own mixed solves convert the links of the evolving U;
    the reject puts the old U back, and the fp32 links have to follow."""
    q = REJECT
    p = sm.HMCParams(q["m0"], q["beta"], q["tau"], q["steps"], TOL, MAXIT, q["seed"], 0)
    r = sm.HMCResult()
    sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(p), 0, ctypes.byref(r)))
    print(f"trajectory: dH {r.dH:.3e} accepted {r.accepted} CG iterations {r.cg_iterations} "
          f"failures {r.cg_failures}; mixed used {L.last_cg_mixed.used}")
    assert r.accepted == 0, "precondition: the trajectory must be rejected"
    assert L.last_cg_mixed.used == 1  # its solves were mixed ones, on the evolved links


CHANGES = {"upload": _change_by_upload, "upload_dev": _change_by_upload_dev, "fill_dev": _change_by_fill_dev,
           "rejected_trajectory": _change_by_rejected_trajectory}


@pytest.mark.parametrize("how", sorted(CHANGES))
def test_fp32_links_follow_the_gauge_field(sm, how):
    """Mixed solve on U_a, change U, mixed solve: bitwise the solve of a fresh
    context given the same U (stale fp32 links would still converge -- every
    reliable update is fp64 -- but along other iterates)."""
    Nx, Nt = 32, 48
    Ua, phi = mm.synthetic(sm, Nx, Nt)
    Ub, _ = mm.synthetic(sm, Nx, Nt, sigma=0.41, gauge_seed=1234)
    L = sm.Lattice(Nx, Nt)
    F = sm.Lattice(Nx, Nt)
    try:
        upload(sm, L, Ua)
        L.cg_precision("mixed")
        first = full_solve(sm, L, phi)
        assert first[2] == 1 and first[3][0] == 1
        CHANGES[how](sm, L, Ub)
        Unow = download(sm, L)
        if how in ("upload", "upload_dev"):
            assert bits_equal(Unow, Ub)
        elif how == "rejected_trajectory":
            assert bits_equal(Unow, Ua)  # so the trajectory's converted links are the stale ones, not U_a's
        else:
            assert not np.array_equal(Unow, Ua)
        again = full_solve(sm, L, phi)
        upload(sm, F, Unow)
        F.cg_precision("mixed")
        fresh = full_solve(sm, F, phi)
    finally:
        L.close()
        F.close()
    print(f"{how}: iterations {again[1]} counters {again[3]} (fresh context {fresh[1]} {fresh[3]})")
    assert again[2] == 1
    same_solve(again, fresh)
    if how != "rejected_trajectory":
        assert not np.array_equal(again[0], first[0])


# ---- d. range edges of the fp32 side ------------------------------------------------
def test_power_of_two_scaling_commutes(sm, base3248):
    """phi 2^40: every step of the solve is homogeneous in phi and a power of
    two commutes with every rounding while nothing under- or overflows."""
    U, phi, (x, iters, conv, cnt) = base3248
    L = sm.Lattice(32, 48)
    try:
        upload(sm, L, U)
        L.cg_precision("mixed")
        xs, its, convs, cnts = full_solve(sm, L, np.ldexp(phi, 40))
    finally:
        L.close()
    print(f"2^40: iterations {its} counters {cnts} (unscaled {iters} {cnt})")
    assert (its, convs, cnts) == (iters, conv, cnt)
    assert bits_equal(xs, np.ldexp(x, 40)), np.abs(np.ldexp(xs, -40) - x).max()


@pytest.mark.parametrize("s", [127, -160], ids=["overflow", "flush_to_zero"])
def test_fp32_range_exit_finishes_in_fp64(sm, oracle, base3248, s):
    """(float) r overflows (2^127) or is zero (2^-160): the first pass's
    scalars are not finite, the driver discards y and the fp64 solver finishes."""
    U, phi = base3248[:2]
    phis = np.ldexp(phi, s)
    L = sm.Lattice(32, 48)
    try:
        upload(sm, L, U)
        L.cg_precision("mixed")
        res, info, x = cg(sm, L, phis, TOL, MAXIT)
    finally:
        L.close()
    rho = relres(oracle, 32, 48, U, phis, x) if np.all(np.isfinite(x)) else math.nan
    print(f"2^{s}: converged {res.converged} iterations {res.iterations} counters {counters(info)} relres {rho:.3e}")
    assert res.converged == 1 and info.used == 1 and info.fell_back == 1
    assert info.inner_iterations <= 1
    assert np.all(np.isfinite(x))
    assert rho < TOL


def test_fp32_residual_drifting_into_denormals(sm, oracle, base3248):
    """phi 2^-100: the fp32 residual leaves the normal range as the solve
    proceeds; whichever way the driver takes, the stop test holds in fp64."""
    U, phi = base3248[:2]
    phis = np.ldexp(phi, -100)
    L = sm.Lattice(32, 48)
    try:
        upload(sm, L, U)
        L.cg_precision("mixed")
        res, info, x = cg(sm, L, phis, TOL, MAXIT)
    finally:
        L.close()
    rho = relres(oracle, 32, 48, U, phis, x)
    print(f"2^-100: converged {res.converged} iterations {res.iterations} counters {counters(info)} relres {rho:.3e}")
    assert res.converged == 1
    assert rho < TOL
