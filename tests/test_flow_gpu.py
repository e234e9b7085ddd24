"""sm_topology / sm_wilson_flow and their ensemble forms against the host model of
tests/flow_model.py, and their bitwise properties.

Inputs are the model's charge-Q backgrounds with Gaussian link noise (fm.CASES; hot
starts are no valid input: flow drives some of their plaquettes through -1, where the
charge hangs on the last bit). Before anything is asked of the device each test
asserts on the model alone that every plaquette angle of the double model stays at
least 1e-3 from +-pi at every measured point, and that numpy.longdouble is wider
than double.

Against the model.
  charge   nint(q_geo) == Q exactly; q_geo and q_sin within 1e-14 V of the model's
           (the plaquettes are the model's bits; atan2 differs by a few ulp of pi,
           and the sums run in another order); action against oracle_plaquette_sums at
           beta = 1 within test_quenched_gpu.py's 1e-13 max(1, |ref|) + 1e-13 V.
  field    every component of the flowed field within allowed = 32 * delta_ref of the
           double model's, delta_ref being the double model's largest component
           deviation from the same recurrence in numpy.longdouble over the same
           steps: computed here on the CPU, the code under test has no part in it. A
           few ulp per sincos, 3 nsteps link updates, feedback through the force: the
           rule and the factor of the quenched test.
  series   at every point k >= 1 |d action|, 2 pi |d q_geo| and 2 pi |d q_sin| within
           8 V allowed + 1e-13 V (a plaquette is a product of four links, each within
           allowed), nint(q_geo) == Q, and the device's action strictly decreasing.
The 1025 x 1030 case (topology and one step: the stage launch's grid-stride loop
runs twice) takes delta_ref from rows 3..66 of a 70-row window of the field, on which
both models are exactly the full lattice's (a step reaches three sites): a maximum
over fewer links, so no larger than the full one.

Measured on an MI355X (ROCm 7.2), deviation / allowed of the flowed field
(deviation, delta_ref):
    2x8     eps 0.05, 10 steps: 0.0000 (0, 7.7e-16)      4x4   eps 0.1,  10 steps: 0.0000 (0, 6.9e-16)
    5x9     eps 0.05, 20 steps: 0.0056 (2.2e-16, 1.2e-15) 6x10  eps 0.1,  10 steps: 0.0000 (0, 7.6e-16)
    16x16   eps 0.02, 30 steps: 0.0000 (0, 1.5e-15)      37x130 eps 0.05, 10 steps: 0.0059 (2.2e-16, 1.2e-15)
    1025x1030 eps 0.05, 1 step: 0.0173 (2.2e-16, 4.0e-16)
Four of the seven flowed fields are the double model's bit for bit; the others differ
in one ulp of a component. The worst ratio, 0.0173, is recorded in DESIGN.md section
6.4. The series' worst deviations: |d action| 7.3e-12 against a bound of 2.1e-7
(1025x1030), 5.7e-14 against 1.4e-9 (37x130); the charges within 3.4e-14.

Bitwise: the ensemble's replica against a lone context (R = 1; R = 5 at positions 0
and 4 among other fields), repeated calls, nsteps = 0 against sm_topology, a
meas_every = 1 series against the meas_every = 5 one, sm_topology on an RCCL loopback
context against the one-shard context. A flow is a measurement: the downloaded
fields, a trajectory (lone; ensemble, plain and even-odd) and a batched solve after a
flow are bitwise those without it.
"""
import ctypes
import functools

import numpy as np
import pytest

import flow_model as fm
from conftest import bits_equal, ptr

pytestmark = pytest.mark.gpu
SM_ERR_ARG, SM_ERR_STATE = 1, 4
TWO_PI = 2.0 * np.pi


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


@functools.lru_cache(maxsize=None)
def reference(case):
    """The model's side of a case, computed once and shared (read-only): the start
    field, delta_ref up to each step, the double model's fields and their sums."""
    Nx, Nt, Q, seed, eps, nsteps, _ = case
    U = fm.background(Nx, Nt, Q, seed)
    deltas, fields = fm.delta_ref(U, eps, nsteps)
    tops = [fm.topology(f) for f in fields]
    for a in [U] + fields:
        a.setflags(write=False)
    return U, deltas, fields, tops


def model_is_a_valid_input(tops, steps):
    assert np.finfo(np.longdouble).eps < 1e-18, "numpy.longdouble is no wider than double here"
    for s in steps:
        assert tops[s][3] >= 1e-3, f"a plaquette angle of the model is {tops[s][3]} from +-pi after step {s}"


def flat(U):
    """(2, Nx, Nt) -> (2, V), site n = x * Nt + t."""
    return np.ascontiguousarray(U).reshape(2, -1)


def lone(sm, Nx, Nt, U, loopback=False):
    L = sm.Lattice(Nx, Nt, loopback=loopback)
    F = flat(U)
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(F[0]), ptr(F[1])))
    return L


def download(sm, L):
    U = np.empty((2, L.V), dtype=np.complex128)
    sm.check(sm.lib.sm_download_gauge(L.ctx, ptr(U[0]), ptr(U[1])))
    return U


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bits_equal(a.view(np.float64).reshape(-1), b.view(np.float64).reshape(-1))


def same_series(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def check_charge(sm, oracle, L, U, Q, model_top):
    Nx, Nt = U.shape[1:]
    V = Nx * Nt
    t = L.topology()
    a, qg, qs, _ = model_top
    print(f"topology {Nx}x{Nt}: q_geo {float(t.q_geo)!r} (model {float(qg)!r}), q_sin {float(t.q_sin)!r} "
          f"(model {float(qs)!r}), action {float(t.action)!r} (model {float(a)!r})")
    assert t.action.shape == t.q_geo.shape == t.q_sin.shape == ()
    assert int(np.rint(t.q_geo)) == Q
    assert abs(t.q_geo - qg) <= 1e-14 * V and abs(t.q_sin - qs) <= 1e-14 * V
    F = flat(U)
    rsp, ract = ctypes.c_double(), ctypes.c_double()
    oracle.oracle_plaquette_sums(Nx, Nt, ptr(F[0]), ptr(F[1]), 1.0, ctypes.byref(rsp), ctypes.byref(ract))
    assert abs(t.action - ract.value) <= 1e-13 * max(1.0, abs(ract.value)) + 1e-13 * V, (t.action, ract.value)
    # and bitwise sm_plaquette's own sum at beta = 1
    sp, act = ctypes.c_double(), ctypes.c_double()
    sm.check(sm.lib.sm_plaquette(L.ctx, 1.0, ctypes.byref(sp), ctypes.byref(act), None))
    assert float(t.action) == act.value
    return t


@pytest.mark.parametrize("case", fm.CASES, ids=fm.CASE_IDS)
def test_charge_of_the_unflowed_field(sm, oracle, case):
    Nx, Nt, Q = case[:3]
    U, _, _, tops = reference(case)
    model_is_a_valid_input(tops, [0])
    L = lone(sm, Nx, Nt, U)
    try:
        check_charge(sm, oracle, L, U, Q, tops[0])
    finally:
        L.close()


def check_flow(Nx, Nt, Q, eps, me, series, field, deltas, fields, tops):
    """The flowed field and the series of one device flow against the model; returns deviation / allowed."""
    V = Nx * Nt
    nsteps = len(fields) - 1
    allowed = fm.ALLOWED_FACTOR * deltas[-1]
    dev = fm.max_component_deviation(field.reshape(2, Nx, Nt), fields[-1])
    print(f"flow {Nx}x{Nt} eps {eps} steps {nsteps}: deviation {dev:.3e}, delta_ref {deltas[-1]:.3e}, "
          f"allowed {allowed:.3e}, ratio {dev / allowed:.4f}")
    npts = 1 + nsteps // me
    assert series.t.shape == series.action.shape == series.q_geo.shape == series.q_sin.shape == (npts,)
    assert np.array_equal(series.t, np.arange(npts) * (me * eps))
    for k in range(npts):
        a, qg, qs, _ = tops[k * me]
        assert int(np.rint(series.q_geo[k])) == Q, (k, series.q_geo[k])
        if k == 0:
            continue
        bound = 8.0 * V * fm.ALLOWED_FACTOR * deltas[k * me] + 1e-13 * V
        d = (abs(series.action[k] - a), TWO_PI * abs(series.q_geo[k] - qg), TWO_PI * abs(series.q_sin[k] - qs))
        print(f"  point {k}: |d action| {d[0]:.3e}, 2 pi |d q_geo| {d[1]:.3e}, 2 pi |d q_sin| {d[2]:.3e}, "
              f"bound {bound:.3e}")
        assert max(d) <= bound, (k, d, bound)
    assert np.all(np.diff(series.action) < 0.0), series.action
    assert dev <= allowed, (dev, allowed)
    return dev / allowed


@pytest.mark.parametrize("case", fm.CASES, ids=fm.CASE_IDS)
def test_flow_matches_host_model(sm, case):
    Nx, Nt, Q, _, eps, nsteps, me = case
    U, deltas, fields, tops = reference(case)
    model_is_a_valid_input(tops, range(0, nsteps + 1, me))
    L = lone(sm, Nx, Nt, U)
    try:
        series, field = L.wilson_flow(eps, nsteps, me, return_field=True)
        after = download(sm, L)
    finally:
        L.close()
    check_flow(Nx, Nt, Q, eps, me, series, field, deltas, fields, tops)
    assert same_bits(after, flat(U))                                   # the context's field is untouched
    assert fm.max_component_deviation(field, flat(U)) > 1e-3           # and the flow did move the links


def test_large_lattice_one_step(sm, oracle):
    """More sites than 4096 blocks of 256: the stage kernel's grid-stride loop runs twice."""
    Nx, Nt, Q, seed, eps, nsteps, me = fm.LARGE
    assert Nx * Nt > 4096 * 256 and nsteps == 1
    U = fm.background(Nx, Nt, Q, seed, sigma=fm.LARGE_SIGMA)
    fields = fm.flow(U, eps, 1)
    tops = [fm.topology(f) for f in fields]
    model_is_a_valid_input(tops, [0, 1])
    W, edge = 70, 3
    dw, fw = fm.delta_ref(U[:, :W], eps, 1)
    inner = slice(edge, W - edge)
    assert same_bits(fw[1][:, inner], fields[1][:, inner])      # the window's interior IS the full model
    lw = fm.flow(U[:, :W], eps, 1, np.longdouble)[1]
    deltas = [0.0, fm.max_component_deviation(fw[1][:, inner], lw[:, inner])]
    assert 0.0 < deltas[1] <= dw[1]
    L = lone(sm, Nx, Nt, U)
    try:
        check_charge(sm, oracle, L, U, Q, tops[0])
        series, field = L.wilson_flow(eps, 1, 1, return_field=True)
    finally:
        L.close()
    check_flow(Nx, Nt, Q, eps, me, series, field, deltas, fields, tops)


# ---- bitwise properties ----------------------------------------------------------
def neighbours(sm, E, skip, seed):
    for r in range(E.R):
        if r != skip:
            E.fill_gauge(r, seed + r, 0.3 + 0.05 * r)


@pytest.mark.parametrize("case", [fm.CASES[0], fm.CASES[2], fm.CASES[5]],
                         ids=[fm.CASE_IDS[0], fm.CASE_IDS[2], fm.CASE_IDS[5]])
def test_replica_is_bitwise_the_lone_context(sm, case):
    Nx, Nt, Q, _, eps, nsteps, me = case
    U, _, _, tops = reference(case)
    model_is_a_valid_input(tops, range(0, nsteps + 1, me))
    F = flat(U)
    L = lone(sm, Nx, Nt, U)
    try:
        top = L.topology()
        series, field = L.wilson_flow(eps, nsteps, me, return_field=True)
        again, field2 = L.wilson_flow(eps, nsteps, me, return_field=True)
        assert same_series(series, again) and same_bits(field, field2)          # repeated calls
        assert same_series(series, L.wilson_flow(eps, nsteps, me))              # with or without the field
        zero, field0 = L.wilson_flow(eps, 0, return_field=True)                 # nsteps = 0 is sm_topology
        assert zero.action.shape == (1,) and same_bits(field0, F)
        assert same_series([z[0] for z in zero[1:]], top)
        assert same_series([s[0] for s in series[1:]], top)
        fine = L.wilson_flow(eps, nsteps, 1)                                    # every step contains every me-th
        assert fine.action.shape == (nsteps + 1,)
        assert same_series([f[::me] for f in fine], series)
        for R, pos in ((1, 0), (5, 0), (5, 4)):
            E = L.ensemble(R)
            try:
                neighbours(sm, E, pos, 40 + pos)
                E.upload_gauge(pos, F)
                et = E.topology()
                es, ef = E.wilson_flow(eps, nsteps, me, return_field=True)
                es2 = E.wilson_flow(eps, nsteps, me)
                assert es.action.shape == (R, 1 + nsteps // me) and ef.shape == (R, 2, Nx * Nt)
                assert same_series([x[pos] for x in et], top), (R, pos)
                assert same_series([x[pos] for x in es], series), (R, pos)
                assert same_bits(ef[pos], field), (R, pos)
                assert same_series(es, es2)
                if R > 1:   # the neighbours are other fields with other results
                    other = (pos + 1) % R
                    assert not same_bits(ef[other], field) and es.action[other, -1] != es.action[pos, -1]
            finally:
                E.close()
    finally:
        L.close()


def test_loopback_topology_and_flow_refusal(sm):
    case = fm.CASES[5]
    Nx, Nt, Q, _, eps, nsteps, me = case
    U, _, _, tops = reference(case)
    model_is_a_valid_input(tops, [0])
    L = lone(sm, Nx, Nt, U)
    try:
        top = L.topology()
    finally:
        L.close()
    K = lone(sm, Nx, Nt, U, loopback=True)
    try:
        assert same_series(K.topology(), top)
        p = sm._lib.FlowParams(eps, 2, 1)
        series = (sm._lib.Topo * 3)()
        assert sm.lib.sm_wilson_flow(K.ctx, ctypes.byref(p), series, None, None) == SM_ERR_ARG
        assert b"one-shard" in sm.lib.sm_last_error()
        assert same_series(K.topology(), top)
    finally:
        K.close()


def test_refusals_on_a_device(sm):
    L = sm.Lattice(4, 4)
    series = (sm._lib.Topo * 3)()
    p = sm._lib.FlowParams(0.1, 2, 1)
    try:
        assert sm.lib.sm_topology(L.ctx, series) == SM_ERR_STATE    # before a gauge upload
        assert b"gauge" in sm.lib.sm_last_error()
        assert sm.lib.sm_wilson_flow(L.ctx, ctypes.byref(p), series, None, None) == SM_ERR_STATE
        E = L.ensemble(2)
        try:
            E.fill_gauge(0, 1, 0.3)
            assert sm.lib.sm_ens_topology(E.ens, series) == SM_ERR_STATE      # replica 1 has no field
            assert sm.lib.sm_ens_wilson_flow(E.ens, ctypes.byref(p), series, None) == SM_ERR_STATE
            assert b"replica 1" in sm.lib.sm_last_error()
            E.fill_gauge(1, 2, 0.3)
            for bad in (sm._lib.FlowParams(0.0, 2, 1), sm._lib.FlowParams(0.1, -1, 1), sm._lib.FlowParams(0.1, 2, 0),
                        sm._lib.FlowParams(float("nan"), 2, 1)):
                assert sm.lib.sm_ens_wilson_flow(E.ens, ctypes.byref(bad), series, None) == SM_ERR_ARG
            assert sm.lib.sm_ens_wilson_flow(E.ens, ctypes.byref(p), None, None) == SM_ERR_ARG
            assert sm.lib.sm_ens_topology(E.ens, None) == SM_ERR_ARG
        finally:
            E.close()
        L.upload_gauge(sm.spinor.from_arrays(np.ones(16, complex), np.ones(16, complex)))
        for bad in (sm._lib.FlowParams(0.0, 2, 1), sm._lib.FlowParams(0.1, -1, 1), sm._lib.FlowParams(0.1, 2, 0)):
            assert sm.lib.sm_wilson_flow(L.ctx, ctypes.byref(bad), series, None, None) == SM_ERR_ARG
        buf = np.zeros(32)
        assert sm.lib.sm_wilson_flow(L.ctx, ctypes.byref(p), series, ptr(buf), None) == SM_ERR_ARG
        assert sm.lib.sm_wilson_flow(L.ctx, ctypes.byref(p), None, None, None) == SM_ERR_ARG
        assert sm.lib.sm_topology(L.ctx, None) == SM_ERR_ARG
        t = L.topology()                                            # the unit field: no action, no charge
        assert (float(t.action), float(t.q_geo), float(t.q_sin)) == (0.0, 0.0, 0.0)
    finally:
        L.close()


# ---- a flow is a measurement -----------------------------------------------------
def hmc_params(sm, seed, even_odd, beta=2.0, m0=0.1):
    return sm.HMCParams(m0, beta, 0.3, 4, 1e-10, 10000, seed, even_odd)


def result_tuple(r):
    return tuple(getattr(r, f) for f, _ in r._fields_)


@pytest.mark.parametrize("even_odd", [0, 1], ids=["plain", "even_odd"])
def test_trajectory_after_a_flow_is_the_trajectory_without_it(sm, even_odd):
    case = fm.CASES[3]                                    # 6 x 10: even, so the checkerboard exists
    Nx, Nt, Q, _, eps, nsteps, me = case
    U, _, _, _ = reference(case)
    F = flat(U)
    R = 3

    def run(with_flow):
        L = lone(sm, Nx, Nt, U)
        E = L.ensemble(R)
        try:
            E.upload_gauge(1, F)
            neighbours(sm, E, 1, 70)
            before = [E.download_gauge(r) for r in range(R)]
            kept = download(sm, L)
            if with_flow:
                E.wilson_flow(eps, nsteps, me, return_field=True)
                L.wilson_flow(eps, nsteps, me)
                assert all(same_bits(E.download_gauge(r), before[r]) for r in range(R))
                assert same_bits(download(sm, L), kept)
            prm = [hmc_params(sm, 11 + r, even_odd, beta=2.0 + r) for r in range(R)]
            eres = [result_tuple(r) for r in E.trajectory(prm, 5)]
            if with_flow:                                 # also between two trajectories
                E.wilson_flow(eps, 3)
            eres += [result_tuple(r) for r in E.trajectory(prm, 6)]
            lres = sm.HMCResult()
            lp = hmc_params(sm, 21, even_odd)
            sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(lp), 5, ctypes.byref(lres)))
            if with_flow:
                L.wilson_flow(eps, 3)
            lres2 = sm.HMCResult()
            sm.check(sm.lib.sm_hmc_trajectory(L.ctx, ctypes.byref(lp), 6, ctypes.byref(lres2)))
            return eres, [E.download_gauge(r) for r in range(R)], [result_tuple(lres), result_tuple(lres2)], \
                download(sm, L)
        finally:
            E.close()
            L.close()

    e0, f0, l0, u0 = run(False)
    e1, f1, l1, u1 = run(True)
    assert e0 == e1 and l0 == l1
    assert all(same_bits(a, b) for a, b in zip(f0, f1)) and same_bits(u0, u1)
    assert all(np.isfinite(r[2]) and r[7] > 0 for r in e0)   # real trajectories: a finite dH, CG iterations


def test_batched_solve_before_and_after_a_flow(sm):
    from hiprt import Hip
    case = fm.CASES[4]
    Nx, Nt, Q, _, eps, nsteps, me = case
    U, _, _, _ = reference(case)
    V, K, m0 = Nx * Nt, 3, 0.05
    rng = np.random.default_rng(5)
    phi = rng.standard_normal((K, 2, V)) + 1j * rng.standard_normal((K, 2, V))
    L = lone(sm, Nx, Nt, U)
    hip = Hip()
    try:
        dphi, dx = hip.upload(phi), hip.malloc(phi.nbytes)

        def solve():
            res = (sm.CGResult * K)()
            sm.check(sm.lib.sm_cg_batch_dev(L.ctx, K, dphi, dx, m0, 1e-10, 10000, res))
            return hip.download(dx, np.empty_like(phi)), [result_tuple(r) for r in res]

        x0, r0 = solve()
        L.wilson_flow(eps, nsteps, me)
        x1, r1 = solve()
        assert all(r[0] == 1 for r in r0)
        assert r0 == r1 and same_bits(x0, x1)
    finally:
        hip.free_all()
        L.close()
