"""Caller streams (sm_set_stream) and the streaming kernel (sm_bench_stream).

sm_set_stream is the documented hand-off to a caller's stream (torch's current
stream, say): everything the context enqueues afterwards must run there, so
synchronising THAT stream alone must be enough to read the results. The same
calls on the context's own stream must give the same bits, and the operators the
oracle's.

sm_bench_stream is the roofline reference bench.py divides by: out = a + b or
out = a over n complex elements in block-contiguous chunks, for any n and block
count, writing nothing past n.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal, ptr
from hiprt import POISON, Hip, poisoned

pytestmark = pytest.mark.gpu

SM_ERR_ARG = 1
M0 = -0.07


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def test_set_stream_runs_on_the_callers_stream(sm, oracle):
    Nx, Nt = 12, 70
    S = Nx * Nt
    U, psi, chi = np.empty(4 * S), np.empty(4 * S), np.empty(4 * S)
    sm.lib.sm_fill_gauge(4321, 0.4242, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
    sm.lib.sm_fill_spinor(5678, Nt, 0, Nx, 0, Nt, ptr(psi[:2 * S]), ptr(psi[2 * S:]))
    sm.lib.sm_fill_spinor(91011, Nt, 0, Nx, 0, Nt, ptr(chi[:2 * S]), ptr(chi[2 * S:]))
    h = lambda a: (ptr(a[:2 * S]), ptr(a[2 * S:]))  # noqa: E731

    ref = {k: np.empty(4 * S) for k in ("D", "Ddag", "DDdag")}
    oracle.oracle_dirac(Nx, Nt, *h(U), *h(psi), *h(ref["D"]), M0, 0)
    oracle.oracle_dirac(Nx, Nt, *h(U), *h(psi), *h(ref["Ddag"]), M0, 1)
    oracle.oracle_dirac(Nx, Nt, *h(U), *h(ref["Ddag"]), *h(ref["DDdag"]), M0, 0)
    ref["F"] = np.empty(2 * S)
    oracle.oracle_force(Nx, Nt, *h(U), *h(psi), *h(chi), ptr(ref["F"][:S]), ptr(ref["F"][S:]))

    L = sm.Lattice(Nx, Nt)
    c = L.ctx
    hip = Hip()
    dU, dpsi, dchi = hip.upload(U), hip.upload(psi), hip.upload(chi)
    sizes = {"D": 4 * S, "Ddag": 4 * S, "DDdag": 4 * S, "F": 2 * S, "x": 4 * S}
    dev = {k: hip.malloc(8 * n) for k, n in sizes.items()}

    def run_set(sync):
        """Every device entry point once, into poisoned buffers; `sync` waits for them."""
        for k, n in sizes.items():
            hip.poison(dev[k], n)
        sm.check(sm.lib.sm_upload_gauge_dev(c, dU))
        sm.check(sm.lib.sm_dirac_dev(c, dpsi, dev["D"], M0, 0))
        sm.check(sm.lib.sm_dirac_dev(c, dpsi, dev["Ddag"], M0, 1))
        sm.check(sm.lib.sm_ddag_dev(c, dpsi, dev["DDdag"], M0))
        sm.check(sm.lib.sm_force_dev(c, dpsi, dchi, dev["F"]))
        sm.check(sm.lib.sm_cg_begin(c, dpsi, dev["x"], M0, 1e-10))
        sm.check(sm.lib.sm_cg_iterate(c, 20))
        res = sm.CGResult()
        sm.check(sm.lib.sm_cg_finish(c, ctypes.byref(res)))
        sync()
        out = {k: hip.download(dev[k], np.empty(n), sync=False) for k, n in sizes.items()}
        return out, res.iterations

    stream = hip.stream_create()
    try:
        assert sm.lib.sm_set_stream(None, stream) == SM_ERR_ARG
        sm.check(sm.lib.sm_set_stream(c, stream))
        mine, it_mine = run_set(lambda: hip.stream_synchronize(stream))   # that stream alone
        sm.check(sm.lib.sm_set_stream(c, None))
        own, it_own = run_set(lambda: sm.check(sm.lib.sm_synchronize(c)))
        sm.check(sm.lib.sm_set_stream(c, stream))                         # the switch is repeatable
        again, it_again = run_set(lambda: hip.stream_synchronize(stream))
    finally:
        sm.check(sm.lib.sm_set_stream(c, None))   # before the stream goes
        hip.stream_destroy(stream)
        hip.free_all()
        L.close()

    assert it_mine == it_own == it_again and it_own > 0
    for k in sizes:
        assert poisoned(mine[k]) == 0 and poisoned(own[k]) == 0, k
        assert bits_equal(mine[k], own[k]), k
        assert bits_equal(again[k], own[k]), k
    for k in ref:
        assert bits_equal(own[k], ref[k]), k
    # the CG iterate after as many iterations, by the bar of test_gpu_parity.py
    xr = np.empty(4 * S)
    it, e = ctypes.c_int(), ctypes.c_double()
    oracle.oracle_cg(Nx, Nt, *h(U), *h(psi), *h(xr), M0, 1e-10, it_own, ctypes.byref(it), ctypes.byref(e))
    assert it.value == it_own
    assert np.linalg.norm(own["x"] - xr) / np.linalg.norm(xr) <= 1e-12


@pytest.mark.parametrize("blocks", [0, 1, 7])
@pytest.mark.parametrize("n", [1, 255, 1023, 4097, 300001])
def test_bench_stream_copies_and_adds(sm, n, blocks):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(2 * n), rng.standard_normal(2 * n)
    L = sm.Lattice(8, 8)
    c = L.ctx
    hip = Hip()
    try:
        da, db = hip.upload(a), hip.upload(b)
        dout = hip.malloc(8 * 2 * (n + 1))
        for two, want in ((1, a + b), (0, a)):
            hip.poison(dout, 2 * (n + 1))
            sm.check(sm.lib.sm_bench_stream(c, two, n, da, db, dout, blocks))
            sm.check(sm.lib.sm_synchronize(c))
            out = hip.download(dout, np.empty(2 * (n + 1)), sync=False)
            assert bits_equal(out[:2 * n], want), (two, int(np.count_nonzero(out[:2 * n] != want)))
            assert (out[2 * n:].view(np.uint64) == POISON).all(), two
        # out = a needs no b
        hip.poison(dout, 2 * (n + 1))
        sm.check(sm.lib.sm_bench_stream(c, 0, n, da, None, dout, blocks))
        sm.check(sm.lib.sm_synchronize(c))
        assert bits_equal(hip.download(dout, np.empty(2 * (n + 1)), sync=False)[:2 * n], a)
        assert sm.lib.sm_bench_stream(c, 1, n, None, db, dout, blocks) == SM_ERR_ARG
        assert sm.lib.sm_bench_stream(c, 1, n, da, db, None, blocks) == SM_ERR_ARG
        assert sm.lib.sm_bench_stream(c, 1, n, da, None, dout, blocks) == SM_ERR_ARG
        assert sm.lib.sm_bench_stream(None, 1, n, da, db, dout, blocks) == SM_ERR_ARG
    finally:
        hip.free_all()
        L.close()
