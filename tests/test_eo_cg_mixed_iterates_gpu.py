"""The fp32 even-odd CG pass (sm_eosp.hip) and its driver (sm_eomp.cpp) looked
at directly: iterate by iterate, at the pass's geometry edges.

A mixed sm_eo_cg cut off at max_iter = k (tol 0) returns x_k = phi_e + (the fp32
correction, folded), the k-th CG iterate from x0 = phi_e -- before any reliable
update or fp64 finish can repair a wrong hop, sign, row parity or buffer
rotation. It is compared per site with a plain fp64 CG on Dhat Dhat^dag
composed from the CPU oracle's oracle_dirac and parity masks
(eo_mixed_model.py; never the GPU's own fp64 even-odd path) in the max norm
relative to the correction,
    deviation <= bound = 8 max(max_k deviation(fp32 numpy model_k), 2^-23),
the bound computed per shape from the numpy model, never from the kernel;
test_eo_mixed_model_host.py shows that a lost antiperiodic sign, a misplaced
one and a 1e-3 rad link error each land 10x or more over it. Every case prints
its deviation, the bound and the ratio to the model's own deviation.
"""
import ctypes

import numpy as np
import pytest

import eo_mixed_model as em
from conftest import opts_env, ptr

pytestmark = pytest.mark.gpu

M0 = -0.10
KS = (1, 2, 3, 4, 5, 6, 7, 12)
KMAX = max(KS)


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def eo_cg(sm, L, phi, tol, max_iter, m0=M0):
    S = L.V
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_eo_cg(L.ctx, ptr(phi[:2 * S]), ptr(phi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), m0, tol,
                             max_iter, ctypes.byref(res)))
    return res, L.last_eo_cg_mixed, x


def upload(sm, L, U):
    S = L.V
    sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))


_REFS = {}


@pytest.fixture(scope="module")
def refs(sm, oracle):
    """shape -> (U, phi_e, fp64 iterates x_1..x_12, bound, model deviation), computed once per shape."""
    def get(shape):
        if shape not in _REFS:
            Nx, Nt = shape
            U, psi = em.synthetic(sm, Nx, Nt)
            phi = em.even_part(psi, Nx, Nt)
            ref = em.cg_iterates_fp64(oracle, Nx, Nt, U, phi, M0, KMAX)
            model = em.cg_iterates_fp32_model(Nx, Nt, U, phi, M0, KMAX)
            for a in [U, phi] + ref:
                a.setflags(write=False)
            _REFS[shape] = (U, phi, ref, em.bound(model, ref, phi), em.model_deviation(model, ref, phi))
        return _REFS[shape]
    return get


# Shapes Nx x Nt, Wh = Nt / 2 k-columns per row of one parity:
#   4x6      Wh = 3: narrower than the halo, fewer rows than the march's lead-in
#   6x10     odd Wh, Nx not a multiple of 4
#   4x112    Wh = 56: exactly one wave
#   6x114    one column spills into a second wave
#   8x120    the second wave owns exactly a halo's width
#   14x450   Wh = 4*56 + 1: one column past a whole 4-wave block
#   130x72   many x-chunks (2-row chunks)
#   1026x8   16-row chunks with a 2-row last chunk
# mp_delta_pct 1: no reliable update inside 12 iterations (an operator error
# shows undamped); 10: the default; 99: an update after almost every pass (the
# injection with beta != 0, the fold after J = 1, 2, 3, the buffer rotation).
ALL_MODES = [(6, 114), (14, 450), (130, 72)]
SHAPES = [(4, 6), (6, 10), (4, 112), (6, 114), (8, 120), (14, 450), (130, 72), (1026, 8)]
CASES = [(s, 1) for s in SHAPES] + [(s, m) for s in ALL_MODES for m in (10, 99)]


@pytest.mark.parametrize("shape,mode", CASES, ids=[f"{s[0]}x{s[1]}-delta{m}" for s, m in CASES])
def test_iterates_match_fp64_cg(sm, refs, shape, mode):
    Nx, Nt = shape
    U, phi, ref, bound, mdev = refs(shape)
    odd = ~em.even_mask(Nx, Nt)
    with opts_env(mp_delta_pct=mode):
        L = sm.Lattice(Nx, Nt)
    dev, ups = {}, {}
    try:
        upload(sm, L, U)
        assert L.eo_cg_precision("mixed") == "mixed"
        for k in KS:
            res, info, x = eo_cg(sm, L, phi, 0.0, k)
            assert res.iterations == k and res.converged == 0, (k, res.iterations, res.converged)
            assert info.used == 1 and info.fell_back == 0 and info.inner_iterations == k, \
                (k, info.used, info.fell_back, info.inner_iterations)
            assert np.all(np.isfinite(x)), k
            assert np.all(em.to_planes(x, Nx, Nt)[:, odd] == 0.0), k  # the odd sites of x are exactly 0
            dev[k] = em.deviation(x, ref[k - 1], phi)
            ups[k] = info.reliable_updates
    finally:
        L.close()
    worst = max(dev.values())
    print(f"EO ITERATES {Nx}x{Nt} delta {mode}%: deviation " + " ".join(f"k{k}={d:.2e}" for k, d in dev.items())
          + f"; updates {list(ups.values())}; max {worst:.3e} bound {bound:.3e} model {mdev:.3e} "
          f"ratio {worst / mdev:.2f}")
    for k in KS:
        assert dev[k] <= bound, (k, dev[k], bound)
        if mode == 99:  # the first three updates each follow a single pass: the fold after J = 1, the rotation by 1
            assert ups[k] >= min(k, 3), (k, ups[k])
