"""The Dirac apply under every launch geometry sm_tune offers, bitwise against the oracle.

The rest of the suite runs the apply at the one geometry dslash_config picks for
a shape. Here every stencil variant (0: one-row lookahead, 1: two-row lookahead,
2: the same capped at 168 VGPRs), both tile orders (xcd_remap 0 / 1), every
block width and chunk lengths from 1 row (shorter than the lookahead) to more
than the lattice run D, D^dag and D D^dag into caller device buffers that hold a
NaN pattern, and the result must be the oracle's bits: a tile no block wrote
keeps the pattern, a tile marched wrongly differs.

Shapes (Nx x Nt): 5x9 is less than a wave; 12x70 has a 6-column second block at
bt = 64; 9x200 has TB = 4, 2, 2, 1 t-blocks for bt = 64, 128, 192, 256; 37x130
puts the tile count off every multiple of 8 (the remap's q / r split); 6x257 has
a one-column last block at bt = 256.

bt = 192 (three waves) is bitwise under the same sweep, so the header lists it
next to 64, 128 and 256; other widths are refused.

The t-shard apply splits into an interior launch and a wrapped edge launch
(t-blocks TB-1 and 0) from TB = 3; the RCCL loopback cases run it at TB = 3 and
4 with a last block of 2 and of 1 columns, and unsplit (TB = 2) as the control.

The six-launch CG takes <d, Ad> from the apply's dot epilogue, one partial per
tile; it is held to oracle_cg by the bar of test_gpu_parity.py under the same
geometries.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal, opts_env, ptr
from hiprt import Hip, poisoned

pytestmark = pytest.mark.gpu

M0 = -0.07
SIGMA = 0.4242
SM_ERR_ARG = 1
BTS = (64, 128, 256)
SHAPES = [(5, 9, SIGMA), (12, 70, SIGMA), (9, 200, SIGMA), (37, 130, SIGMA), (6, 257, SIGMA), (37, 130, -1.0)]
SHAPE_IDS = ["5x9", "12x70", "9x200", "37x130", "6x257", "37x130_hot"]


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


_CASES = {}


def case(sm, oracle, Nx, Nt, sigma):
    """Fields of a shape and the oracle's D psi, D^dag psi, D D^dag psi (built once)."""
    key = (Nx, Nt, sigma)
    if key not in _CASES:
        S = Nx * Nt
        U, psi = np.empty(4 * S), np.empty(4 * S)
        sm.lib.sm_fill_gauge(4321, sigma, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
        sm.lib.sm_fill_spinor(5678, Nt, 0, Nx, 0, Nt, ptr(psi[:2 * S]), ptr(psi[2 * S:]))

        def D(v, dag):
            o = np.empty(4 * S)
            oracle.oracle_dirac(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(v[:2 * S]), ptr(v[2 * S:]),
                                ptr(o[:2 * S]), ptr(o[2 * S:]), M0, dag)
            return o

        ref = {"D": D(psi, 0), "Ddag": D(psi, 1)}
        ref["DDdag"] = D(ref["Ddag"], 0)
        for a in (U, psi, *ref.values()):
            a.setflags(write=False)
        _CASES[key] = (U, psi, ref)
    return _CASES[key]


class Device:
    """A context with U uploaded and psi / one output buffer resident."""

    def __init__(self, sm, Nx, Nt, U, psi, loopback=False, **opts):
        self.sm, self.S = sm, Nx * Nt
        with opts_env(**opts):
            self.L = sm.Lattice(Nx, Nt, loopback=loopback)
        self.hip = Hip()
        self.dU, self.dpsi = self.hip.upload(U), self.hip.upload(psi)
        self.dout = self.hip.malloc(8 * 4 * self.S)
        sm.check(sm.lib.sm_upload_gauge_dev(self.L.ctx, self.dU))
        sm.check(sm.lib.sm_synchronize(self.L.ctx))

    def run(self, which):
        """One operator into the poisoned output buffer; returns it downloaded."""
        sm, c = self.sm, self.L.ctx
        self.hip.poison(self.dout, 4 * self.S)
        if which == "DDdag":
            sm.check(sm.lib.sm_ddag_dev(c, self.dpsi, self.dout, M0))
        else:
            sm.check(sm.lib.sm_dirac_dev(c, self.dpsi, self.dout, M0, 1 if which == "Ddag" else 0))
        return self.hip.download(self.dout, np.empty(4 * self.S))

    def check_ops(self, ref, tag, bad):
        for which in ("D", "Ddag", "DDdag"):
            out = self.run(which)
            if not bits_equal(out, ref[which]):
                bad.append((tag, which, poisoned(out), int(np.count_nonzero(out.view(np.uint64)
                                                                             != ref[which].view(np.uint64)))))

    def close(self):
        self.hip.free_all()
        self.L.close()


def sweep(sm, oracle, Nx, Nt, sigma, bts):
    U, psi, ref = case(sm, oracle, Nx, Nt, sigma)
    dev = Device(sm, Nx, Nt, U, psi)
    bad, n = [], 0
    try:
        for bt in bts:
            for variant in (0, 1, 2):
                for remap in (0, 1):
                    for xchunk in (1, 2, 3, Nx - 1, Nx, Nx + 5):
                        sm.check(sm.lib.sm_tune(dev.L.ctx, bt, xchunk, remap, variant))
                        dev.check_ops(ref, (bt, variant, remap, xchunk), bad)
                        n += 1
    finally:
        dev.close()
    # (geometry, operator, words still poisoned, words that differ)
    assert not bad, (len(bad), bad[:8])
    return n


@pytest.mark.parametrize("Nx,Nt,sigma", SHAPES, ids=SHAPE_IDS)
def test_geometry_sweep_bitwise_vs_oracle(sm, oracle, Nx, Nt, sigma):
    """bt x variant x xchunk = 54 geometries under each tile order (xcd_remap 0 / 1),
    108 in all; D, D^dag and D D^dag each."""
    assert sweep(sm, oracle, Nx, Nt, sigma, BTS) == 108


@pytest.mark.parametrize("Nx,Nt,sigma", SHAPES, ids=SHAPE_IDS)
def test_bt192_sweep_bitwise_vs_oracle(sm, oracle, Nx, Nt, sigma):
    """Three-wave blocks: sm_tune accepts bt = 192 and the header lists it."""
    assert sweep(sm, oracle, Nx, Nt, sigma, (192,)) == 36


def test_sm_tune_refusals_keep_the_configuration(sm, oracle):
    Nx, Nt = 12, 70
    U, psi, ref = case(sm, oracle, Nx, Nt, SIGMA)
    dev = Device(sm, Nx, Nt, U, psi)
    c = dev.L.ctx
    bad = []
    try:
        sm.check(sm.lib.sm_tune(c, 128, 3, 0, 0))
        for bt in (32, 96, 320):
            # the other arguments are valid and differ from the current setting
            assert sm.lib.sm_tune(c, bt, 5, 1, 2) == SM_ERR_ARG, bt
            assert b"bt=" in sm.lib.sm_last_error()
            dev.check_ops(ref, ("refused", bt), bad)
        assert sm.lib.sm_tune(None, 64, 1, 0, 0) == SM_ERR_ARG
        # zero and negative arguments keep the current setting
        for args in ((0, 0, -1, -1), (-64, -3, -1, -1), (0, 2, -1, 1), (64, 0, 1, -1)):
            sm.check(sm.lib.sm_tune(c, *args))
            dev.check_ops(ref, ("kept", args), bad)
    finally:
        dev.close()
    assert not bad, bad


def oracle_cg(oracle, Nx, Nt, U, psi, tol=1e-10, max_iter=10000):
    S = Nx * Nt
    x = np.empty(4 * S)
    it, err = ctypes.c_int(), ctypes.c_double()
    conv = oracle.oracle_cg(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(psi[:2 * S]), ptr(psi[2 * S:]),
                            ptr(x[:2 * S]), ptr(x[2 * S:]), M0, tol, max_iter, ctypes.byref(it), ctypes.byref(err))
    assert conv == 1
    return x, it.value


def host_cg(sm, L, S, psi):
    x = np.empty(4 * S)
    res = sm.CGResult()
    sm.check(sm.lib.sm_cg(L.ctx, ptr(psi[:2 * S]), ptr(psi[2 * S:]), ptr(x[:2 * S]), ptr(x[2 * S:]), M0, 1e-10,
                          10000, ctypes.byref(res)))
    return x, res


def cg_bar(x, res, xr, itr):
    """The bar of test_gpu_parity.py; returns what missed it."""
    rel = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    ok = (res.converged == 1 and abs(res.iterations - itr) <= max(1, itr // 100) and rel <= 1e-12
          and res.residual < 1e-10 * res.phi_norm)
    return None if ok else (res.converged, res.iterations, itr, float(rel), res.residual, res.phi_norm)


def test_dot_epilogue_cg_under_geometries(sm, oracle):
    """The six-launch CG: alpha's <d, Ad> is summed from the apply's per-tile partials."""
    Nx, Nt = 37, 130
    S = Nx * Nt
    U, psi, _ = case(sm, oracle, Nx, Nt, SIGMA)
    xr, itr = oracle_cg(oracle, Nx, Nt, U, psi)
    L = sm.Lattice(Nx, Nt)
    bad = []
    try:
        sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
        sm.check(sm.lib.sm_tune_cg(L.ctx, 0, 0))
        for bt in BTS + (192,):
            for variant in (0, 1, 2):
                for remap in (0, 1):
                    for xchunk in (1, 7, Nx + 5):
                        sm.check(sm.lib.sm_tune(L.ctx, bt, xchunk, remap, variant))
                        x, res = host_cg(sm, L, S, psi)
                        miss = cg_bar(x, res, xr, itr)
                        if miss:
                            bad.append(((bt, variant, remap, xchunk), miss))
    finally:
        L.close()
    assert not bad, bad[:8]


# (Nx, Nt, bt): TB = 3 with a 2-column last block; TB = 4; TB = 3 with a
# 1-column last block; TB = 2, which the split leaves as one launch
SPLIT_CASES = [(8, 130, 64), (8, 200, 64), (6, 257, 128), (8, 130, 128)]


@pytest.mark.parametrize("sigma", [SIGMA, -1.0], ids=["gauss", "hot"])
@pytest.mark.parametrize("Nx,Nt,bt", SPLIT_CASES, ids=["8x130_bt64", "8x200_bt64", "6x257_bt128", "8x130_bt128"])
def test_tshard_split_edges_bitwise_vs_oracle(sm, oracle, Nx, Nt, bt, sigma):
    """Interior launch over t-blocks 1..TB-2, edge launch over TB-1 and 0 (wrapped) behind
    the faces: every column written once, with the projected faces on the edge lanes."""
    U, psi, ref = case(sm, oracle, Nx, Nt, sigma)
    dev = Device(sm, Nx, Nt, U, psi, loopback=True, apply_split=1)
    bad = []
    try:
        for remap in (0, 1):
            for xchunk in (1, 3):
                sm.check(sm.lib.sm_tune(dev.L.ctx, bt, xchunk, remap, -1))
                dev.check_ops(ref, (bt, remap, xchunk), bad)
    finally:
        dev.close()
    assert not bad, bad


def test_tshard_split_dot_epilogue_cg(sm, oracle):
    """8x200 at bt = 64 (TB = 4): the partials of one apply come from two launches."""
    Nx, Nt, bt = 8, 200, 64
    S = Nx * Nt
    U, psi, _ = case(sm, oracle, Nx, Nt, SIGMA)
    xr, itr = oracle_cg(oracle, Nx, Nt, U, psi)
    got = {}
    for loop in (False, True):
        with opts_env(apply_split=1):
            L = sm.Lattice(Nx, Nt, loopback=loop)
        try:
            sm.check(sm.lib.sm_upload_gauge(L.ctx, ptr(U[:2 * S]), ptr(U[2 * S:])))
            sm.check(sm.lib.sm_tune_cg(L.ctx, 0, 0))
            for remap in (0, 1):
                sm.check(sm.lib.sm_tune(L.ctx, bt, 3, remap, -1))
                got[(loop, remap)] = host_cg(sm, L, S, psi)
        finally:
            L.close()
    for remap in (0, 1):
        (x1, r1), (xl, rl) = got[(False, remap)], got[(True, remap)]
        assert cg_bar(x1, r1, xr, itr) is None, cg_bar(x1, r1, xr, itr)
        assert cg_bar(xl, rl, xr, itr) is None, cg_bar(xl, rl, xr, itr)
        assert rl.iterations == r1.iterations, (rl.iterations, r1.iterations)
        rel = np.linalg.norm(xl - x1) / np.linalg.norm(x1)
        assert rel <= 1e-13, rel
