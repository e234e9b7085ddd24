"""The gauge kernels off the fixture shapes, bitwise against the oracle.

test_md_gpu.py pins sm_plaquette, sm_staples and sm_gauge_force to the
reference on 8x8, 16x16, 32x48 and 64x64. Here they run on odd extents, on
Nt = 2 and 3 (where t+1 and t-1 wrap onto the same or the neighbouring column),
on an Nt just past a block (257), and on 1030x1040: 1 071 200 sites, more than
the 4096 x 256 threads of staple_force_kernel's grid, so its grid-stride loop
takes a second trip with a ragged tail (plaquette_kernel's smaller grid takes
four trips there). The RCCL loopback contexts read the t-neighbours from the
2-deep ghost links instead of the periodic wrap.

The plaquette field, both staple planes and the gauge force (accumulated onto a
nonzero F) must be the oracle's bits; Sp and the gauge action, which the device
sums in another order, are held to the bound of test_md_gpu.py.
"""
import ctypes

import numpy as np
import pytest

from conftest import bits_equal, ptr

pytestmark = pytest.mark.gpu

BETA = 2.3
FIELDS = [0.4242, -1.0]
FIELD_IDS = ["gauss", "hot"]


@pytest.fixture(scope="module")
def sm():
    import schwingermodel_amd
    return schwingermodel_amd


def check_gauge_kernels(sm, oracle, Nx, Nt, sigma, loopback=False):
    S = Nx * Nt
    U = np.empty(4 * S)
    sm.lib.sm_fill_gauge(4321, sigma, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
    U0, U1 = ptr(U[:2 * S]), ptr(U[2 * S:])
    F_start = np.random.default_rng(17).standard_normal(2 * S)

    ref_plaq, ref_st, ref_F = np.empty(2 * S), np.empty(4 * S), F_start.copy()
    oracle.oracle_plaquette(Nx, Nt, U0, U1, ptr(ref_plaq))
    oracle.oracle_staples(Nx, Nt, U0, U1, ptr(ref_st[:2 * S]), ptr(ref_st[2 * S:]))
    oracle.oracle_gauge_force(Nx, Nt, U0, U1, BETA, ptr(ref_F[:S]), ptr(ref_F[S:]))
    ref_sp, ref_act = ctypes.c_double(), ctypes.c_double()
    oracle.oracle_plaquette_sums(Nx, Nt, U0, U1, BETA, ctypes.byref(ref_sp), ctypes.byref(ref_act))

    L = sm.Lattice(Nx, Nt, loopback=loopback)
    try:
        sm.check(sm.lib.sm_upload_gauge(L.ctx, U0, U1))
        sp, act = ctypes.c_double(), ctypes.c_double()
        plaq = np.full(2 * S, np.nan)
        sm.check(sm.lib.sm_plaquette(L.ctx, BETA, ctypes.byref(sp), ctypes.byref(act), ptr(plaq)))
        st = np.full(4 * S, np.nan)
        sm.check(sm.lib.sm_staples(L.ctx, ptr(st[:2 * S]), ptr(st[2 * S:])))
        F = F_start.copy()
        sm.check(sm.lib.sm_gauge_force(L.ctx, BETA, ptr(F[:S]), ptr(F[S:])))
        # the sums without the field output (the path sm_hamiltonian takes)
        sp2, act2 = ctypes.c_double(), ctypes.c_double()
        sm.check(sm.lib.sm_plaquette(L.ctx, BETA, ctypes.byref(sp2), ctypes.byref(act2), None))
    finally:
        L.close()
    assert bits_equal(plaq, ref_plaq), int(np.count_nonzero(plaq.view(np.uint64) != ref_plaq.view(np.uint64)))
    assert bits_equal(st, ref_st), int(np.count_nonzero(st.view(np.uint64) != ref_st.view(np.uint64)))
    assert bits_equal(F, ref_F), int(np.count_nonzero(F.view(np.uint64) != ref_F.view(np.uint64)))
    assert not bits_equal(F, F_start)
    for got, ref in ((sp.value, ref_sp.value), (act.value, ref_act.value)):
        assert abs(got - ref) <= 1e-13 * max(1.0, abs(ref)) + 1e-13 * S, (got, ref)
    assert (sp2.value, act2.value) == (sp.value, act.value)


@pytest.mark.parametrize("sigma", FIELDS, ids=FIELD_IDS)
@pytest.mark.parametrize("Nx,Nt", [(5, 9), (7, 2), (9, 3), (6, 257), (37, 130)])
def test_gauge_kernels_small_shapes_bitwise(sm, oracle, Nx, Nt, sigma):
    check_gauge_kernels(sm, oracle, Nx, Nt, sigma)


@pytest.mark.parametrize("sigma", FIELDS, ids=FIELD_IDS)
def test_gauge_kernels_grid_stride_1030x1040_bitwise(sm, oracle, sigma):
    """More sites than staple_force_kernel's 4096 x 256 threads: a second trip, ragged."""
    assert 1030 * 1040 > 4096 * 256 and 1030 * 1040 % (4096 * 256) % 256 != 0
    check_gauge_kernels(sm, oracle, 1030, 1040, sigma)


@pytest.mark.parametrize("sigma", FIELDS, ids=FIELD_IDS)
@pytest.mark.parametrize("Nx,Nt", [(8, 2), (24, 3), (6, 257), (37, 130)])
def test_gauge_kernels_loopback_ghost_links_bitwise(sm, oracle, Nx, Nt, sigma):
    """t-neighbours from the 2-deep ghost links of an RCCL loopback context."""
    check_gauge_kernels(sm, oracle, Nx, Nt, sigma, loopback=True)
