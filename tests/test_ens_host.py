"""The replica ensemble's entry points exist, state their cap and refuse bad
arguments before touching a device; the Python layer checks its arguments
before any library call (no GPU needed)."""
import ctypes
import re

import numpy as np
import pytest

import schwingermodel_amd as sm
from schwingermodel_amd import _lib

lib = sm.lib
NEW = ("sm_ens_max", "sm_ens_create", "sm_ens_destroy", "sm_ens_size", "sm_ens_upload_gauge",
       "sm_ens_download_gauge", "sm_ens_fill_gauge", "sm_ens_plaquette", "sm_ens_hmc_trajectory", "sm_ens_hmc_run")
SM_ERR_ARG = 1


def test_symbols_exist_and_are_declared():
    src = open(_lib.__file__).read()
    header = open(_lib.HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert f'"{name}"' in src, name                 # _lib.py gives it a signature
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(rf"\bint {name}\(", header), name
    assert "typedef struct sm_ens sm_ens;" in header
    assert lib.sm_abi_version() == 1


def test_cap():
    assert lib.sm_ens_max() >= 64
    assert lib.sm_ens_max() == lib.sm_cg_batch_max()


def test_null_context_or_ensemble_is_an_argument_error():
    h = ctypes.c_void_p()
    assert lib.sm_ens_create(None, 2, ctypes.byref(h)) == SM_ERR_ARG
    assert not h.value
    buf = np.zeros(8)
    p = buf.ctypes.data
    n = ctypes.c_int()
    prm = (sm.HMCParams * 1)(sm.HMCParams(0.0, 2.0, 0.3, 6, 1e-10, 100, 1, 0))
    res = (sm.HMCResult * 1)()
    summ = (sm.HMCSummary * 1)()
    assert lib.sm_ens_destroy(None) == SM_ERR_ARG
    assert lib.sm_ens_size(None, ctypes.byref(n)) == SM_ERR_ARG
    assert lib.sm_ens_upload_gauge(None, 0, p, p) == SM_ERR_ARG
    assert lib.sm_ens_download_gauge(None, 0, p, p) == SM_ERR_ARG
    assert lib.sm_ens_fill_gauge(None, 0, 1, -1.0) == SM_ERR_ARG
    assert lib.sm_ens_plaquette(None, p, p, p) == SM_ERR_ARG
    assert lib.sm_ens_hmc_trajectory(None, prm, 0, res) == SM_ERR_ARG
    assert lib.sm_ens_hmc_run(None, prm, 1, 0, 0, 1, 0, None, summ, None, None) == SM_ERR_ARG
    assert b"null" in lib.sm_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


V = 24


@pytest.fixture()
def ens(monkeypatch):
    """An Ensemble of 3 without a library object behind it; any library call
    through the package fails the test."""
    E = object.__new__(sm.Ensemble)
    E.lattice, E.R, E.V, E.ens = None, 3, V, None
    monkeypatch.setattr(sm, "lib", _NoLibrary())
    return E


def prm(md_steps=6, tol=1e-10, max_iter=1000, even_odd=0, m0=0.1):
    return sm.HMCParams(m0, 2.0, 0.3, md_steps, tol, max_iter, 7, even_odd)


@pytest.mark.parametrize("U,exc", [
    (np.zeros((2, V), dtype=np.float64), TypeError),
    (np.zeros((2, V), dtype=np.complex64), TypeError),
    ([[0j] * V] * 2, TypeError),
    (np.zeros((2 * V,), dtype=np.complex128), ValueError),
    (np.zeros((2, V - 1), dtype=np.complex128), ValueError),
    (np.zeros((1, V), dtype=np.complex128), ValueError),
], ids=["float64", "complex64", "list", "flat", "short", "one-plane"])
def test_upload_rejects_before_any_library_call(ens, U, exc):
    with pytest.raises(exc):
        ens.upload_gauge(0, U)


@pytest.mark.parametrize("r", [-1, 3, 1.0, "0"])
def test_replica_index_is_checked(ens, r):
    good = np.zeros((2, V), dtype=np.complex128)
    with pytest.raises(ValueError):
        ens.upload_gauge(r, good)
    with pytest.raises(ValueError):
        ens.download_gauge(r)
    with pytest.raises(ValueError):
        ens.fill_gauge(r, 1, -1.0)


@pytest.mark.parametrize("params,exc", [
    ([prm(), prm()], ValueError),                                   # 2 sets for 3 replicas
    ([prm(), prm(), prm(), prm()], ValueError),
    ([prm(), prm(md_steps=7), prm()], ValueError),
    ([prm(), prm(), prm(tol=1e-9)], ValueError),
    ([prm(), prm(max_iter=999), prm()], ValueError),
    ([prm(), prm(), prm(even_odd=1)], ValueError),
    ([prm(), (0.1, 2.0), prm()], TypeError),
], ids=["short", "long", "md_steps", "cg_tol", "cg_max_iter", "even_odd", "not-params"])
def test_params_are_checked_before_any_library_call(ens, params, exc):
    with pytest.raises(exc):
        ens.trajectory(params, 0)
    with pytest.raises(exc):
        ens.run(params, 0, 1, 0)


def test_differing_physics_parameters_pass_the_check(ens):
    """m0, beta, tau and seed are per replica: the check lets them through (and
    the call then reaches the library, which this fixture turns into an error)."""
    params = [sm.HMCParams(0.0, 2.0, 0.3, 6, 1e-10, 1000, 1, 0), sm.HMCParams(0.1, 3.0, 0.4, 6, 1e-10, 1000, 2, 0),
              sm.HMCParams(0.2, 2.0, 0.5, 6, 1e-10, 1000, 3, 0)]
    with pytest.raises(AssertionError, match="library call sm_ens_hmc_trajectory"):
        ens.trajectory(params, 0)


def test_plaquette_and_run_arguments(ens):
    with pytest.raises(ValueError):
        ens.plaquette([2.0, 3.0])
    with pytest.raises(ValueError):
        ens.run([prm(), prm(), prm()], 0, 0, 0)
    with pytest.raises(ValueError):
        sm.Ensemble(None, 0)
    with pytest.raises(ValueError):
        sm.Ensemble(None, 2.5)
