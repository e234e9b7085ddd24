"""The batched even-odd CG's entry points exist and refuse a null context
before touching a device; the ensemble's Python layer knows the even-odd
lockstep rule (even_odd is 0 or 1 and common to the replicas) before any
library call (no GPU needed)."""
import re

import numpy as np
import pytest

import schwingermodel_amd as sm
from schwingermodel_amd import _lib
from test_ens_host import _NoLibrary, prm

lib = sm.lib
NEW = ("sm_eo_cg_batch_dev", "sm_eo_cg_batch")
SM_ERR_ARG = 1
V = 24


def test_symbols_exist_and_are_declared():
    src = open(_lib.__file__).read()
    header = open(_lib.HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert f'"{name}"' in src, name                 # _lib.py gives it a signature
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(rf"\bint {name}\(", header), name
    assert lib.sm_abi_version() == 1


def test_null_context_is_an_argument_error():
    buf = np.zeros(8)
    out = np.zeros(8)
    res = (sm.CGResult * 1)()
    for name in NEW:
        assert getattr(lib, name)(None, 1, buf.ctypes.data, out.ctypes.data, 0.1, 1e-10, 10, res) == SM_ERR_ARG
        assert b"null" in lib.sm_last_error()


@pytest.fixture()
def ens(monkeypatch):
    """test_ens_host.py's fixture: an Ensemble of 3 without a library object
    behind it; any library call through the package fails the test."""
    E = object.__new__(sm.Ensemble)
    E.lattice, E.R, E.V, E.ens = None, 3, V, None
    monkeypatch.setattr(sm, "lib", _NoLibrary())
    return E


def test_three_even_odd_sets_pass_the_check(ens):
    params = [prm(even_odd=1, m0=0.0), prm(even_odd=1, m0=0.1), prm(even_odd=1, m0=0.2)]
    p = ens._params(params)
    assert [q.even_odd for q in p] == [1, 1, 1]
    with pytest.raises(AssertionError, match="library call sm_ens_hmc_trajectory"):
        ens.trajectory(params, 0)


@pytest.mark.parametrize("values", [(0, 1, 0), (1, 1, 0), (1, 0, 1), (0, 0, 1)])
def test_mixed_even_odd_is_refused_before_any_library_call(ens, values):
    params = [prm(even_odd=v) for v in values]
    with pytest.raises(ValueError, match="even_odd"):
        ens.trajectory(params, 0)
    with pytest.raises(ValueError, match="even_odd"):
        ens.run(params, 0, 1, 0)


@pytest.mark.parametrize("values", [(2, 2, 2), (1, 2, 1), (-1, -1, -1)])
def test_even_odd_other_than_0_or_1_is_refused(ens, values):
    params = [prm(even_odd=v) for v in values]
    with pytest.raises(ValueError, match="even_odd"):
        ens.trajectory(params, 0)
