"""The batched CG's and the pion correlator's entry points exist, state their
cap and refuse bad arguments before touching a device (no GPU needed)."""
import re

import numpy as np
import pytest

import schwingermodel_amd as sm
from schwingermodel_amd import _lib

lib = sm.lib
NEW = ("sm_cg_batch_max", "sm_cg_batch_dev", "sm_cg_batch", "sm_pion_correlator")


def test_symbols_exist_and_are_declared():
    src = open(_lib.__file__).read()
    header = open(_lib.HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert f'"{name}"' in src, name                 # _lib.py gives it a signature
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(rf"\bint {name}\(", header), name
    assert lib.sm_abi_version() == 1


def test_cap():
    assert lib.sm_cg_batch_max() >= 64


def test_null_context_is_an_argument_error():
    res = (sm.CGResult * 2)()
    buf = np.zeros(8)
    p = buf.ctypes.data
    assert lib.sm_cg_batch(None, 1, p, p, 0.0, 1e-10, 10, res) == 1  # SM_ERR_ARG
    assert lib.sm_cg_batch_dev(None, 1, p, p, 0.0, 1e-10, 10, res) == 1
    assert lib.sm_pion_correlator(None, 0.0, 1e-10, 10, 1, None, None, p, res) == 1


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


@pytest.fixture()
def lattice(monkeypatch):
    """A Lattice without a context; any library call through the package fails the test."""
    L = object.__new__(sm.Lattice)
    L.Nx, L.Nt, L.Wt, L.V, L.ctx = 4, 6, 6, 24, None
    monkeypatch.setattr(sm, "lib", _NoLibrary())
    return L


@pytest.mark.parametrize("phi,exc", [
    (np.zeros((3, 2, 24), dtype=np.float64), TypeError),
    (np.zeros((3, 2, 24), dtype=np.complex64), TypeError),
    ([[0j] * 24] * 2, TypeError),
    (np.zeros((2, 24), dtype=np.complex128), ValueError),
    (np.zeros((3, 2, 23), dtype=np.complex128), ValueError),
    (np.zeros((3, 1, 24), dtype=np.complex128), ValueError),
    (np.zeros((0, 2, 24), dtype=np.complex128), ValueError),
], ids=["float64", "complex64", "list", "2d", "short", "one-plane", "empty"])
def test_cg_batch_rejects_before_any_library_call(lattice, phi, exc):
    with pytest.raises(exc):
        lattice.cg_batch(phi, -0.1)
