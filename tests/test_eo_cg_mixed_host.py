"""The mixed-precision even-odd CG's entry points exist, are in the ctypes
table and refuse a null context (no GPU needed)."""
import ctypes
import inspect

import pytest

sm = pytest.importorskip("schwingermodel_amd")
lib = sm.lib


def test_symbols_exist():
    assert hasattr(lib, "sm_eo_cg_precision") and hasattr(lib, "sm_eo_cg_mixed_last")


def test_null_context_is_an_argument_error():
    mode = ctypes.c_int(-7)
    assert lib.sm_eo_cg_precision(None, 1, ctypes.byref(mode)) == 1  # SM_ERR_ARG
    assert mode.value == -7
    assert lib.sm_eo_cg_precision(None, 1, None) == 1
    info = sm.CGMixedInfo()
    assert lib.sm_eo_cg_mixed_last(None, ctypes.byref(info)) == 1
    assert lib.sm_eo_cg_mixed_last(None, None) == 1


def test_prototypes_are_in_the_ctypes_table():
    from schwingermodel_amd import _lib
    src = inspect.getsource(_lib)
    assert '"sm_eo_cg_precision"' in src and '"sm_eo_cg_mixed_last"' in src
    assert lib.sm_eo_cg_precision.argtypes is not None and len(lib.sm_eo_cg_precision.argtypes) == 3
    assert lib.sm_eo_cg_mixed_last.argtypes is not None and len(lib.sm_eo_cg_mixed_last.argtypes) == 2


def test_python_interface_is_there():
    assert callable(getattr(sm.Lattice, "eo_cg_precision", None))
    assert isinstance(getattr(sm.Lattice, "last_eo_cg_mixed", None), property)
