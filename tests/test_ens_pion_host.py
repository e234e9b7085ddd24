"""The ensemble's pion correlator and the even-odd correlator without a GPU: the
entry points exist and refuse bad arguments before touching a device, the
Python layer checks its arguments before any library call, the index
arithmetic of csrc/sm_pion_host.h runs under the host sanitizers
(tools/pion_host_check.cpp), and the dense model the GPU tests are held to
(ens_pion_model.py) agrees with itself: the even-odd path reproduces the exact
correlator, and the derived bound rejects every damaged variant of it."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ens_pion_model as epm
import schwingermodel_amd as sm
from schwingermodel_amd import _lib

lib = sm.lib
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SM_ERR_ARG = 1
M0 = -0.10


def test_symbols_exist_and_are_declared():
    src = open(_lib.__file__).read()
    header = open(_lib.HEADER).read()
    for name in ("sm_ens_pion_correlator", "sm_pion_solver"):
        assert hasattr(lib, name), name
        assert f'"{name}"' in src, name
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(rf"\bint {name}\(", header), name
    assert lib.sm_abi_version() == 1


def test_null_handles_are_argument_errors():
    buf = np.zeros(8)
    p = buf.ctypes.data
    sx = (ctypes.c_int * 1)(0)
    mode = ctypes.c_int(7)
    assert lib.sm_ens_pion_correlator(None, p, 1e-10, 10, 0, 1, sx, sx, p, None) == SM_ERR_ARG
    assert b"null" in lib.sm_last_error()
    assert lib.sm_pion_solver(None, 1, ctypes.byref(mode)) == SM_ERR_ARG
    assert mode.value == 7
    assert lib.sm_pion_solver(None, -1, None) == SM_ERR_ARG


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


class _Lat:
    Wt = 10


@pytest.fixture()
def ens(monkeypatch):
    E = object.__new__(sm.Ensemble)
    E.lattice, E.R, E.V, E.ens = _Lat(), 3, 60, None
    monkeypatch.setattr(sm, "lib", _NoLibrary())
    return E


def test_python_checks_come_before_any_library_call(ens):
    with pytest.raises(ValueError):
        ens.pion_correlator([0.0, 0.1], [(0, 0)])                       # 2 masses for 3 replicas
    with pytest.raises(ValueError):
        ens.pion_correlator([0.0, 0.1, 0.2], [(0, 0)], solver="eo")     # no such solver
    with pytest.raises(ValueError):
        ens.pion_correlator([0.0, 0.1, 0.2], [(0, 0)], solver=2)
    with pytest.raises(AssertionError, match="library call sm_ens_pion_correlator"):
        ens.pion_correlator([0.0, 0.1, 0.2], [(0, 0)], solver="even_odd")
    L = object.__new__(sm.Lattice)
    L.ctx = None
    with pytest.raises(ValueError):
        L.pion_solver("fast")
    with pytest.raises(AssertionError, match="library call sm_pion_solver"):
        L.pion_solver("even_odd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pion_host_check(tmp_path):
    exe = str(tmp_path / "pion_host_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(REPO, "tools", "pion_host_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "pion_host_check ok"


@pytest.mark.parametrize("shape", epm.SHAPES_EVEN, ids=epm.shape_id)
def test_schur_path_is_the_exact_correlator_and_the_bound_rejects_damage(shape):
    """The even-odd algebra against numpy.linalg.solve on the dense D to 1e-12
    relative, both source parities; each damaged variant leaves 2 x the derived
    bound somewhere (they are off by O(0.1) of C, the bound is below 1e-6 of it)."""
    Nx, Nt = shape
    M = epm.model(sm, Nx, Nt, epm.SEEDS[0], M0)
    nsrc = len(M["src"])
    parities = {(x + t) & 1 for x, t in M["src"]}
    assert parities == {0, 1}
    S, _ = epm.schur_propagators(M["D"], Nx, Nt, M0, M["phi"])
    C = epm.slices(S, Nx, Nt, nsrc)
    rel = np.abs(C - M["C"]) / M["C"]
    B = epm.MARGIN * epm.bound(M, Nx, Nt, even_odd=True)
    print(f"ENS PION MODEL {Nx}x{Nt}: schur vs dense {rel.max():.3e}; sigma_min {M['sigma_min']:.4f}; "
          f"bound / C in [{(B / M['C']).min():.2e}, {(B / M['C']).max():.2e}]; C in [{M['C'].min():.3e}, "
          f"{M['C'].max():.3e}]")
    assert rel.max() <= 1e-12
    assert np.all(np.abs(C - M["C"]) <= B)
    damaged = {
        "(1/m) phi_o dropped": epm.slices(epm.schur_propagators(M["D"], Nx, Nt, M0, M["phi"], drop_phi_o_term=True)[0],
                                          Nx, Nt, nsrc),
        "(1/2m) H_eo phi_o dropped": epm.slices(
            epm.schur_propagators(M["D"], Nx, Nt, M0, M["phi"], drop_heo_term=True)[0], Nx, Nt, nsrc),
        "parity flipped": epm.slices(epm.schur_propagators(M["D"], Nx, Nt, M0, M["phi"], flip_parity=True)[0],
                                     Nx, Nt, nsrc),
        "spin 1 dropped": epm.slices(S, Nx, Nt, nsrc, spins=(0,)),
    }
    odd = [s for s, (x, t) in enumerate(M["src"]) if (x + t) & 1]
    for name, Cd in damaged.items():
        over = np.abs(Cd - M["C"]) > B
        worst = (np.abs(Cd - M["C"]) / M["C"]).max()
        print(f"  {name}: off by up to {worst:.2e} of C")
        assert over.any(), name
        if "phi_o" in name:  # these two touch the odd sources only, and must be caught there
            assert over[odd].any(), name
