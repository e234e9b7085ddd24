"""Topological charge and Wilson flow without a GPU: the entry points exist and
refuse bad arguments before touching a device, the Python layer checks its
arguments before any library call, and the host model of tests/flow_model.py
(the checker of test_flow_gpu.py) has the properties the device is held to."""
import ctypes
import re

import numpy as np
import pytest

import flow_model as fm
import schwingermodel_amd as sm
from schwingermodel_amd import _lib

lib = sm.lib
FUNCS = ("sm_flow_points", "sm_topology", "sm_wilson_flow", "sm_ens_topology", "sm_ens_wilson_flow")
TYPES = ("sm_topo", "sm_flow_params")
SM_ERR_ARG = 1


def test_symbols_exist_and_are_declared():
    src = open(_lib.__file__).read()
    header = open(_lib.HEADER).read()
    for name in FUNCS:
        assert hasattr(lib, name), name
        assert f'"{name}"' in src, name                 # _lib.py gives it a signature
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(rf"\bint {name}\(", header), name
    for name in TYPES:
        assert re.search(rf"typedef struct {{[^}}]*}} {name};", header), name
    assert "typedef struct { double action, q_geo, q_sin; } sm_topo;" in header
    assert "typedef struct { double eps; int nsteps; int meas_every; } sm_flow_params;" in header
    assert ctypes.sizeof(_lib.Topo) == 24 and ctypes.sizeof(_lib.FlowParams) == 16
    assert lib.sm_abi_version() == 1


def points(eps, nsteps, meas_every):
    return lib.sm_flow_points(ctypes.byref(_lib.FlowParams(eps, nsteps, meas_every)))


def test_flow_points():
    assert points(0.1, 0, 1) == 1
    assert points(0.1, 10, 3) == 4
    assert points(0.1, 10, 10) == 2
    assert points(0.1, 9, 10) == 1
    for bad in ((0.0, 1, 1), (-0.1, 1, 1), (float("nan"), 1, 1), (float("inf"), 1, 1), (0.1, -1, 1), (0.1, 1, 0),
                (0.1, 1, -3)):
        assert points(*bad) < 0, bad
    assert lib.sm_flow_points(None) < 0


def test_null_arguments_are_argument_errors():
    t = (_lib.Topo * 4)()
    p = _lib.FlowParams(0.1, 2, 1)
    buf = np.zeros(8)
    assert lib.sm_topology(None, t) == SM_ERR_ARG
    assert b"null" in lib.sm_last_error()
    assert lib.sm_wilson_flow(None, ctypes.byref(p), t, None, None) == SM_ERR_ARG
    assert lib.sm_wilson_flow(None, None, None, buf.ctypes.data, None) == SM_ERR_ARG
    assert lib.sm_ens_topology(None, t) == SM_ERR_ARG
    assert lib.sm_ens_wilson_flow(None, ctypes.byref(p), t, None) == SM_ERR_ARG
    assert lib.sm_ens_wilson_flow(None, None, None, None) == SM_ERR_ARG
    assert b"null" in lib.sm_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


V = 24


@pytest.fixture()
def objs(monkeypatch):
    """A Lattice and an Ensemble of 3 without library objects behind them; any
    library call through the package fails the test."""
    L = object.__new__(sm.Lattice)
    L.ctx, L.V = None, V
    E = object.__new__(sm.Ensemble)
    E.lattice, E.R, E.V, E.ens = None, 3, V, None
    monkeypatch.setattr(sm, "lib", _NoLibrary())
    return L, E


@pytest.mark.parametrize("args,exc", [
    ((0.0, 10), ValueError), ((-0.1, 10), ValueError), ((float("nan"), 10), ValueError),
    ((float("inf"), 10), ValueError), (("0.1", 10), TypeError), ((True, 10), TypeError), ((None, 10), TypeError),
    ((0.1, -1), ValueError), ((0.1, 2.0), TypeError), ((0.1, "3"), TypeError), ((0.1, True), TypeError),
    ((0.1, 2**31), ValueError),
    ((0.1, 10, 0), ValueError), ((0.1, 10, -2), ValueError), ((0.1, 10, 1.0), TypeError), ((0.1, 10, None), TypeError),
], ids=["eps0", "eps<0", "nan", "inf", "eps-str", "eps-bool", "eps-none", "nsteps<0", "nsteps-float", "nsteps-str",
        "nsteps-bool", "nsteps-huge", "every0", "every<0", "every-float", "every-none"])
def test_wilson_flow_rejects_before_any_library_call(objs, args, exc):
    for o in objs:
        with pytest.raises(exc):
            o.wilson_flow(*args)
        with pytest.raises(exc):
            o.wilson_flow(*args, return_field=True)


def test_good_arguments_reach_the_library(objs):
    L, E = objs
    with pytest.raises(AssertionError, match="library call sm_wilson_flow"):
        L.wilson_flow(0.05, 10, 5)
    with pytest.raises(AssertionError, match="library call sm_ens_wilson_flow"):
        E.wilson_flow(np.float64(0.05), np.int64(0), return_field=True)
    with pytest.raises(AssertionError, match="library call sm_topology"):
        L.topology()
    with pytest.raises(AssertionError, match="library call sm_ens_topology"):
        E.topology()


def test_result_shapes():
    """The arrays the methods hand back, from the sm_topo records as the library lays them out."""
    buf = (_lib.Topo * 6)(*[_lib.Topo(i, 10 + i, 20 + i) for i in range(6)])
    a, g, s = sm._topo_arrays(buf, (2, 3))
    assert a.shape == g.shape == s.shape == (2, 3)
    assert a.tolist() == [[0, 1, 2], [3, 4, 5]] and g[1, 0] == 13 and s[0, 2] == 22   # replica-major
    one = sm._topo_arrays((_lib.Topo * 1)(_lib.Topo(1.5, 2.0, 2.5)), ())
    assert [x.shape for x in one] == [(), (), ()] and float(one[2]) == 2.5
    p, n = sm._flow_params(0.05, 10, 3)
    assert (p.eps, p.nsteps, p.meas_every, n) == (0.05, 10, 3, 4)


# ---- the model ------------------------------------------------------------------
def test_longdouble_is_wider():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize("case", fm.CASES, ids=fm.CASE_IDS)
def test_model_on_the_backgrounds(case):
    Nx, Nt, Q, seed, eps, nsteps, _ = case
    V_ = Nx * Nt
    clean = fm.topology(fm.background(Nx, Nt, Q, seed, sigma=0.0))
    assert round(float(clean[1])) == Q and abs(clean[1] - Q) < 1e-12
    U = fm.background(Nx, Nt, Q, seed)
    a, qg, qs, margin = fm.topology(U)
    assert round(float(qg)) == Q and abs(qg - Q) <= 1e-14 * V_
    # a gauge transformation changes no plaquette
    ag, qgg, qsg, _ = fm.topology(fm.gauge_transform(U, seed + 1))
    assert abs(ag - a) <= 1e-12 * V_ and abs(qgg - qg) <= 1e-12 * V_ and abs(qsg - qs) <= 1e-12 * V_
    assert fm.max_component_deviation(fm.gauge_transform(U, seed + 1), U) > 0.1
    deltas, fields = fm.delta_ref(U, eps, nsteps)
    tops = [fm.topology(f) for f in fields]
    for t in tops:
        assert round(float(t[1])) == Q
        assert t[3] >= 0.2          # every plaquette angle well away from +-pi at every step
    acts = [float(t[0]) for t in tops]
    assert all(b < a for a, b in zip(acts, acts[1:]))
    assert abs(tops[-1][2] - Q) < abs(tops[0][2] - Q)     # q_sin approaches q_geo
    print(f"flow model {Nx}x{Nt} Q {Q}: delta_ref {deltas[-1]:.3e}, margin {min(float(t[3]) for t in tops):.3f}")
    assert 0.0 < deltas[-1] < 1e-14


def test_large_case_background():
    Nx, Nt, Q, seed, eps, nsteps, _ = fm.LARGE
    U = fm.background(Nx, Nt, Q, seed, sigma=fm.LARGE_SIGMA)
    for f in fm.flow(U, eps, nsteps):
        _, qg, _, margin = fm.topology(f)
        assert round(float(qg)) == Q and margin >= 0.2
    assert Nx * Nt > 4096 * 256


def test_third_order():
    """Halving eps at fixed flow time shrinks the deviation from an eps / 8 run by 2^3,
    within 6x to 10x (9.0 at eps = 0.05, 8.6 at 0.025; the limit is 8.1 with this
    reference, whose own error is 1/512 of the coarse run's)."""
    U = fm.background(6, 10, 1, 103)
    t, eps = 0.4, 0.05
    ref = fm.flow(U, eps / 8, round(t / (eps / 8)))[-1]
    e1 = fm.max_component_deviation(fm.flow(U, eps, round(t / eps))[-1], ref)
    e2 = fm.max_component_deviation(fm.flow(U, eps / 2, round(t / (eps / 2)))[-1], ref)
    assert e2 > 1e-9          # far above rounding
    assert 6.0 <= e1 / e2 <= 10.0, (e1, e2)


@pytest.mark.parametrize("damage", [dict(c2=(17.0, 32.0)), dict(stage1=False), dict(zsign=+1.0),
                                    dict(wrong_neighbour=True), dict(rot0=0.5)],
                         ids=["17/32", "no-stage-1", "Z-sign", "wrong-neighbour", "rot-0.5"])
def test_each_damage_moves_a_link(damage):
    """What the device comparison can tell apart: every single change of the
    definition moves a flowed link by more than 1e-4, allowed being below 1e-12."""
    for case in (fm.CASES[3], fm.CASES[5]):
        Nx, Nt, Q, seed, eps, nsteps, _ = case
        U = fm.background(Nx, Nt, Q, seed)
        good = fm.flow(U, eps, nsteps)[-1]
        bad = fm.flow(U, eps, nsteps, **damage)[-1]
        assert fm.max_component_deviation(good, bad) > 1e-4, damage
