"""schwingermodel_amd -- MI355X-native hot path of Fabian2598/SchwingerModel.

The Wilson-Dirac apply D, D^dagger, D D^dagger, the fermion-force bilinear
and the CG solve of (D D^dagger)^{-1} run as hand-written HIP kernels for
gfx950 inside libsm_hip.so (C-ABI: include/sm_hip.h). This package is the
thin host-side mirror of the reference's function interface, so that code
written against src/dirac_operator.cpp / src/conjugate_gradient.cpp reads the
same:

    reference (C++)                                   here (Python)
    D_phi(U, phi, Dphi, m0)          :24             D_phi(U, phi, Dphi, m0)
    D_dagger_phi(U, phi, Dphi, m0)   :247            D_dagger_phi(U, phi, Dphi, m0)
    D_D_dagger_phi(U, phi, Dphi, m0) :477            D_D_dagger_phi(U, phi, Dphi, m0)
    phi_dag_partialD_phi(U, l, r)    :486            phi_dag_partialD_phi(U, l, r)
    conjugate_gradient(U, phi, x, m0)  cg.cpp:4      conjugate_gradient(U, phi, x, m0)
    dot(x, y)              include/variables.h:181   dot(x, y)
    CG::tol, CG::max_iter  src/variables.cpp:35-38   CG.tol, CG.max_iter
    spinor / re_field      include/variables.h:54    spinor / re_field

The lattice geometry (the reference's compile-time NS/NT plus mpi::) is set
once with init(Nx, Nt, nshard, shard, device, unique_id). There is no CPU
fallback: without the HIP library or a GPU every call raises.
"""
import collections
import ctypes
import math

import numpy as np

from ._lib import (CGMixedInfo, CGResult, FlowParams, HamiltonianTerms, HMCParams, HMCResult, HMCSummary, SMError,
                   Topo, check, lib)

__all__ = ["spinor", "re_field", "c_double", "I_number", "CG", "init", "lattice", "Lattice", "Ensemble",
           "D_phi", "D_dagger_phi", "D_D_dagger_phi", "phi_dag_partialD_phi",
           "conjugate_gradient", "dot", "SMError", "CGResult", "lib", "check", "Topology", "FlowSeries"]

c_double = complex
I_number = complex(0.0, 1.0)


class CG:
    """Mirror of namespace CG (src/variables.cpp:35-38; set in src/main.cpp:26-27)."""
    max_iter = 10000
    tol = 1e-10
    precision = "double"  # or "mixed" (Lattice.cg_precision; not in the reference)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


# What topology() / wilson_flow() return: float arrays, 0-d for a lattice's
# topology, (R,) for an ensemble's; a flow's have one more axis, the measured
# points, and t is the flow time of each (include/sm_hip.h "topological charge
# and Wilson flow").
Topology = collections.namedtuple("Topology", "action q_geo q_sin")
FlowSeries = collections.namedtuple("FlowSeries", "t action q_geo q_sin")


def _flow_params(eps, nsteps, meas_every):
    """(FlowParams, points) of a Wilson flow, checked as sm_wilson_flow checks them."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise TypeError(f"wilson_flow: eps = {eps!r}, expected a number")
    if not math.isfinite(eps) or not eps > 0:
        raise ValueError(f"wilson_flow: eps = {eps!r}, expected a finite step > 0")
    for name, v, lo in (("nsteps", nsteps, 0), ("meas_every", meas_every, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"wilson_flow: {name} = {v!r}, expected an integer")
        if v < lo or v > 2**31 - 2:
            raise ValueError(f"wilson_flow: {name} = {v!r}, expected an integer >= {lo}")
    return FlowParams(float(eps), int(nsteps), int(meas_every)), 1 + int(nsteps) // int(meas_every)


def _topo_arrays(buf, shape):
    """The (action, q_geo, q_sin) arrays of a ctypes array of sm_topo laid out as `shape`."""
    a = np.ctypeslib.as_array(buf).view(np.float64).reshape(shape + (3,))
    return tuple(np.array(a[..., i]) for i in range(3))


def _loops_args(who, solver, nnoise, seeds, R):
    """(solver mode, nnoise, seeds as a uint64 array of R) of a quark_loops call,
    checked as sm_quark_loops / sm_ens_quark_loops check them."""
    mode = Lattice.PION_SOLVERS.get(solver, solver) if isinstance(solver, str) else solver
    if not isinstance(mode, int) or isinstance(mode, bool) or mode not in (0, 1):
        raise ValueError(f"{who}: solver {solver!r}: 'plain' or 'even_odd'")
    if isinstance(nnoise, bool) or not isinstance(nnoise, (int, np.integer)):
        raise TypeError(f"{who}: nnoise = {nnoise!r}, expected an integer")
    if nnoise < 1 or nnoise > 2**31 - 1:
        raise ValueError(f"{who}: nnoise = {nnoise!r}, expected an integer >= 1")
    seeds = list(seeds)
    if len(seeds) != R:
        raise ValueError(f"{who}: {len(seeds)} seeds for {R} replicas")
    for s in seeds:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
            raise TypeError(f"{who}: seed = {s!r}, expected an integer")
        if not 0 <= s < 2**64:
            raise ValueError(f"{who}: seed = {s!r} outside 0..2^64 - 1")
    return mode, int(nnoise), np.array([int(s) for s in seeds], dtype=np.uint64)


class spinor:
    """Reference spinor (include/variables.h:54): two complex<double> arrays."""

    def __init__(self, N=None):
        if N is None:
            N = lattice().V
        self.size = int(N)
        self.mu0 = np.zeros(self.size, dtype=np.complex128)
        self.mu1 = np.zeros(self.size, dtype=np.complex128)

    @classmethod
    def from_arrays(cls, mu0, mu1):
        s = cls.__new__(cls)
        s.mu0 = np.ascontiguousarray(mu0, dtype=np.complex128)
        s.mu1 = np.ascontiguousarray(mu1, dtype=np.complex128)
        s.size = s.mu0.size
        return s

    def copy(self):
        return spinor.from_arrays(self.mu0.copy(), self.mu1.copy())


class re_field:
    """Reference re_field (include/variables.h:102): two double arrays."""

    def __init__(self, N=None):
        if N is None:
            N = lattice().V
        self.size = int(N)
        self.mu0 = np.zeros(self.size, dtype=np.float64)
        self.mu1 = np.zeros(self.size, dtype=np.float64)


class Lattice:
    """One t-shard of an Nx x Nt lattice on one GPU (owns an sm_ctx)."""

    def __init__(self, Nx, Nt, nshard=1, shard=0, device=0, unique_id=None, loopback=False):
        self.Nx, self.Nt, self.nshard, self.shard, self.device = Nx, Nt, nshard, shard, device
        t0, Wt = ctypes.c_int(), ctypes.c_int()
        check(lib.sm_shard_plan(Nt, nshard, shard, ctypes.byref(t0), ctypes.byref(Wt)))
        self.t0, self.Wt = t0.value, Wt.value
        self.V = Nx * self.Wt
        h = ctypes.c_void_p()
        uid = None
        if unique_id is not None:
            uid = ctypes.create_string_buffer(bytes(unique_id), len(unique_id))
        if loopback == "peer":  # one shard through the t-shard path over the peer transport, to itself
            if nshard != 1:
                raise ValueError("loopback is one shard")
            check(lib.sm_create_peer_loopback(ctypes.byref(h), Nx, Nt, device))
        elif loopback:  # one shard through the t-shard path over a one-rank RCCL communicator
            if nshard != 1:
                raise ValueError("loopback is one shard")
            if uid is None:
                uid = ctypes.create_string_buffer(128)
                check(lib.sm_comm_unique_id(uid, 128))
            check(lib.sm_create_loopback(ctypes.byref(h), Nx, Nt, device, uid))
        else:
            check(lib.sm_create(ctypes.byref(h), Nx, Nt, nshard, shard, device, uid))
        self.ctx = h
        self.last_cg = CGResult()

    TRANSPORTS = {0: "none", 1: "hosted", 2: "rccl", 3: "peer"}

    def comm_info(self):
        """(transport, nranks, rank) as the context's transport reports them
        (sm_comm_info: ncclCommCount / ncclCommUserRank for RCCL)."""
        t, n, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib.sm_comm_info(self.ctx, ctypes.byref(t), ctypes.byref(n), ctypes.byref(r)))
        return self.TRANSPORTS[t.value], n.value, r.value

    PRECISIONS = {"double": 0, "mixed": 1}

    def cg_precision(self, mode=None):
        """Set ("double" / "mixed", or 0 / 1) and return the precision of the
        solves that go through sm_cg_dev (sm_cg_precision; None only reads).
        Mixed runs on one-shard contexts: fp32 iterations held to the fp64
        stop test by reliable updates, so x passes the same test but is not
        the reference's iterate sequence."""
        m = -1 if mode is None else self.PRECISIONS.get(mode, mode)
        if not isinstance(m, int):
            raise ValueError(f"CG precision {mode!r}: 'double' or 'mixed'")
        cur = ctypes.c_int()
        check(lib.sm_cg_precision(self.ctx, m, ctypes.byref(cur)))
        return "mixed" if cur.value == 1 else "double"

    @property
    def last_cg_mixed(self):
        """sm_cg_mixed_info of the context's last sm_cg_dev (used = 0: it ran fp64)."""
        info = CGMixedInfo()
        check(lib.sm_cg_mixed_last(self.ctx, ctypes.byref(info)))
        return info

    def eo_cg_precision(self, mode=None):
        """Set ("double" / "mixed", or 0 / 1) and return the precision of the
        even-odd solver: sm_eo_cg and the even-odd action's solves
        (sm_eo_cg_precision; None only reads). Independent of cg_precision;
        one-shard contexts only."""
        m = -1 if mode is None else self.PRECISIONS.get(mode, mode)
        if not isinstance(m, int):
            raise ValueError(f"even-odd CG precision {mode!r}: 'double' or 'mixed'")
        cur = ctypes.c_int()
        check(lib.sm_eo_cg_precision(self.ctx, m, ctypes.byref(cur)))
        return "mixed" if cur.value == 1 else "double"

    @property
    def last_eo_cg_mixed(self):
        """sm_cg_mixed_info of the context's last even-odd solve (used = 0: it ran fp64)."""
        info = CGMixedInfo()
        check(lib.sm_eo_cg_mixed_last(self.ctx, ctypes.byref(info)))
        return info

    def cg_batch_precision(self, mode=None):
        """Set ("double" / "mixed", or 0 / 1) and return the precision of
        cg_batch and of the solve inside pion_correlator
        (sm_cg_batch_precision; None only reads). Independent of cg_precision
        and eo_cg_precision; one-shard contexts only. Mixed: every column
        passes the fp64 stop test but is not the reference's iterate sequence."""
        m = -1 if mode is None else self.PRECISIONS.get(mode, mode)
        if not isinstance(m, int):
            raise ValueError(f"batched CG precision {mode!r}: 'double' or 'mixed'")
        cur = ctypes.c_int()
        check(lib.sm_cg_batch_precision(self.ctx, m, ctypes.byref(cur)))
        return "mixed" if cur.value == 1 else "double"

    @property
    def last_cg_batch_mixed(self):
        """[sm_cg_mixed_info] of the K columns of the last cg_batch or
        pion_correlator of this object (used = 0: it ran fp64; [] before the
        first). sm_cg_batch_mixed_last serves callers of the C entry points."""
        K = getattr(self, "_batch_K", 0)
        if K < 1:
            return []
        info = (CGMixedInfo * K)()
        check(lib.sm_cg_batch_mixed_last(self.ctx, K, info))
        return list(info)

    def cg_batch(self, phi, m0, tol=None, max_iter=None):
        """Solve D D^dagger x_b = phi_b for K right-hand sides on the context's
        current gauge field in one batched solve (sm_cg_batch; no implicit
        upload). phi: complex128 of shape (K, 2, V), column b = (plane mu0,
        plane mu1). Returns (x, [CGResult] * K), each column with its own stop
        test and iteration count; fp64 unless cg_batch_precision("mixed")."""
        if not isinstance(phi, np.ndarray) or phi.dtype != np.complex128:
            raise TypeError("cg_batch: phi must be a complex128 numpy array")
        if phi.ndim != 3 or phi.shape[1:] != (2, self.V) or phi.shape[0] < 1:
            raise ValueError(f"cg_batch: phi has shape {phi.shape}, expected (K, 2, {self.V})")
        K = phi.shape[0]
        phi = np.ascontiguousarray(phi)
        x = np.empty_like(phi)
        res = (CGResult * K)()
        check(lib.sm_cg_batch(self.ctx, K, _vp(phi), _vp(x), float(m0), float(CG.tol if tol is None else tol),
                              int(CG.max_iter if max_iter is None else max_iter), res))
        self._batch_K = K
        return x, list(res)

    def eo_cg_batch(self, phi, m0, tol=None, max_iter=None):
        """Solve Dhat Dhat^dagger x_b = phi_b,e on the even sites for K
        right-hand sides on the context's current gauge field in one batched
        solve (sm_eo_cg_batch; no implicit upload). phi: complex128 of shape
        (K, 2, V) in the full layout, its even part is the source. Returns
        (x, [CGResult] * K); x is zero on the odd sites. Always fp64."""
        if not isinstance(phi, np.ndarray) or phi.dtype != np.complex128:
            raise TypeError("eo_cg_batch: phi must be a complex128 numpy array")
        if phi.ndim != 3 or phi.shape[1:] != (2, self.V) or phi.shape[0] < 1:
            raise ValueError(f"eo_cg_batch: phi has shape {phi.shape}, expected (K, 2, {self.V})")
        K = phi.shape[0]
        phi = np.ascontiguousarray(phi)
        x = np.empty_like(phi)
        res = (CGResult * K)()
        check(lib.sm_eo_cg_batch(self.ctx, K, _vp(phi), _vp(x), float(m0), float(CG.tol if tol is None else tol),
                                 int(CG.max_iter if max_iter is None else max_iter), res))
        return x, list(res)

    def pion_correlator(self, m0, sources, tol=None, max_iter=None):
        """Pion correlator from point sources on the context's current gauge
        field (sm_pion_correlator; no implicit upload). sources: a list of
        (x, t). Returns (C, results): C[s, t] = sum_x tr S S^dag at absolute
        time t for source s, results = the 2 * len(sources) solves (column
        2 s + spin)."""
        src = [(int(x), int(t)) for x, t in sources]
        n = len(src)
        sx = (ctypes.c_int * max(n, 1))(*[s[0] for s in src])
        st = (ctypes.c_int * max(n, 1))(*[s[1] for s in src])
        C = np.zeros((max(n, 1), self.Wt))
        res = (CGResult * max(2 * n, 1))()
        check(lib.sm_pion_correlator(self.ctx, float(m0), float(CG.tol if tol is None else tol),
                                     int(CG.max_iter if max_iter is None else max_iter), n, sx, st, _vp(C), res))
        self._batch_K = 2 * n
        return C, list(res)

    PION_SOLVERS = {"plain": 0, "even_odd": 1}

    def pion_solver(self, mode=None):
        """Set ("plain" / "even_odd", or 0 / 1) and return the solve inside
        pion_correlator (sm_pion_solver; None only reads): D D^dag, or the
        even-odd system with about half the iterations (always fp64, even Nx
        and Nt). One-shard contexts only."""
        m = -1 if mode is None else self.PION_SOLVERS.get(mode, mode)
        if not isinstance(m, int):
            raise ValueError(f"pion solver {mode!r}: 'plain' or 'even_odd'")
        cur = ctypes.c_int()
        check(lib.sm_pion_solver(self.ctx, m, ctypes.byref(cur)))
        return "even_odd" if cur.value == 1 else "plain"

    def quark_loops(self, m0, nnoise, seed, solver="plain", tol=None, max_iter=None):
        """Stochastic quark loops on the context's current gauge field
        (sm_quark_loops; no implicit upload): nnoise Z2 x Z2 noise vectors of
        `seed`, vector k bitwise sm_fill_noise(seed, k, ...). Returns (loops,
        results): loops complex of shape (nnoise, Nt, 2), [k, t, 0] = S_k(t) =
        sum_x eta^dag D^-1 eta and [k, t, 1] = P_k(t) = sum_x eta^dag gamma5
        D^-1 eta at absolute time t; results[k] the solve of vector k. solver:
        "plain" (D D^dag, following cg_batch_precision) or "even_odd" (always
        fp64, even Nx and Nt). The estimators are in schwingermodel_amd.loops."""
        mode, n, sd = _loops_args("quark_loops", solver, nnoise, [seed], 1)
        out = np.zeros((n, self.Wt, 4))
        res = (CGResult * n)()
        check(lib.sm_quark_loops(self.ctx, float(m0), float(CG.tol if tol is None else tol),
                                 int(CG.max_iter if max_iter is None else max_iter), mode, n,
                                 ctypes.c_uint64(int(sd[0])), _vp(out), res))
        self._batch_K = (n - 1) % lib.sm_cg_batch_max() + 1  # the last chunk's columns
        return out.view(np.complex128), list(res)

    def topology(self):
        """Topology(action, q_geo, q_sin) of the context's current gauge field
        (sm_topology; 0-d float arrays): sum (1 - Re U_01), the geometric charge
        (1/2 pi) sum arg U_01 and the field-theoretic one (1/2 pi) sum Im U_01.
        Works on every context plaquette sums work on; global values."""
        out = (Topo * 1)()
        check(lib.sm_topology(self.ctx, out))
        return Topology(*_topo_arrays(out, ()))

    def wilson_flow(self, eps, nsteps, meas_every=1, return_field=False):
        """Wilson flow of the current gauge field by nsteps third-order steps of
        size eps (sm_wilson_flow; the context's field is not changed). Returns
        FlowSeries(t, action, q_geo, q_sin), arrays of 1 + nsteps // meas_every
        points: the unflowed field, then every meas_every steps. With
        return_field also the flowed field, complex128 of shape (2, V).
        One-shard contexts."""
        p, points = _flow_params(eps, nsteps, meas_every)
        series = (Topo * points)()
        U = np.empty((2, self.V), dtype=np.complex128) if return_field else None
        check(lib.sm_wilson_flow(self.ctx, ctypes.byref(p), series, None if U is None else _vp(U[0]),
                                 None if U is None else _vp(U[1])))
        t = np.arange(points, dtype=np.float64) * (p.meas_every * p.eps)
        s = FlowSeries(t, *_topo_arrays(series, (points,)))
        return (s, U) if return_field else s

    def ensemble(self, R):
        """An Ensemble of R independent HMC chains on this lattice, evolved in
        lockstep with one launch per step for all of them (sm_ens_create)."""
        return Ensemble(self, R)

    def close(self):
        if self.ctx:
            lib.sm_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_field(self, s, name):
        if s.mu0.size < self.V or s.mu1.size < self.V:
            raise ValueError(f"{name}: size {s.mu0.size} < local volume {self.V}")
        for a in (s.mu0, s.mu1):
            if not a.flags.c_contiguous:
                raise ValueError(f"{name}: arrays must be C-contiguous")

    def upload_gauge(self, U):
        self._check_field(U, "U")
        check(lib.sm_upload_gauge(self.ctx, _vp(U.mu0), _vp(U.mu1)))


class Ensemble:
    """R replicas of a Lattice's gauge field, each with its own m0, beta, tau
    and seed, evolved by HMC in lockstep (owns an sm_ens; include/sm_hip.h
    "replica ensemble"). Close it before its Lattice. Gauge fields are
    complex128 arrays of shape (2, V): plane U_t, then plane U_x."""

    def __init__(self, lattice, R):
        if not isinstance(R, int) or isinstance(R, bool) or R < 1:
            raise ValueError(f"ensemble: R = {R!r}, expected an integer >= 1")
        self.lattice, self.R, self.V = lattice, R, lattice.V
        h = ctypes.c_void_p()
        check(lib.sm_ens_create(lattice.ctx, R, ctypes.byref(h)))
        self.ens = h

    def close(self):
        if self.ens:
            lib.sm_ens_destroy(self.ens)
            self.ens = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _replica(self, r):
        if not isinstance(r, (int, np.integer)) or not 0 <= r < self.R:
            raise ValueError(f"ensemble: replica {r!r} outside 0..{self.R - 1}")
        return int(r)

    def _params(self, params):
        """The R parameter sets as a ctypes array, checked for lockstep."""
        params = list(params)
        if len(params) != self.R:
            raise ValueError(f"ensemble: {len(params)} parameter sets for {self.R} replicas")
        for p in params:
            if not isinstance(p, HMCParams):
                raise TypeError("ensemble: params must be HMCParams")
            for name in ("md_steps", "cg_tol", "cg_max_iter"):
                if getattr(p, name) != getattr(params[0], name):
                    raise ValueError(f"ensemble: {name} must be the same for every replica")
            if p.even_odd not in (0, 1) or p.even_odd != params[0].even_odd:
                raise ValueError("ensemble: even_odd must be 0 or 1 and the same for every replica")
        return (HMCParams * self.R)(*params)

    def upload_gauge(self, r, U):
        r = self._replica(r)
        if not isinstance(U, np.ndarray) or U.dtype != np.complex128:
            raise TypeError("ensemble: U must be a complex128 numpy array")
        if U.shape != (2, self.V):
            raise ValueError(f"ensemble: U has shape {U.shape}, expected (2, {self.V})")
        U = np.ascontiguousarray(U)
        check(lib.sm_ens_upload_gauge(self.ens, r, _vp(U[0]), _vp(U[1])))

    def download_gauge(self, r):
        r = self._replica(r)
        U = np.empty((2, self.V), dtype=np.complex128)
        check(lib.sm_ens_download_gauge(self.ens, r, _vp(U[0]), _vp(U[1])))
        return U

    def fill_gauge(self, r, seed, sigma):
        """Replica r's field drawn on the device as sm_fill_gauge_dev draws it
        (sigma < 0: uniform angles, the hot start)."""
        r = self._replica(r)
        check(lib.sm_ens_fill_gauge(self.ens, r, int(seed), float(sigma)))

    def plaquette(self, betas):
        """(sp, gauge_action): arrays of R, sum Re U_01 and beta_r sum Re(1 - U_01)."""
        b = np.ascontiguousarray(betas, dtype=np.float64)
        if b.shape != (self.R,):
            raise ValueError(f"ensemble: {b.size} betas for {self.R} replicas")
        sp, act = np.empty(self.R), np.empty(self.R)
        check(lib.sm_ens_plaquette(self.ens, _vp(b), _vp(sp), _vp(act)))
        return sp, act

    def pion_correlator(self, m0s, sources, solver="plain", tol=None, max_iter=None):
        """The pion correlator of every replica on its current field with its
        own mass m0s[r], from point sources common to all replicas
        (sm_ens_pion_correlator). sources: a list of (x, t); solver: "plain"
        (D D^dag; bitwise Lattice.pion_correlator on a lone context with that
        field) or "even_odd". Returns (C, results): C of shape (R, nsrc, Nt),
        results[r][2 * s + a] the solve of replica r, source s, spin a."""
        m = np.ascontiguousarray(m0s, dtype=np.float64)
        if m.shape != (self.R,):
            raise ValueError(f"ensemble: {m.size} masses for {self.R} replicas")
        mode = Lattice.PION_SOLVERS.get(solver, solver)
        if not isinstance(mode, int) or isinstance(mode, bool) or mode not in (0, 1):
            raise ValueError(f"ensemble: pion solver {solver!r}: 'plain' or 'even_odd'")
        src = [(int(x), int(t)) for x, t in sources]
        n = len(src)
        sx = (ctypes.c_int * max(n, 1))(*[s[0] for s in src])
        st = (ctypes.c_int * max(n, 1))(*[s[1] for s in src])
        Nt = self.lattice.Wt
        C = np.zeros((self.R, max(n, 1), Nt))
        res = (CGResult * (self.R * max(2 * n, 1)))()
        check(lib.sm_ens_pion_correlator(self.ens, _vp(m), float(CG.tol if tol is None else tol),
                                         int(CG.max_iter if max_iter is None else max_iter), mode, n, sx, st, _vp(C),
                                         res))
        return C, [list(res[r * 2 * n:(r + 1) * 2 * n]) for r in range(self.R)]

    def quark_loops(self, m0s, nnoise, seeds, solver="plain", tol=None, max_iter=None):
        """Stochastic quark loops of every replica on its current field with its
        own mass m0s[r] and noise seed seeds[r] (sm_ens_quark_loops): for each
        vector one batched solve of R columns and one contraction launch for
        all replicas. Returns (loops, results): loops complex of shape (R,
        nnoise, Nt, 2) as Lattice.quark_loops, results[r][k] the solve of
        replica r's vector k. Replica r's row is bitwise Lattice.quark_loops on
        a lone context holding that field, with either solver. Always fp64."""
        m = np.ascontiguousarray(m0s, dtype=np.float64)
        if m.shape != (self.R,):
            raise ValueError(f"ensemble: {m.size} masses for {self.R} replicas")
        mode, n, sd = _loops_args("ensemble quark_loops", solver, nnoise, seeds, self.R)
        out = np.zeros((self.R, n, self.lattice.Wt, 4))
        res = (CGResult * (self.R * n))()
        check(lib.sm_ens_quark_loops(self.ens, _vp(m), float(CG.tol if tol is None else tol),
                                     int(CG.max_iter if max_iter is None else max_iter), mode, n, _vp(sd), _vp(out),
                                     res))
        return out.view(np.complex128), [list(res[r * n:(r + 1) * n]) for r in range(self.R)]

    def topology(self):
        """Topology(action, q_geo, q_sin) of every replica's current field, arrays
        of R (sm_ens_topology): one launch for all replicas, bitwise
        Lattice.topology on a lone context holding that field."""
        out = (Topo * self.R)()
        check(lib.sm_ens_topology(self.ens, out))
        return Topology(*_topo_arrays(out, (self.R,)))

    def wilson_flow(self, eps, nsteps, meas_every=1, return_field=False):
        """Wilson flow of every replica's field, one launch per stage for all of
        them (sm_ens_wilson_flow; the replicas' fields are not changed, and a
        trajectory after it is the trajectory without it). Returns
        FlowSeries(t, action, q_geo, q_sin), arrays of shape (R, points) with
        points = 1 + nsteps // meas_every; with return_field also the flowed
        fields, complex128 of shape (R, 2, V). Replica r's row is bitwise
        Lattice.wilson_flow on a lone context holding that field."""
        p, points = _flow_params(eps, nsteps, meas_every)
        series = (Topo * (self.R * points))()
        U = np.empty((self.R, 2, self.V), dtype=np.complex128) if return_field else None
        check(lib.sm_ens_wilson_flow(self.ens, ctypes.byref(p), series, None if U is None else _vp(U)))
        t = np.broadcast_to(np.arange(points, dtype=np.float64) * (p.meas_every * p.eps), (self.R, points)).copy()
        s = FlowSeries(t, *_topo_arrays(series, (self.R, points)))
        return (s, U) if return_field else s

    def trajectory(self, params, traj):
        """One HMC update of every replica (sm_ens_hmc_trajectory): params is a
        list of R HMCParams; returns R HMCResult."""
        p = self._params(params)
        out = (HMCResult * self.R)()
        check(lib.sm_ens_hmc_trajectory(self.ens, p, int(traj), out))
        return list(out)

    def run(self, params, Ntherm, Nmeas, Nsteps, hot_start=True, first_traj=0, save_prefix=None):
        """sm_ens_hmc_run: returns (R HMCSummary, sp, gs), the series of shape
        (R, Nmeas). save_prefix: <save_prefix>_r<r>_<i>.ctxt after measurement i."""
        p = self._params(params)
        if Ntherm < 0 or Nmeas < 1 or Nsteps < 0:
            raise ValueError(f"ensemble: Ntherm={Ntherm} Nmeas={Nmeas} Nsteps={Nsteps}")
        out = (HMCSummary * self.R)()
        sp, gs = np.empty((self.R, Nmeas)), np.empty((self.R, Nmeas))
        prefix = None if save_prefix is None else str(save_prefix).encode()
        check(lib.sm_ens_hmc_run(self.ens, p, 1 if hot_start else 0, int(first_traj), int(Ntherm), int(Nmeas),
                                 int(Nsteps), prefix, out, _vp(sp), _vp(gs)))
        return list(out), sp, gs


_LATTICE = None


def init(Nx, Nt, nshard=1, shard=0, device=0, unique_id=None, loopback=False):
    """Set the lattice geometry (the reference's NS/NT + mpi:: setup).
    loopback=True: one shard driven through the multi-GPU (RCCL) code path."""
    global _LATTICE
    if _LATTICE is not None:
        _LATTICE.close()
    _LATTICE = Lattice(Nx, Nt, nshard, shard, device, unique_id, loopback)
    return _LATTICE


def lattice():
    if _LATTICE is None:
        raise SMError("call schwingermodel_amd.init(Nx, Nt, ...) first")
    return _LATTICE


def _apply(U, phi, Dphi, m0, dagger):
    L = lattice()
    L._check_field(phi, "phi")
    L._check_field(Dphi, "Dphi")
    L.upload_gauge(U)  # the caller may have changed U since the last call (src/hmc.cpp:69-99)
    check(lib.sm_dirac(L.ctx, _vp(phi.mu0), _vp(phi.mu1), _vp(Dphi.mu0), _vp(Dphi.mu1),
                       float(m0), dagger))


def D_phi(U, phi, Dphi, m0):
    """Dphi = D phi, eq. (34); src/dirac_operator.cpp:24."""
    _apply(U, phi, Dphi, m0, 0)


def D_dagger_phi(U, phi, Dphi, m0):
    """Dphi = D^dagger phi, eqs. (35)-(36); src/dirac_operator.cpp:247."""
    _apply(U, phi, Dphi, m0, 1)


def D_D_dagger_phi(U, phi, Dphi, m0):
    """Dphi = D D^dagger phi; src/dirac_operator.cpp:477."""
    L = lattice()
    L._check_field(phi, "phi")
    L._check_field(Dphi, "Dphi")
    L.upload_gauge(U)
    check(lib.sm_ddag(L.ctx, _vp(phi.mu0), _vp(phi.mu1), _vp(Dphi.mu0), _vp(Dphi.mu1), float(m0)))


def phi_dag_partialD_phi(U, left, right):
    """Fermion-force bilinear, eqs. (37)-(38); src/dirac_operator.cpp:486. Returns a re_field."""
    L = lattice()
    L._check_field(left, "left")
    L._check_field(right, "right")
    L.upload_gauge(U)
    F = re_field(L.V)
    check(lib.sm_force(L.ctx, _vp(left.mu0), _vp(left.mu1), _vp(right.mu0), _vp(right.mu1),
                       _vp(F.mu0), _vp(F.mu1)))
    return F


def dot(x, y):
    """sum_n x conj(y) over all shards; include/variables.h:181."""
    L = lattice()
    out = np.zeros(2)
    check(lib.sm_dot(L.ctx, _vp(x.mu0), _vp(x.mu1), _vp(y.mu0), _vp(y.mu1), _vp(out)))
    return complex(out[0], out[1])


def conjugate_gradient(U, phi, x, m0):
    """Solve D D^dagger x = phi (x0 = phi); src/conjugate_gradient.cpp:4.

    Returns 1 if converged, 0 otherwise (and prints the reference's message on
    shard 0). Details of the last solve are in lattice().last_cg.
    """
    L = lattice()
    L._check_field(phi, "phi")
    if x.mu0.size != phi.mu0.size:  # spinor::operator= reallocates, include/variables.h:73-86
        x.mu0 = np.zeros_like(phi.mu0)
        x.mu1 = np.zeros_like(phi.mu1)
        x.size = phi.size
    L.upload_gauge(U)
    if L.cg_precision() != CG.precision:
        L.cg_precision(CG.precision)
    res = CGResult()
    check(lib.sm_cg(L.ctx, _vp(phi.mu0), _vp(phi.mu1), _vp(x.mu0), _vp(x.mu1), float(m0),
                    float(CG.tol), int(CG.max_iter), ctypes.byref(res)))
    L.last_cg = res
    if not res.converged and L.shard == 0:
        print(f"CG for DD^+ did not converge in {CG.max_iter} iterations Error {res.residual}")
    return 1 if res.converged else 0
