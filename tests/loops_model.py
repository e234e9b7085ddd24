"""Dense numpy model of the stochastic quark loops (test helper of
test_loops_host.py and test_loops_gpu.py), on ens_pion_model's dense Dirac
matrix D (index = plane * V + x * Nt + t):

    eta_k   = sm_fill_noise(seed, k), the library's host filler
    psi*_k  = D^-1 eta_k                                   (numpy.linalg.solve)
    S*_k(t) = sum_x sum_a conj(eta_a) psi*_a,  P*_k(t) = sum_x (conj(eta_0) psi*_0 - conj(eta_1) psi*_1)
    Tr_t D^-1, Tr_t gamma5 D^-1 = the diagonal of D^-1 summed over the slice,
                                  gamma5 = diag(+1 on plane 0, -1 on plane 1)

The bound, derived. Both solvers stop on ||r|| < tol ||b||, and the residual
carries over to the full system (ens_pion_model's argument: the odd rows are
solved exactly by the reconstruction). So ||d psi_k|| <= eps_k = tol beta_k /
sigma_min(D), beta_k = ||eta|| = sqrt(2 V) for solver 0 and ||phihat_e,k|| for
solver 1. A slice of eta has norm sqrt(2 Nx) (every component has modulus 1), so
by Cauchy-Schwarz |d S_k(t)|, |d P_k(t)| <= sqrt(2 Nx) eps_k. The tests allow
ens_pion_model.MARGIN = 2 x that, for the reason given there.

The noise seeds below were fixed after test_loops_host.py's statistical checks
passed with them on the CPU (ESTIMATOR_SEED keeps the 64-vector means within 3
standard errors of the exact traces, the tests allow 4).
"""
import functools

import numpy as np

import ens_pion_model as epm
from conftest import ptr

NNOISE = 3
NOISE_SEEDS = (1011, 2022, 3033)     # one per replica, next to epm.SEEDS / epm.MASSES
ESTIMATOR_SHAPE, ESTIMATOR_N, ESTIMATOR_SEED = (16, 16), 64, 20261
NF = 2


def noise(sm, Nx, Nt, seed, k):
    """Noise vector k of seed: complex (2 V,), plane 0 then plane 1."""
    S = Nx * Nt
    p = np.empty(4 * S)
    sm.lib.sm_fill_noise(seed, k, Nt, 0, Nx, 0, Nt, ptr(p[:2 * S]), ptr(p[2 * S:]))
    return p.view(np.complex128).copy()


def noise_matrix(sm, Nx, Nt, seed, nnoise):
    return np.stack([noise(sm, Nx, Nt, seed, k) for k in range(nnoise)], axis=1)


def slice_sums(eta, psi, Nx, Nt):
    """(S, P), each (K, Nt), of the columns of eta and psi (n, K)."""
    w = (np.conj(eta) * psi).reshape(2, Nx, Nt, -1)
    return (w[0] + w[1]).sum(axis=0).T, (w[0] - w[1]).sum(axis=0).T


def exact_traces(G, Nx, Nt):
    """(Tr_t D^-1, Tr_t gamma5 D^-1), each (Nt,), from G = D^-1."""
    d = np.diagonal(G).reshape(2, Nx, Nt)
    return (d[0] + d[1]).sum(axis=0), (d[0] - d[1]).sum(axis=0)


@functools.lru_cache(maxsize=None)
def _model(sm_key, Nx, Nt, gseed, m0, nseed, nnoise):
    sm = epm._SM[sm_key]
    E = epm.model(sm, Nx, Nt, gseed, m0)
    eta = noise_matrix(sm, Nx, Nt, nseed, nnoise)
    psi = np.linalg.solve(E["D"], eta)
    S, P = slice_sums(eta, psi, Nx, Nt)
    out = {"eta": eta, "psi": psi, "S": S, "P": P, "sigma_min": E["sigma_min"], "D": E["D"]}
    if Nx % 2 == 0 and Nt % 2 == 0:
        out["phihat_norm"] = epm.schur_propagators(E["D"], Nx, Nt, m0, eta)[1]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def model(sm, Nx, Nt, gseed, m0, nseed, nnoise=NNOISE):
    """The dense model of one (field, mass, noise seed), computed once per session and read-only."""
    epm._SM[id(sm)] = sm
    return _model(id(sm), Nx, Nt, gseed, m0, nseed, nnoise)


def bound(M, Nx, Nt, tol=epm.TOL, even_odd=False):
    """[K]: sqrt(2 Nx) tol beta_k / sigma_min(D), without the margin; the same for every t, S and P."""
    K = M["eta"].shape[1]
    beta = M["phihat_norm"] if even_odd else np.full(K, np.sqrt(2.0 * Nx * Nt))
    return np.sqrt(2.0 * Nx) * tol * beta / M["sigma_min"]


def loops_array(S, P):
    """(K, Nt, 2) complex, the layout Lattice.quark_loops returns."""
    return np.stack([S, P], axis=2)


def singlet_correlator(G, Nx, Nt, nf=NF):
    """(C_pi, C_eta), each (Nt,), straight from G = D^-1, averaged over every source site n0 and
    shifted to dt = t - t0: the connected piece sum_x tr[gamma5 S(n, n0) gamma5 S(n0, n)] (written with
    both propagators, no gamma5-hermiticity) and the full Wick contraction, connected - nf sum_x
    tr[gamma5 S(n, n)] tr[gamma5 S(n0, n0)]."""
    V = Nx * Nt
    g5 = np.repeat([1.0, -1.0], V)
    H = g5[:, None] * G                                     # gamma5 D^-1
    W = (H * H.T).reshape(2, V, 2, V).sum(axis=(0, 2))      # W[n, n0] = tr[g5 S(n, n0) g5 S(n0, n)]
    loop = np.diagonal(H).reshape(2, V).sum(axis=0)          # tr g5 S(n, n)
    W = W.reshape(Nx, Nt, Nx, Nt)
    L = loop.reshape(Nx, Nt)
    conn, disc = np.zeros(Nt, dtype=np.complex128), np.zeros(Nt, dtype=np.complex128)
    for t0 in range(Nt):
        for dt in range(Nt):
            t = (t0 + dt) % Nt
            conn[dt] += W[:, t, :, t0].sum()
            disc[dt] += L[:, t].sum() * L[:, t0].sum()
    conn /= V
    disc /= V
    return conn, conn - nf * disc


def pion_all_sources(G, Nx, Nt):
    """The library's pion correlator sum_x tr S S^dag averaged over every source site, shifted to dt."""
    V = Nx * Nt
    A = (G.real ** 2 + G.imag ** 2).reshape(2, Nx, Nt, 2, Nx, Nt).sum(axis=(0, 1, 3, 4))   # [t, t0]
    return np.array([sum(A[(t0 + dt) % Nt, t0] for t0 in range(Nt)) for dt in range(Nt)]) / V
