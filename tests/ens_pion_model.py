"""Dense numpy model of the pion correlator (test helper of the ensemble's and
the even-odd correlator's tests).

The Dirac matrix D (2 Nx Nt square, at most 1952) is built column by column
from mixed_model.np_dirac on signed_links; the exact correlator C* comes from
numpy.linalg.solve:
    S_a = D^-1 phi_a,  C*[s, t] = sum_x sum_a (|S_a,0(x,t)|^2 + |S_a,1(x,t)|^2).

schur_correlator is the even-odd path of sm_pion.cpp written from the blocks of
that matrix (m = m0 + 2, D_ee = D_oo = m, D_eo = -H_eo / 2):
    phihat_e = phi_e - D_eo phi_o / m,   Dhat = m - D_eo D_oe / m
    S_e = Dhat^-1 phihat_e,              S_o = (phi_o - D_oe S_e) / m
with switches for the damaged variants the host test must see rejected.

The end-to-end bound, derived: both solvers stop on ||r|| < tol ||b||, so S
satisfies ||D S - phi|| <= tol max(1, ||phihat_e||) (D D^dag: b = phi of norm 1;
even-odd: the residual of the full system is the even one's, the odd rows being
solved exactly by the reconstruction). Hence ||dS_a|| <= eps_a = tol max(1,
||phihat_e||) / sigma_min(D) and
    |C - C*|[t] <= sum_a (2 ||S*_a(., t)|| eps_a + eps_a^2).
The tests allow MARGIN = 2 x that: the stop test is on the recursive residual,
and the reconstruction rounds at 1e-15.

Fields are the library's: 4 S doubles, plane 0 then plane 1, each (Nx, Nt)
row-major (t fastest), interleaved complex.
"""
import functools

import numpy as np

import mixed_model as mm

TOL, MAX_ITER = 1e-10, 10000
MARGIN = 2.0
SIGMA = 0.3246
SHAPES_EVEN = [(6, 10), (16, 16), (16, 62), (8, 122)]
SHAPES_ALL = [(6, 10), (16, 16), (5, 9), (16, 62), (8, 122)]
SEEDS = (4321, 777, 90210)
MASSES = (-0.10, 0.0, 0.05)


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def sources(Nx, Nt):
    """Both site parities and both t-boundary wraps."""
    return [(0, 0), (Nx - 1, Nt - 1), (Nx // 2, Nt // 3), (1, 0)]


def gauge(sm, Nx, Nt, seed):
    """The library's host draw: 4 S doubles."""
    return mm.synthetic(sm, Nx, Nt, sigma=SIGMA, gauge_seed=seed)[0]


def as_complex(U, Nx, Nt):
    """(2, V) complex128, the layout Ensemble.upload_gauge takes."""
    return np.ascontiguousarray(U.view(np.complex128).reshape(2, Nx * Nt))


def dense_dirac(U, Nx, Nt, m0, chunk=244):
    """D as an (n, n) matrix, n = 2 Nx Nt, index = plane * V + x * Nt + t."""
    n = 2 * Nx * Nt
    ut, ux = mm.signed_links(U, Nx, Nt)
    links = [ut[..., None], ux[..., None]]
    D = np.empty((n, n), dtype=np.complex128)
    for j0 in range(0, n, chunk):
        j1 = min(n, j0 + chunk)
        e = np.zeros((n, j1 - j0), dtype=np.complex128)
        e[np.arange(j0, j1), np.arange(j1 - j0)] = 1.0
        D[:, j0:j1] = mm.np_dirac(links, e.reshape(2, Nx, Nt, j1 - j0), m0 + 2.0, 0).reshape(n, j1 - j0)
    return D


def source_matrix(Nx, Nt, src):
    """(n, 2 nsrc): column 2 s + a = the unit vector at source s of plane a."""
    V = Nx * Nt
    phi = np.zeros((2 * V, 2 * len(src)), dtype=np.complex128)
    for s, (x, t) in enumerate(src):
        for a in (0, 1):
            phi[a * V + x * Nt + t, 2 * s + a] = 1.0
    return phi


def slices(S, Nx, Nt, nsrc, spins=(0, 1)):
    """C[s, t] from the propagator columns S (n, 2 nsrc)."""
    w = (S.real ** 2 + S.imag ** 2).reshape(2, Nx, Nt, nsrc, 2)
    return w[..., list(spins)].sum(axis=(0, 1, 4)).T


def parity_sets(Nx, Nt):
    x, t = np.meshgrid(np.arange(Nx), np.arange(Nt), indexing="ij")
    par = np.tile(((x + t) & 1).reshape(-1), 2)
    return np.flatnonzero(par == 0), np.flatnonzero(par == 1)


def schur_propagators(D, Nx, Nt, m0, phi, drop_phi_o_term=False, drop_heo_term=False, flip_parity=False):
    """S (n, K) through the even-odd system, and ||phihat_e|| per column."""
    m = m0 + 2.0
    ev, od = parity_sets(Nx, Nt)
    Deo, Doe = D[np.ix_(ev, od)], D[np.ix_(od, ev)]
    pe, po = phi[ev], phi[od]
    if flip_parity:
        pe, po = po, pe
    ph = pe.copy()
    if not drop_heo_term:
        ph = ph - Deo @ po / m
    Dhat = m * np.eye(len(ev)) - Deo @ Doe / m
    Se = np.linalg.solve(Dhat, ph)
    So = -(Doe @ Se) / m
    if not drop_phi_o_term:
        So = So + po / m
    S = np.empty_like(phi)
    S[ev], S[od] = Se, So
    return S, np.linalg.norm(ph, axis=0)


@functools.lru_cache(maxsize=None)
def _model(sm_key, Nx, Nt, seed, m0):
    sm = _SM[sm_key]
    U = gauge(sm, Nx, Nt, seed)
    src = sources(Nx, Nt)
    D = dense_dirac(U, Nx, Nt, m0)
    phi = source_matrix(Nx, Nt, src)
    S = np.linalg.solve(D, phi)
    smin = float(np.sqrt(np.linalg.eigvalsh(D.conj().T @ D)[0]))
    out = {"U": U, "src": src, "D": D, "phi": phi, "S": S, "C": slices(S, Nx, Nt, len(src)), "sigma_min": smin}
    if Nx % 2 == 0 and Nt % 2 == 0:
        out["phihat_norm"] = schur_propagators(D, Nx, Nt, m0, phi)[1]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


_SM = {}


def model(sm, Nx, Nt, seed, m0):
    """The dense model of one (field, mass), computed once per session and read-only."""
    _SM[id(sm)] = sm
    return _model(id(sm), Nx, Nt, seed, m0)


def bound(M, Nx, Nt, tol=TOL, even_odd=False):
    """[nsrc, Nt]: sum_a (2 ||S*_a(., t)|| eps_a + eps_a^2), without the margin."""
    nsrc = len(M["src"])
    rhs = np.maximum(1.0, M["phihat_norm"]) if even_odd else np.ones(2 * nsrc)
    eps = tol * rhs / M["sigma_min"]                                   # per column 2 s + a
    w = (M["S"].real ** 2 + M["S"].imag ** 2).reshape(2, Nx, Nt, nsrc, 2)
    norm_t = np.sqrt(w.sum(axis=(0, 1)))                               # (Nt, nsrc, 2)
    e = eps.reshape(nsrc, 2)
    return (2.0 * norm_t * e[None] + e[None] ** 2).sum(axis=2).T
