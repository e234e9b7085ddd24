"""Plain numpy models of the first CG iterates on Dhat Dhat^dag, the even-odd
operator (test helper; the full operator's are in mixed_model.py).

    Dhat = m - (1/m) D_eo D_oe  on the even sites ((x + t) even), m = m0 + 2,

composed from a full Dirac apply and parity masks: the odd part of D v_e is
D_oe v_e, the even part of D w_o is D_eo w_o (the mass term is diagonal). The
reference of every check composes it from the CPU oracle's oracle_dirac; the
numpy operator (np.roll, complex128 or complex64) is shown equal to that one
in test_eo_mixed_model_host.py. Nothing here uses the GPU.

A mixed even-odd solve (sm_eo_cg_precision = 1) cut off at max_iter = k returns
x_k = phi_e + (the fp32 correction, folded): the k-th CG iterate from
x0 = phi_e. Two references of that quantity:

  cg_iterates_fp64        textbook CG in fp64 on the oracle-composed operator;
  cg_iterates_fp32_model  the fp32 pass's recurrence (sm_eosp.hip's header)
                          without reliable updates, on the complex64 operator.

deviation() and bound() are mixed_model.py's: the GPU tests allow 8x the
model's own worst deviation (at least 2^-23), never a figure from the kernel.

solve_model() is the whole reliable-update scheme (sm_eomp.cpp) in numpy, for
the iteration-count ratios of test_eo_mixed_model_host.py.

Fields are the library's: 4 S doubles, plane 0 then plane 1, each (Nx, Nt)
row-major interleaved complex; even vectors carry zeros on the odd sites.
"""
import numpy as np

import mixed_model as mm
from conftest import ptr

deviation = mm.deviation
model_deviation = mm.model_deviation
bound = mm.bound
synthetic = mm.synthetic
to_planes = mm.to_planes
from_planes = mm.from_planes
rdot = mm.rdot


def even_mask(Nx, Nt):
    x, t = np.meshgrid(np.arange(Nx), np.arange(Nt), indexing="ij")
    return (x + t) % 2 == 0


def even_part(v, Nx, Nt):
    """4 S doubles with the odd sites zeroed."""
    return from_planes(to_planes(v, Nx, Nt) * even_mask(Nx, Nt))


def oracle_dirac(oracle, Nx, Nt, U, v, m0, dag):
    S = Nx * Nt
    out = np.empty(4 * S)
    oracle.oracle_dirac(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(v[:2 * S]), ptr(v[2 * S:]), ptr(out[:2 * S]),
                        ptr(out[2 * S:]), m0, dag)
    return out


def oracle_dhat(oracle, Nx, Nt, U, v, m0, dag):
    """Dhat v_e (dag = 0) / Dhat^dag v_e (1) from two oracle_dirac calls and masks."""
    m = m0 + 2.0
    ve = even_part(v, Nx, Nt)
    w = oracle_dirac(oracle, Nx, Nt, U, ve, m0, dag)
    wo = w - even_part(w, Nx, Nt)
    z = oracle_dirac(oracle, Nx, Nt, U, wo, m0, dag)
    return m * ve - (1.0 / m) * even_part(z, Nx, Nt)


def oracle_dhatdhat(oracle, Nx, Nt, U, v, m0):
    return oracle_dhat(oracle, Nx, Nt, U, oracle_dhat(oracle, Nx, Nt, U, v, m0, 1), m0, 0)


def np_dhat(links, p, mass, dagger):
    """Dhat / Dhat^dag on (2, Nx, Nt) arrays in p's precision; links = mm.signed_links()."""
    dt = p.dtype.type
    rt = p.real.dtype.type
    even = even_mask(*p.shape[1:]).astype(rt)
    odd = rt(1) - even
    pe = p * even
    w = mm.np_dirac(links, pe, mass, dagger) * odd
    z = mm.np_dirac(links, w, mass, dagger) * even
    out = dt(mass) * pe - dt(rt(1.0 / mass)) * z
    assert out.dtype == p.dtype
    return out


def np_dhatdhat(links, p, mass):
    return np_dhat(links, np_dhat(links, p, mass, 1), mass, 0)


def cg_iterates_fp64(oracle, Nx, Nt, U, phi, m0, K):
    """x_1 .. x_K of textbook CG on the oracle-composed Dhat Dhat^dag from x0 = phi_e, no stop test."""
    A = lambda v: oracle_dhatdhat(oracle, Nx, Nt, U, v, m0)  # noqa: E731
    x = even_part(phi, Nx, Nt)
    r = x - A(x)
    d = r.copy()
    rr = float(np.dot(r, r))
    out = []
    for _ in range(K):
        Ad = A(d)
        alpha = rr / float(np.dot(d, Ad))
        x = x + alpha * d
        r = r - alpha * Ad
        rn = float(np.dot(r, r))
        d = r + (rn / rr) * d
        rr = rn
        out.append(x.copy())
    return out


def cg_iterates_fp32_model(Nx, Nt, U, phi, m0, K, mutate=None):
    """phi_e + y_k, k = 1 .. K, of the fp32 pass's recurrence without reliable
    updates: r_0 the fp64 true residual rounded to complex64, y from 0 in
    complex64, dots in fp64 (<d, Ad> as |Dhat^dag d|^2), alpha and beta formed
    in fp64 and used as fp32, beta_j from the estimate |r_j|^2 - 2 a <r_j, Ad_j>
    + a^2 |Ad_j|^2, and r_{j-1} rebuilt as d_{j-1} - beta_{j-2} d_{j-2}.
    mutate(links32): a hook to damage the fp32 operator's links in place."""
    mass = m0 + 2.0
    l64 = mm.signed_links(U, Nx, Nt)
    p = to_planes(even_part(phi, Nx, Nt), Nx, Nt)
    r0 = (p - np_dhatdhat(l64, p, mass)).astype(np.complex64)
    l32 = mm.signed_links(U, Nx, Nt, np.complex64)
    if mutate is not None:
        mutate(l32)
    f = np.float32
    d, dprev, beta_prev = r0.copy(), r0.copy(), f(0)
    y = np.zeros_like(r0)
    out = []
    for _ in range(K):
        r = d - beta_prev * dprev
        W = np_dhat(l32, d, f(mass), 1)
        Ad = np_dhat(l32, W, f(mass), 0)
        rr, dA, rA, AA = rdot(r, r), rdot(W, W), rdot(r, Ad), rdot(Ad, Ad)
        alpha = rr / dA
        beta = (rr - 2.0 * alpha * rA + alpha * alpha * AA) / rr
        y = y + f(alpha) * d
        rn = r - f(alpha) * Ad
        dprev, d, beta_prev = d, rn + f(beta) * d, f(beta)
        assert y.dtype == np.complex64 and d.dtype == np.complex64
        out.append(from_planes(p + y.astype(np.complex128)))
    return out


def fp64_cg_count(Nx, Nt, U, phi, m0, tol, max_iter=10000):
    """Iterations of plain fp64 CG on the complex128 numpy Dhat Dhat^dag from
    x0 = phi_e to the iterated |r| < tol |phi_e| (the library's stop test)."""
    mass = m0 + 2.0
    l64 = mm.signed_links(U, Nx, Nt)
    p = to_planes(even_part(phi, Nx, Nt), Nx, Nt)
    target = tol * np.sqrt(rdot(p, p))
    r = p - np_dhatdhat(l64, p, mass)
    d, rr = r.copy(), rdot(r, r)
    for k in range(1, max_iter + 1):
        Ad = np_dhatdhat(l64, d, mass)
        alpha = rr / rdot(d, Ad)
        r = r - alpha * Ad
        rn = rdot(r, r)
        if np.sqrt(rn) < target:
            return k
        d, rr = r + (rn / rr) * d, rn
    return max_iter


def solve_model(Nx, Nt, U, phi, m0, tol, delta=0.1, keep_direction=True, max_iter=10000):
    """The mixed solve of sm_eomp.cpp in numpy: fp32 segments (complex64
    operator, the pass's recurrence and scalar step) between fp64 true
    residuals; keep_direction = False restarts every segment from d_0 = r (a
    plain defect correction). Returns (inner iterations, updates, final true
    relative residual)."""
    mass = m0 + 2.0
    l64 = mm.signed_links(U, Nx, Nt)
    l32 = mm.signed_links(U, Nx, Nt, np.complex64)
    f = np.float32
    p = to_planes(even_part(phi, Nx, Nt), Nx, Nt)
    phi_norm = np.sqrt(rdot(p, p))
    x = p.copy()
    r = p - np_dhatdhat(l64, x, mass)
    k_total, updates, rn_prev, dkeep = 0, 0, 0.0, None
    while True:
        true_rr = rdot(r, r)
        if np.sqrt(true_rr) < tol * phi_norm or k_total >= max_iter:
            return k_total, updates, np.sqrt(true_rr) / phi_norm
        beta0 = true_rr / rn_prev if (keep_direction and dkeep is not None and rn_prev > 0.0) else 0.0
        r32 = r.astype(np.complex64)
        if beta0 == 0.0:
            dprev = r32.copy()
            d = r32.copy()
        else:
            dprev = dkeep
            d = r32 + f(beta0) * dprev
        beta_prev = f(beta0)
        y = np.zeros_like(r32)
        M = np.sqrt(true_rr)
        alpha = 0.0
        j = 0
        while True:
            rj = d - beta_prev * dprev
            W = np_dhat(l32, d, f(mass), 1)
            Ad = np_dhat(l32, W, f(mass), 0)
            rr, dA, rA, AA = rdot(rj, rj), rdot(W, W), rdot(rj, Ad), rdot(Ad, Ad)
            if j > 0:
                y = y + f(alpha) * dprev  # iteration j is complete: x_j = x_{j-1} + alpha_{j-1} d_{j-1}
                k_total += 1
                err = np.sqrt(rr)
                M = max(M, err)
                if err < tol * phi_norm or err < delta * M or k_total >= max_iter:
                    break  # rn_prev = |r_{j-1}|^2 and dprev = d_{j-1} stay for the injection
            alpha = rr / dA
            beta = (rr - 2.0 * alpha * rA + alpha * alpha * AA) / rr
            rn_prev = rr
            rnew = rj - f(alpha) * Ad
            dprev, d, beta_prev = d, rnew + f(beta) * d, f(beta)
            j += 1
        dkeep = dprev
        x = x + y.astype(np.complex128)
        r = p - np_dhatdhat(l64, x, mass)
        updates += 1
