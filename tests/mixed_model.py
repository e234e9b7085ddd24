"""Plain numpy models of the first CG iterates on D D^dag (test helper).

A mixed-precision solve (sm_cg_precision = 1) cut off at max_iter = k returns
x_k = phi + (the fp32 correction, folded): the k-th CG iterate from x0 = phi.
Two references of that quantity:

  cg_iterates_fp64        textbook CG in fp64 on the oracle's D D^dag;
  cg_iterates_fp32_model  the fp32 pass's recurrence (sm_cgsp.hip) without
                          reliable updates, on a complex64 np.roll operator.

The distance between the two is what fp32 arithmetic alone costs; the GPU
tests allow 8x that (bound()), computed per case and never from the kernel.

Fields are the library's: 4 S doubles, plane 0 then plane 1, each (Nx, Nt)
row-major (t fastest) interleaved complex.
"""
import numpy as np

from conftest import ptr


def synthetic(sm, Nx, Nt, sigma=0.3246, gauge_seed=4321, spinor_seed=5678):
    S = Nx * Nt
    U, psi = np.empty(4 * S), np.empty(4 * S)
    sm.lib.sm_fill_gauge(gauge_seed, sigma, Nt, 0, Nx, 0, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]))
    sm.lib.sm_fill_spinor(spinor_seed, Nt, 0, Nx, 0, Nt, ptr(psi[:2 * S]), ptr(psi[2 * S:]))
    return U, psi


def oracle_ddag(oracle, Nx, Nt, U, v, m0):
    S = Nx * Nt
    tmp, out = np.empty(4 * S), np.empty(4 * S)
    oracle.oracle_ddag(Nx, Nt, ptr(U[:2 * S]), ptr(U[2 * S:]), ptr(v[:2 * S]), ptr(v[2 * S:]), ptr(tmp[:2 * S]),
                       ptr(tmp[2 * S:]), ptr(out[:2 * S]), ptr(out[2 * S:]), m0)
    return out


def to_planes(v, Nx, Nt):
    """4 S doubles -> complex128 array (2, Nx, Nt)."""
    return v.view(np.complex128).reshape(2, Nx, Nt)


def from_planes(c):
    """complex (2, Nx, Nt) -> 4 S doubles."""
    return np.ascontiguousarray(c, dtype=np.complex128).reshape(-1).view(np.float64).copy()


def signed_links(U, Nx, Nt, dtype=np.complex128):
    """(U_t with the antiperiodic sign of the forward hop out of t = Nt - 1
    folded in, U_x), rounded to dtype: the form the fp32 pass keeps."""
    u = to_planes(U, Nx, Nt)
    ut = u[0].copy()
    ut[:, Nt - 1] *= -1.0
    return [ut.astype(dtype), u[1].astype(dtype)]


def np_dirac(links, p, mass, dagger):
    """D (dagger = 0) / D^dag (1) of the oracle (sm_oracle.c dirac_site) on
    (2, Nx, Nt) arrays; links = signed_links(). The backward t hop into t = 0
    takes conj of the signed link at Nt - 1, i.e. SignL."""
    ut, ux = links
    dt = p.dtype.type
    I, half, mass = dt(1j), dt(0.5), dt(mass)
    p0, p1 = p[0], p[1]
    pt0, pt1 = np.roll(p0, -1, axis=1), np.roll(p1, -1, axis=1)
    pm0, pm1 = np.roll(p0, 1, axis=1), np.roll(p1, 1, axis=1)
    px0, px1 = np.roll(p0, -1, axis=0), np.roll(p1, -1, axis=0)
    pxm0, pxm1 = np.roll(p0, 1, axis=0), np.roll(p1, 1, axis=0)
    a, b = ut, ux
    c, e = np.conj(np.roll(ut, 1, axis=1)), np.conj(np.roll(ux, 1, axis=0))
    if not dagger:
        s0 = mass * p0 - half * (a * (pt0 - pt1) + b * (px0 + I * px1) + c * (pm0 + pm1) + e * (pxm0 - I * pxm1))
        s1 = mass * p1 - half * (a * (pt1 - pt0) + b * (px1 - I * px0) + c * (pm0 + pm1) + e * (I * pxm0 + pxm1))
    else:
        s0 = mass * p0 - half * (c * (pm0 - pm1) + e * (pxm0 + I * pxm1) + a * (pt0 + pt1) + b * (px0 - I * px1))
        s1 = mass * p1 - half * (c * (pm1 - pm0) + e * (pxm1 - I * pxm0) + a * (pt0 + pt1) + b * (I * px0 + px1))
    out = np.stack([s0, s1])
    assert out.dtype == p.dtype
    return out


def np_ddag(links, p, mass):
    return np_dirac(links, np_dirac(links, p, mass, 1), mass, 0)


def rdot(a, b):
    """Re <a, b> in fp64 whatever the fields' precision."""
    a, b = a.astype(np.complex128).ravel(), b.astype(np.complex128).ravel()
    return float(np.dot(a.real, b.real) + np.dot(a.imag, b.imag))


def cg_iterates_fp64(oracle, Nx, Nt, U, phi, m0, K):
    """x_1 .. x_K of textbook CG on D D^dag from x0 = phi, no stop test."""
    A = lambda v: oracle_ddag(oracle, Nx, Nt, U, v, m0)  # noqa: E731
    x = phi.copy()
    r = phi - A(x)
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
    """phi + y_k, k = 1 .. K, of the fp32 pass's recurrence without reliable
    updates: r_0 the fp64 true residual rounded to complex64, y from 0 in
    complex64, dots in fp64, alpha and beta formed in fp64 and used as fp32,
    beta_j from the estimate |r_j|^2 - 2 a <r_j, Ad_j> + a^2 |Ad_j|^2, and
    r_{j-1} rebuilt as d_{j-1} - beta_{j-2} d_{j-2} (sm_cgsp.hip's header).
    mutate(links32): a hook to damage the fp32 operator's links in place."""
    mass = m0 + 2.0
    l64 = signed_links(U, Nx, Nt)
    p = to_planes(phi, Nx, Nt)
    r0 = (p - np_ddag(l64, p, mass)).astype(np.complex64)
    l32 = signed_links(U, Nx, Nt, np.complex64)
    if mutate is not None:
        mutate(l32)
    f = np.float32
    d, dprev, beta_prev = r0.copy(), r0.copy(), f(0)
    y = np.zeros_like(r0)
    out = []
    for _ in range(K):
        r = d - beta_prev * dprev
        Ad = np_ddag(l32, d, f(mass))
        rr, dA, rA, AA = rdot(r, r), rdot(d, Ad), rdot(r, Ad), rdot(Ad, Ad)
        alpha = rr / dA
        beta = (rr - 2.0 * alpha * rA + alpha * alpha * AA) / rr
        y = y + f(alpha) * d
        rn = r - f(alpha) * Ad
        dprev, d, beta_prev = d, rn + f(beta) * d, f(beta)
        assert y.dtype == np.complex64 and d.dtype == np.complex64
        out.append(from_planes(p + y.astype(np.complex128)))
    return out


def deviation(x, x_ref, phi):
    """max |x - x_ref| over sites and components, relative to the largest
    correction max |x_ref - phi| (an L2 norm would dilute a one-column error)."""
    c = lambda v: v.view(np.complex128)  # noqa: E731
    return float(np.abs(c(x) - c(x_ref)).max() / np.abs(c(x_ref) - c(phi)).max())


def model_deviation(model, ref, phi):
    return max(deviation(m, r, phi) for m, r in zip(model, ref))


def bound(model, ref, phi):
    """8 x the model's own worst deviation over the iterates (at least fp32's
    unit roundoff): two summation orders of the model differ by up to 1.3x,
    the kernel is a third ordering with fma and fp64 dots."""
    return 8.0 * max(model_deviation(model, ref, phi), 2.0 ** -23)
