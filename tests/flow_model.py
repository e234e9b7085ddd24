"""Host model of sm_topology and sm_wilson_flow: numpy only, no code shared with the
library under test.

Fields are complex arrays of shape (2, Nx, Nt): plane 0 = U_t, plane 1 = U_x, and
"n+0" is t+1 (the conventions of sm_gauge.hip). With

    U_01(n) = U_0(n) U_1(n+t) U_0*(n+x) U_1*(n)

the three sums are

    action = sum_n (1 - Re U_01(n))
    q_geo  = (1 / 2 pi) sum_n atan2(Im U_01(n), Re U_01(n))
    q_sin  = (1 / 2 pi) sum_n Im U_01(n)

and the flow d theta_mu(n) / dt = Z_mu(n) = -Im(U_mu(n) conj(S_mu(n))), S the
staples from their definition

    S_0(n) = U_1(n) U_0(n+x) U_1*(n+t) + U_1*(n-x) U_0(n-x) U_1(n-x+t)
    S_1(n) = U_0(n) U_1(n+t) U_0*(n+x) + U_0*(n-t) U_1(n-t) U_0(n-t+x)

is integrated by Luescher's third-order scheme in its one-accumulator form; one step
of size eps is

    A = eps Z(W);                          W <- W exp(i A / 4)
    A = (8/9) eps Z(W) - (17/36) A;        W <- W exp(i A)
    A = (3/4) eps Z(W) - A;                W <- W exp(i A)

with exp(i y) = (cos y, sin y). Every complex product is written out as
(ac - bd, ad + bc) on the real and imaginary parts, each operation rounded on its
own: the expression the device evaluates without fused multiply-adds, which numpy's
own complex product does not promise.

dtype = numpy.float64 is the model the device is compared with; dtype =
numpy.longdouble runs the same recurrence in extended precision and serves only to
measure the double model's own rounding (delta_ref).

The keyword arguments of flow_step after `dtype` each damage ONE part of the
definition; the host test shows that every such change moves a flowed link far
outside the tolerance the device is held to.
"""
import numpy as np

ALLOWED_FACTOR = 32.0   # allowed = 32 * delta_ref
SIGMA = 0.4242          # width of the Gaussian link noise on the backgrounds

# (Nx, Nt, Q, noise seed, eps, nsteps, meas_every) of the device comparison. The seeds
# are ones for which every plaquette angle stays more than 0.2 away from +-pi along the
# whole flow (the host test asserts it), so q_geo is Q at every step: a plaquette that
# flows through -1 has its charge decided by the last bit.
CASES = [(2, 8, 1, 100, 0.05, 10, 5), (4, 4, 1, 101, 0.1, 10, 5), (5, 9, -2, 102, 0.05, 20, 5),
         (6, 10, 1, 103, 0.1, 10, 2), (16, 16, 3, 104, 0.02, 30, 10), (37, 130, -5, 115, 0.05, 10, 5)]
CASE_IDS = [f"{c[0]}x{c[1]}_Q{c[2]}" for c in CASES]
# More sites than the stage launch's block cap times 256 (its grid-stride loop runs
# twice): topology and one step only. Among 10^6 plaquette angles of width 2 SIGMA some
# reach +-pi, so this field's noise is narrower: 0.2 keeps them 7 widths away.
LARGE = (1025, 1030, 7, 7, 0.05, 1, 1)
LARGE_SIGMA = 0.2


def _ctype(dtype):
    return np.clongdouble if dtype is np.longdouble else np.complex128


def cmul(a, b):
    out = np.empty_like(a)
    out.real = a.real * b.real - a.imag * b.imag
    out.imag = a.real * b.imag + a.imag * b.real
    return out


def _xp(a):
    return np.roll(a, -1, axis=0)   # a(n + x)


def _xm(a):
    return np.roll(a, 1, axis=0)    # a(n - x)


def _tp(a):
    return np.roll(a, -1, axis=1)   # a(n + t)


def _tm(a):
    return np.roll(a, 1, axis=1)    # a(n - t)


def background(Nx, Nt, Q, seed, sigma=SIGMA, gauge_seed=None):
    """A charge-Q field of constant field strength F = 2 pi Q / (Nx Nt),
        theta_x(x, t) = F t,   theta_t(x, t) = -F Nt x on t = Nt - 1 and 0 elsewhere,
    every link multiplied by exp(i sigma g), g standard normal from numpy's seeded
    default generator; gauge_seed: a random gauge transformation on top."""
    F = 2.0 * np.pi * Q / (Nx * Nt)
    x, t = np.meshgrid(np.arange(Nx, dtype=np.float64), np.arange(Nt, dtype=np.float64), indexing="ij")
    theta = np.zeros((2, Nx, Nt))
    theta[1] = F * t
    theta[0][:, Nt - 1] = -F * Nt * x[:, Nt - 1]
    if sigma:
        theta = theta + sigma * np.random.default_rng(seed).standard_normal((2, Nx, Nt))
    U = np.exp(1j * theta)
    return U if gauge_seed is None else gauge_transform(U, gauge_seed)


def gauge_transform(U, seed):
    """U_mu(n) -> Omega(n) U_mu(n) Omega*(n + mu) with random phases Omega."""
    _, Nx, Nt = U.shape
    om = np.exp(1j * np.random.default_rng(seed).uniform(-np.pi, np.pi, (Nx, Nt)))
    return np.stack([om * U[0] * np.conj(_tp(om)), om * U[1] * np.conj(_xp(om))])


def plaquette(U):
    U0, U1 = U[0], U[1]
    return cmul(cmul(cmul(U0, _tp(U1)), np.conj(_xp(U0))), np.conj(U1))


def topology(U, dtype=np.float64):
    """(action, q_geo, q_sin, margin): the three sums and the smallest distance of a
    plaquette angle from +-pi, all in dtype."""
    P = plaquette(np.asarray(U).astype(_ctype(dtype)))
    pi = np.arctan2(dtype(0.0), dtype(-1.0))
    ang = np.arctan2(P.imag, P.real)
    return ((dtype(1.0) - P.real).sum(), ang.sum() / (dtype(2.0) * pi), P.imag.sum() / (dtype(2.0) * pi),
            (pi - np.abs(ang)).min())


def staples(U, wrong_neighbour=False):
    U0, U1 = U[0], U[1]
    far = _xm if not wrong_neighbour else _xp   # damage: the backward staple of S_0 from n+x instead of n-x
    S0 = cmul(cmul(U1, _xp(U0)), np.conj(_tp(U1))) + cmul(cmul(np.conj(far(U1)), far(U0)), _tp(far(U1)))
    S1 = cmul(cmul(U0, _tp(U1)), np.conj(_xp(U0))) + cmul(cmul(np.conj(_tm(U0)), _tm(U1)), _xp(_tm(U0)))
    return np.stack([S0, S1])


def flow_force(U, zsign=-1.0, wrong_neighbour=False):
    """Z_mu(n) = -Im(U_mu(n) conj(S_mu(n)))."""
    z = cmul(U, np.conj(staples(U, wrong_neighbour))).imag
    return -z if zsign < 0 else z


def _rotate(W, y):
    e = np.empty(y.shape, dtype=W.dtype)
    e.real = np.cos(y)
    e.imag = np.sin(y)
    return cmul(W, e)


def flow_step(W, eps, dtype=np.float64, c2=(17.0, 36.0), stage1=True, zsign=-1.0, wrong_neighbour=False, rot0=0.25):
    """One step of size eps from W (not modified). c2: numerator and denominator of
    17/36; stage1 = False drops stage 1; zsign = +1 flips the force; wrong_neighbour
    takes one staple from the wrong site; rot0: stage 0's rotation factor."""
    eps = dtype(eps)
    Z = lambda V: flow_force(V, zsign, wrong_neighbour)   # noqa: E731
    A = eps * Z(W)
    W = _rotate(W, dtype(rot0) * A)
    if stage1:
        A = (dtype(8.0) / dtype(9.0)) * (eps * Z(W)) - (dtype(c2[0]) / dtype(c2[1])) * A
        W = _rotate(W, A)
    A = dtype(0.75) * (eps * Z(W)) - A
    return _rotate(W, A)


def flow(U, eps, nsteps, dtype=np.float64, **damage):
    """The fields after 0, 1, ..., nsteps steps, as a list."""
    W = np.asarray(U).astype(_ctype(dtype))
    out = [W]
    for _ in range(nsteps):
        W = flow_step(W, eps, dtype, **damage)
        out.append(W)
    return out


def max_component_deviation(A, B):
    A, B = np.asarray(A), np.asarray(B)
    return float(max(np.abs(A.real - B.real).max(), np.abs(A.imag - B.imag).max()))


def delta_ref(U, eps, nsteps):
    """The double model against the extended-precision one: ([largest component
    deviation up to and including each step 0..nsteps], [double-model field after each
    step])."""
    assert np.finfo(np.longdouble).eps < 1e-18, "numpy.longdouble is no wider than double here"
    fd, fl = flow(U, eps, nsteps, np.float64), flow(U, eps, nsteps, np.longdouble)
    worst, deltas = 0.0, []
    for a, b in zip(fd, fl):
        worst = max(worst, max_component_deviation(a, b))
        deltas.append(worst)
    return deltas, fd
