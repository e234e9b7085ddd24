"""Estimators on stochastic quark loops (numpy only; no library call).

`loops` is what Lattice.quark_loops returns: complex of shape (N, Nt, 2) for N
noise vectors, [k, t, 0] = S_k(t) and [k, t, 1] = P_k(t), whose means over k
estimate Tr_t D^-1 and Tr_t gamma5 D^-1 on the time slice t (include/sm_hip.h
"stochastic quark loops"). An ensemble's (R, N, Nt, 2) is used one replica at a
time.
"""
import numpy as np

__all__ = ["condensate", "disconnected", "eta_correlator"]


def _check(loops, who):
    a = np.asarray(loops)
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError(f"{who}: loops has shape {a.shape}, expected (N, Nt, 2)")
    return a


def condensate(loops, V, nf=2):
    """(value, standard error) of the chiral condensate (nf / V) Re Tr D^-1:
    the mean over the noise vectors of c_k = nf / V * Re sum_t S_k(t), and the
    standard error of that mean from the spread of the c_k (0 for one vector).
    V = Nx * Nt."""
    a = _check(loops, "condensate")
    c = (nf / V) * a[:, :, 0].real.sum(axis=1)
    err = float(c.std(ddof=1) / np.sqrt(len(c))) if len(c) > 1 else 0.0
    return float(c.mean()), err


def disconnected(loops):
    """C_disc[dt] = (1 / Nt) sum_t Re [ (sum_k P_k(t)) (sum_k P_k(t + dt)) -
    sum_k P_k(t) P_k(t + dt) ] / (N (N - 1)), t + dt modulo Nt: the estimator of
    (1 / Nt) sum_t Tr_t gamma5 D^-1 Tr_{t+dt} gamma5 D^-1 from N >= 2 vectors. It
    leaves out every product of a vector with itself, so it is unbiased: the
    noise of different vectors is independent."""
    a = _check(loops, "disconnected")
    N, Nt = a.shape[0], a.shape[1]
    if N < 2:
        raise ValueError(f"disconnected: {N} noise vector(s); the unbiased estimator needs at least 2")
    P = a[:, :, 1]
    tot = P.sum(axis=0)
    out = np.empty(Nt)
    for dt in range(Nt):
        cross = tot * np.roll(tot, -dt) - (P * np.roll(P, -dt, axis=1)).sum(axis=0)
        out[dt] = cross.real.sum() / (Nt * N * (N - 1))
    return out


def eta_correlator(C_pi, C_disc, Nx, nf=2):
    """The flavour-singlet pseudoscalar (eta) correlator
        C_eta[dt] = C_pi[dt] - nf * C_disc[dt] / Nx.
    Normalisation: C_pi[dt] = sum_x tr S S^dag from ONE point source, shifted
    to the distance dt = t - t_source (Lattice.pion_correlator's row, rolled);
    it is the connected piece sum_x tr[gamma5 S(n, n0) gamma5 S(n0, n)]. With nf
    degenerate flavours the singlet's Wick contraction subtracts nf times
    sum_x tr[gamma5 S(n, n)] tr[gamma5 S(n0, n0)] = Tr_{t0+dt} gamma5 D^-1 times
    the loop at the one source SITE. Averaged over the source's position that
    site loop is Tr_{t0} gamma5 D^-1 / Nx, and over t0 the product is C_disc of
    disconnected(): hence the 1 / Nx. With C_pi averaged over all sources the
    identity is exact on a single gauge field (tests/test_loops_host.py checks
    it on the dense model); with one source it holds in the ensemble average."""
    return np.asarray(C_pi, dtype=np.float64) - nf * np.asarray(C_disc, dtype=np.float64) / Nx
