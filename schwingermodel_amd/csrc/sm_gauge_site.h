// sm_gauge_site.h -- the per-site expressions of the gauge kernels, shared by
// sm_gauge.hip (plaquette sums, staples and gauge force, leapfrog link update)
// and sm_flow.hip (topological charge, Wilson flow), so both evaluate one
// expression in one order: the plaquette, the two staples and exp(i y).
#pragma once
#include "sm_device.h"
#include "sm_internal.h"

#include <float.h>

namespace sm {

struct GArgs {
    const double2 *U;    // 2V: plane 0 U_t, plane 1 U_x
    const double2 *fU;   // 2-deep U faces (nshard > 1)
    long V;
    int Nx, Wt, nshard;
};

inline GArgs gargs(const Geometry &g, int nshard, const double2 *U, const double2 *fU) {
    GArgs a;
    a.U = U;
    a.fU = fU;
    a.V = g.V;
    a.Nx = g.Nx;
    a.Wt = g.Wt;
    a.nshard = nshard;
    return a;
}

// grid of the streaming (non-reducing) kernels over n items: 256 threads, at most 4096 blocks, grid-stride beyond
inline unsigned grid_for(long n) {
    long nb = (n + 255) / 256;
    return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb));
}

// U_plane(x, t = c) for c in [-1, Wt]; x already in [0, Nx).
__device__ __forceinline__ double2 ulink(const GArgs &a, int p, int x, int c) {
    if (c >= 0 && c < a.Wt) return a.U[(long)x * a.Wt + c + p * a.V];
    if (a.nshard == 1) return a.U[(long)x * a.Wt + (c < 0 ? c + a.Wt : c - a.Wt) + p * a.V];
    const int fc = c < 0 ? c + 2 : c - a.Wt + 2;  // face slot of columns -2,-1,Wt,Wt+1
    return a.fU[((long)fc * 2 + p) * a.Nx + x];
}

// ---- plaquette: U_01(n) = U_0(n) U_1(n+0) U*_0(n+1) U*_1(n) ----------------
// src/gauge_conf.cpp:45-49
__device__ __forceinline__ double2 plaquette_site(const GArgs &a, long n) {
    const int x = (int)(n / a.Wt), t = (int)(n - (long)x * a.Wt);
    const int xp = x + 1 == a.Nx ? 0 : x + 1;
    return cmul(cmul(cmul(a.U[n], ulink(a, 1, x, t + 1)), cconj(ulink(a, 0, xp, t))), cconj(a.U[n + a.V]));
}

// ---- staples (src/gauge_conf.cpp:95-125) of the links u0 = U_0(n), u1 = U_1(n) --
//   S_0(n) = U_1(n) U_0(n+1) U*_1(n+0) + U*_1(n-1) U_0(n-1) U_1(n-1+0)
//   S_1(n) = U_0(n) U_1(n+0) U*_0(n+1) + U*_0(n-0) U_1(n-0) U_0(n+1-0)
// (0 = t direction, 1 = x direction; "n+1" is x+1, "n+0" is t+1.)
__device__ __forceinline__ void staples_at(const GArgs &a, long n, double2 u0, double2 u1, double2 &S0, double2 &S1) {
    const int x = (int)(n / a.Wt), t = (int)(n - (long)x * a.Wt);
    const int xp = x + 1 == a.Nx ? 0 : x + 1, xm = x == 0 ? a.Nx - 1 : x - 1;
    S0 = cadd(cmul(cmul(u1, ulink(a, 0, xp, t)), cconj(ulink(a, 1, x, t + 1))),
              cmul(cmul(cconj(ulink(a, 1, xm, t)), ulink(a, 0, xm, t)), ulink(a, 1, xm, t + 1)));
    S1 = cadd(cmul(cmul(u0, ulink(a, 1, x, t + 1)), cconj(ulink(a, 0, xp, t))),
              cmul(cmul(cconj(ulink(a, 0, x, t - 1)), ulink(a, 1, x, t - 1)), ulink(a, 0, xp, t - 1)));
}

// exp(i y) as std::exp of (+-0, y) gives it: glibc cexp = (cos y, sin y) for
// |y| > DBL_MIN and (1, y) below (s_cexp_template.c).
__device__ __forceinline__ double2 cexp_i(double y) {
    double s, c;
    if (fabs(y) > DBL_MIN) {
        sincos(y, &s, &c);
    } else {
        s = y;
        c = 1.0;
    }
    return make_double2(c, s);
}

}  // namespace sm
