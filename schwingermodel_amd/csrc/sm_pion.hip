// sm_pion.hip -- the small kernels of the pion correlator's measurement layer
// (gfx950; host: sm_pion.cpp): point sources for K columns in the full or the
// checkerboard layout, the two additions of the even-odd propagator
//     phihat_e = phi_e + (1/2m) H_eo phi_o,   S_o = (1/m) phi_o + (1/2m) H_oe S_e
// (the hops are sm_eobatch.hip's launch_eob_hop, mode 2), and the time-slice
// sums of two spin columns per replica.
//
// All of them are latency-sized: one thread per column, per half-lattice entry
// or per (t, x-group); column / replica b = blockIdx.y with its mass from
// massv[b] (block-uniform, a scalar load). No atomics; the slice sums add in
// pion_slices_kernel's order (sm_cgbatch.hip), so a replica's C is bitwise what
// that kernel gives the same two fields.
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

namespace {

// Column k of a zeroed field = the unit vector at (sx[s], st[s]) of plane a,
// with (s, a) = (k / 2, k % 2) when per_col, else (s0, a0) for every column.
// full != null: K columns 2V complex apart; else checkerboard columns V complex
// apart (two planes of V / 2), the site's parity choosing e or o.
__global__ void pion_sources_kernel(int K, int Wt, long V, const int *sx, const int *st, int s0, int a0, int per_col,
                                    double2 *full, double2 *e, double2 *o) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int s = per_col ? k >> 1 : s0, al = per_col ? k & 1 : a0;
    const int x = sx[s], t = st[s];
    const double2 one = make_double2(1.0, 0.0);
    if (full) {
        full[(long)k * 2 * V + (long)al * V + (long)x * Wt + t] = one;
        return;
    }
    double2 *dst = ((x + t) & 1) ? o : e;
    dst[(long)k * V + (long)al * (V / 2) + (long)x * (Wt / 2) + (t >> 1)] = one;
}

// out_b += a_b (INV = 0) or out_b += a_b / m_b (INV = 1) on columns of n complex
template <int INV>
__global__ void __launch_bounds__(256) pion_eo_add_kernel(long n, const double2 *a, double2 *out, const double *massv,
                                                          double mass) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    const double m = massv ? massv[b] : mass;
    const double2 v = a[b * n + i], w = out[b * n + i];
    const double2 sv = INV ? make_double2(v.x / m, v.y / m) : v;
    out[b * n + i] = make_double2(sv.x + w.x, sv.y + w.y);
}

// C[b * cstride + t] = sum_x (|A_b,0|^2 + |A_b,1|^2 + |B_b,0|^2 + |B_b,1|^2)(x, t), A_b / B_b = column b
// (2V complex apart) of the spin-0 / spin-1 propagators. pion_slices_kernel's block and order: thread
// (tl, xg) sums rows xg, xg + 4, ..., spin 0 then 1, plane 0 then 1; then the four groups in order.
__global__ void __launch_bounds__(256) ens_pion_slices_kernel(int Nx, int Wt, long V, const double2 *A, const double2 *B,
                                                              double *C, long cstride) {
    __shared__ double sh[4][64];
    const int tl = threadIdx.x & 63, xg = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl;
    const long b = blockIdx.y;
    double acc = 0.0;
    if (t < Wt) {
        const double2 *S0 = A + b * 2 * V + t, *S1 = B + b * 2 * V + t;
        for (int x = xg; x < Nx; x += 4) {
            const long n = (long)x * Wt;
            const double2 v00 = S0[n], v01 = S0[n + V], v10 = S1[n], v11 = S1[n + V];
            acc += v00.x * v00.x + v00.y * v00.y;
            acc += v01.x * v01.x + v01.y * v01.y;
            acc += v10.x * v10.x + v10.y * v10.y;
            acc += v11.x * v11.x + v11.y * v11.y;
        }
    }
    sh[xg][tl] = acc;
    __syncthreads();
    if (xg == 0 && t < Wt) C[b * cstride + t] = ((sh[0][tl] + sh[1][tl]) + sh[2][tl]) + sh[3][tl];
}

}  // namespace

void launch_pion_sources(hipStream_t s, const Geometry &g, int K, const PionCols &src, double2 *full, double2 *e,
                         double2 *o) {
    hipLaunchKernelGGL(pion_sources_kernel, dim3((K + 63) / 64), dim3(64), 0, s, K, g.Wt, g.V, src.sx, src.st, src.s0,
                       src.a0, src.per_col, full, e, o);
}

void launch_pion_eo_add(hipStream_t s, const Geometry &g, int K, int inv_mass, const double2 *a, double2 *out,
                        const EoBatchLinks &l) {
    const dim3 grid((unsigned)((g.V + 255) / 256), (unsigned)K);
    if (inv_mass) hipLaunchKernelGGL(pion_eo_add_kernel<1>, grid, dim3(256), 0, s, g.V, a, out, l.massv, l.mass);
    else hipLaunchKernelGGL(pion_eo_add_kernel<0>, grid, dim3(256), 0, s, g.V, a, out, l.massv, l.mass);
}

void launch_ens_pion_slices(hipStream_t s, const Geometry &g, int R, const double2 *A, const double2 *B, double *C,
                            long cstride) {
    hipLaunchKernelGGL(ens_pion_slices_kernel, dim3((g.Wt + 63) / 64, R), dim3(256), 0, s, g.Nx, g.Wt, g.V, A, B, C,
                       cstride);
}

}  // namespace sm
