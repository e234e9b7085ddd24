// sm_loops.hip -- stochastic quark loops (gfx950; host: sm_loops.cpp): complex
// Z2 x Z2 noise for K columns in one launch, and the contraction that turns the
// batched CG's solution into per-time-slice loops without storing the
// propagator.
//
//   noise        eta_b,a(n) = (+-1 +- i) / sqrt(2) = sm_noise (sm_fields.h) with
//                the key sm_traj_seed(seed[b], k[b]) of column b: a pure
//                function of (seed, k, plane, global site), bitwise what
//                sm_fill_noise writes on the host.
//   contraction  with y_b = (D D^dag)^-1 eta_b: psi_b = D^dag y_b at the site in
//                registers (site_apply<1>, the expression of
//                batch_apply_kernel<1>), eta_b regenerated from the counter,
//                and per column and time slice
//                    S_b(t) = sum_x (conj(eta_0) psi_0 + conj(eta_1) psi_1)
//                    P_b(t) = sum_x (conj(eta_0) psi_0 - conj(eta_1) psi_1)
//                (gamma5 = diag(1, -1)). It reads y (32 B per site and column)
//                and the links (32 B per site, from cache after the first
//                column of a shared field); neither eta nor psi is ever in
//                memory. LOAD = 1 takes psi from memory instead (the even-odd
//                path, whose propagator comes back in the full layout); the
//                sums and their order are the same.
//
// Column b = blockIdx.y reads its links at U + b * ustride and its mass from
// massv[b] (BatchLinks), its seed and k from two small device arrays: all
// block-uniform. t is the contiguous index, so lanes run over t.
#include "sm_device.h"
#include "sm_fields.h"
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

namespace {

constexpr int kLoopXG = 16;  // x-groups of a contraction block (64 t-values each)

__device__ __forceinline__ void noise_site(uint64_t s0, uint64_t s1, uint64_t ng, double2 &e0, double2 &e1) {
    sm_noise_at(s0, ng, &e0.x, &e0.y);
    sm_noise_at(s1, ng, &e1.x, &e1.y);
}

// Column b of `full` (K columns 2V complex apart) or of the checkerboard pair e / o (columns V complex
// apart, two planes of V / 2; the site's parity chooses) = noise vector k[b] of seed[b]. Every site of
// the column is written: no memset ahead of it. Grid (ceil(V / 256), K).
__global__ void __launch_bounds__(256) loops_noise_kernel(int Wt, long V, int Ntg, int t0, const uint64_t *seed,
                                                          const uint64_t *k, double2 *full, double2 *e, double2 *o) {
    const long b = blockIdx.y, n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= V) return;
    const uint64_t key = sm_traj_seed(seed[b], k[b]);
    const int x = (int)(n / Wt), t = (int)(n - (long)x * Wt);
    double2 e0, e1;
    noise_site(sm_noise_stream(key, 0), sm_noise_stream(key, 1), (uint64_t)x * (uint64_t)Ntg + (uint64_t)(t0 + t), e0,
               e1);
    if (full) {
        full[b * 2 * V + n] = e0;
        full[b * 2 * V + V + n] = e1;
        return;
    }
    double2 *dst = ((x + t) & 1) ? o : e;
    const long h = (long)x * (Wt / 2) + (t >> 1);
    dst[b * V + h] = e0;
    dst[b * V + V / 2 + h] = e1;
}

// out[b * ostride + 4 t + (0, 1, 2, 3)] = Re S_b(t), Im S_b(t), Re P_b(t), Im P_b(t). Grid (ceil(Wt / 64), K),
// block 64 t-values x kLoopXG x-groups. Order of the sums, the same for every K, column position and
// LOAD: thread (tl, xg) adds rows xg, xg + kLoopXG, ... in that order, per row
//     S <- (S + conj(eta_0) psi_0) + conj(eta_1) psi_1,   P <- (P + conj(eta_0) psi_0) - conj(eta_1) psi_1
// with separately rounded complex products; then thread (tl, c) adds component c of groups 0, 1, ...,
// kLoopXG - 1 in that order (a group without rows adds +0). No atomics: the same bits on every call.
template <int LOAD>
__global__ void __launch_bounds__(64 * kLoopXG) loops_contract_kernel(int Nx, int Wt, long V, int Ntg, int t0,
                                                                      const double2 *in, BatchLinks l,
                                                                      const uint64_t *seed, const uint64_t *k,
                                                                      double *out, long ostride) {
    __shared__ double sh[4][kLoopXG][64];
    const int tl = threadIdx.x & 63, xg = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl;
    const long b = blockIdx.y;
    const double mass = l.massv ? l.massv[b] : l.mass;
    const uint64_t key = sm_traj_seed(seed[b], k[b]);
    const uint64_t s0 = sm_noise_stream(key, 0), s1 = sm_noise_stream(key, 1);
    const double2 *col = in + b * 2 * V, *U = l.U + b * l.ustride;
    double2 S = make_double2(0.0, 0.0), P = S;
    if (t < Wt) {
        for (int x = xg; x < Nx; x += kLoopXG) {
            double2 p0, p1, e0, e1;
            if (LOAD) {
                const long n = (long)x * Wt + t;
                p0 = col[n];
                p1 = col[n + V];
            } else {
                site_apply<1>(col, U, Nx, Wt, V, mass, x, t, p0, p1);
            }
            noise_site(s0, s1, (uint64_t)x * (uint64_t)Ntg + (uint64_t)(t0 + t), e0, e1);
            const double2 c0 = cmul(cconj(e0), p0), c1 = cmul(cconj(e1), p1);
            S = cadd(cadd(S, c0), c1);
            P = csub(cadd(P, c0), c1);
        }
    }
    sh[0][xg][tl] = S.x;
    sh[1][xg][tl] = S.y;
    sh[2][xg][tl] = P.x;
    sh[3][xg][tl] = P.y;
    __syncthreads();
    if (xg < 4 && t < Wt) {
        double acc = sh[xg][0][tl];
        for (int g = 1; g < kLoopXG; ++g) acc += sh[xg][g][tl];
        out[b * ostride + 4 * (long)t + xg] = acc;
    }
}

}  // namespace

void launch_loops_noise(hipStream_t s, const Geometry &g, int K, const LoopNoise &nz, double2 *full, double2 *e,
                        double2 *o) {
    hipLaunchKernelGGL(loops_noise_kernel, dim3((unsigned)((g.V + 255) / 256), (unsigned)K), dim3(256), 0, s, g.Wt, g.V,
                       g.Ntg, g.t0, nz.seed, nz.k, full, e, o);
}

void launch_loops_contract(hipStream_t s, const Geometry &g, int K, int load_psi, const double2 *in,
                           const BatchLinks &l, const LoopNoise &nz, double *out, long ostride) {
    const dim3 grid((unsigned)((g.Wt + 63) / 64), (unsigned)K), block(64 * kLoopXG);
    if (load_psi)
        hipLaunchKernelGGL(loops_contract_kernel<1>, grid, block, 0, s, g.Nx, g.Wt, g.V, g.Ntg, g.t0, in, l, nz.seed,
                           nz.k, out, ostride);
    else
        hipLaunchKernelGGL(loops_contract_kernel<0>, grid, block, 0, s, g.Nx, g.Wt, g.V, g.Ntg, g.t0, in, l, nz.seed,
                           nz.k, out, ostride);
}

}  // namespace sm
