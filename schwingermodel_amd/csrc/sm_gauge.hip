// sm_gauge.hip -- gauge-field kernels of the molecular-dynamics step on gfx950
// (SURVEY.md §8f rows 1-3): plaquette field and sums, staples + gauge force,
// the fused momentum / link update of the leapfrog, the momentum kinetic
// energy, and device draws of momenta, pseudofermion sources and gauge fields.
//
// All are single-pass streaming kernels over the shard (HBM-bound, a few bytes
// of neighbour reuse per site that the L2 absorbs); the CG solves they sit
// between dominate an MD step by orders of magnitude. What matters here is
// bit-exact parity with the reference's expressions (same complex-multiply
// order, -ffp-contract=off) and that U, P and F never leave the device.
//
// Neighbour links across the t-shard boundary come from the 2-deep U faces
// ([col -2,-1,Wt,Wt+1][plane][x], exchanged by exchange_ghost_U after every
// link update); one shard wraps periodically in place.
#include "sm_device.h"
#include "sm_fields.h"
#include "sm_gauge_site.h"

namespace sm {

// ---- plaquette sums (U_01(n) = plaquette_site, sm_gauge_site.h) as
// MeasureSp_HMC (src/gauge_conf.cpp:430-440) and Compute_gaugeAction
// (:444-453): partial.x = sum Re U_01, partial.y = sum beta Re(1 - U_01).
__global__ void __launch_bounds__(256) plaquette_kernel(GArgs a, double beta, double2 *field,
                                                        double2 *partials) {
    __shared__ double2 sh[4];
    double2 acc = make_double2(0.0, 0.0);
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x) {
        const double2 P = plaquette_site(a, n);
        if (field) field[n] = P;
        acc.x += P.x;
        acc.y += beta * (1.0 - P.x);
    }
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- staples and gauge force (src/gauge_conf.cpp:95-125; src/hmc.cpp:31-40) --
//   S_mu(n): staples_at (sm_gauge_site.h)
//   F_mu(n) += -beta Im(U_mu(n) conj(S_mu(n)))
__device__ __forceinline__ void staple_site(const GArgs &a, long n, double beta, double *F, double2 *staples) {
    const double2 u0 = a.U[n], u1 = a.U[n + a.V];
    double2 S0, S1;
    staples_at(a, n, u0, u1, S0, S1);
    if (staples) {
        staples[n] = S0;
        staples[n + a.V] = S1;
    }
    if (F) {
        F[n] += -beta * cmul(u0, cconj(S0)).y;
        F[n + a.V] += -beta * cmul(u1, cconj(S1)).y;
    }
}

__global__ void __launch_bounds__(256) staple_force_kernel(GArgs a, double beta, double *F,
                                                           double2 *staples) {
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        staple_site(a, n, beta, F, staples);
}

// ---- leapfrog link / momentum update (src/hmc.cpp:63-101) --------------------
//   do_p:  P += eps * F
//   U *= exp(i coef P): cexp_i (sm_gauge_site.h), then the plain complex
//          product. coef = eps (full step) or 0.5*eps (half).
__device__ __forceinline__ void md_update_link(long i, double2 *U, double *P, const double *F, double eps, int do_p,
                                               double coef) {
    double p = P[i];
    if (do_p) {
        p += eps * F[i];
        P[i] = p;
    }
    U[i] = cmul(U[i], cexp_i(coef * p));
}

__global__ void __launch_bounds__(256) md_update_kernel(long n2, double2 *U, double *P, const double *F,
                                                        double eps, int do_p, double coef) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x)
        md_update_link(i, U, P, F, eps, do_p, coef);
}

// ---- momentum kinetic energy: sum_n 0.5 P_0^2 + 0.5 P_1^2 (src/hmc.cpp:107-111)
__global__ void __launch_bounds__(256) kinetic_kernel(long V, const double *P, double2 *partials) {
    __shared__ double2 sh[4];
    double2 acc = make_double2(0.0, 0.0);
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < V; n += (long)gridDim.x * blockDim.x) {
        acc.x += 0.5 * P[n] * P[n];
        acc.x += 0.5 * P[n + V] * P[n + V];
    }
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- device draws (counter-based, keyed by the GLOBAL site: every sharding
// draws the same global field) ------------------------------------------------
struct DrawArgs {
    uint64_t seed;
    long V;
    int Nx, Wt, t0, Ntg;
};

__device__ __forceinline__ uint64_t global_site(const DrawArgs &a, long n, int &x, int &t) {
    x = (int)(n / a.Wt);
    t = (int)(n - (long)x * a.Wt);
    return (uint64_t)x * (uint64_t)a.Ntg + (uint64_t)(a.t0 + t);
}

// HMC::RandomPI (src/hmc.cpp:5-16): Pi_mu(n) ~ N(0, 1).
__device__ __forceinline__ void draw_momenta_site(const DrawArgs &a, long n, double *P) {
    int x, t;
    const uint64_t ng = global_site(a, n, x, t);
    double g1, g2;
    sm_gauss2(a.seed, SM_STREAM_MOMENTA, ng, &g1, &g2);
    P[n] = g1;
    P[n + a.V] = g2;
}

__global__ void __launch_bounds__(256) draw_momenta_kernel(DrawArgs a, double *P) {
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        draw_momenta_site(a, n, P);
}

// HMC::RandomCHI (src/hmc.cpp:19-28): Re, Im ~ N(0, 1/2) per spin component
// (same streams and scaling as the host spinor generator).
__device__ __forceinline__ void draw_source_site(const DrawArgs &a, long n, double2 *chi) {
    const double s = 0.70710678118654752440084436210485;
    int x, t;
    const uint64_t ng = global_site(a, n, x, t);
    double g1, g2;
    sm_gauss2(a.seed, 4, ng, &g1, &g2);
    chi[n] = make_double2(s * g1, s * g2);
    sm_gauss2(a.seed, 5, ng, &g1, &g2);
    chi[n + a.V] = make_double2(s * g1, s * g2);
}

__global__ void __launch_bounds__(256) draw_source_kernel(DrawArgs a, double2 *chi) {
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        draw_source_site(a, n, chi);
}

// Gauge field of the host generator (sm_fields_fill_gauge), drawn in place.
__global__ void __launch_bounds__(256) draw_gauge_kernel(DrawArgs a, double sigma, double2 *U) {
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x) {
        int x, t;
        const uint64_t ng = global_site(a, n, x, t);
        for (int mu = 0; mu < 2; ++mu) {
            double re, im;
            sm_gauge_link(a.seed, sigma, ng, mu, &re, &im);
            U[n + mu * a.V] = make_double2(re, im);
        }
    }
}

// ---- replica ensemble (sm_ens.cpp): R fields per launch, replica r = blockIdx.y
// Replica r's fields lie r * 2V elements into each array, its parameters in
// par[r] (block-uniform). Per replica every kernel runs the one-field kernel's
// site function over the one-field kernel's grid along x, so the values, the
// partials and their order are those of the one-field launch on that field.
__global__ void __launch_bounds__(256) ens_draws_kernel(DrawArgs a, const EnsPar *par, double *P, double2 *chi) {
    const long off = (long)blockIdx.y * 2 * a.V;
    a.seed = par[blockIdx.y].seed;
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x) {
        draw_momenta_site(a, n, P + off);
        draw_source_site(a, n, chi + off);
    }
}

__global__ void __launch_bounds__(256) ens_md_update_kernel(long n2, double2 *U, double *P, const double *F,
                                                            const EnsPar *par, int do_p, double cfac) {
    const long off = (long)blockIdx.y * n2;
    const double eps = par[blockIdx.y].eps;
    const double coef = cfac * eps;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x)
        md_update_link(i, U + off, P + off, F + off, eps, do_p, coef);
}

__global__ void __launch_bounds__(256) ens_staple_force_kernel(GArgs a, const EnsPar *par, double *F) {
    const long off = (long)blockIdx.y * 2 * a.V;
    a.U += off;
    const double beta = par[blockIdx.y].beta;
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        staple_site(a, n, beta, F + off, nullptr);
}

__global__ void __launch_bounds__(256) ens_plaquette_kernel(GArgs a, const EnsPar *par, double2 *partials) {
    __shared__ double2 sh[4];
    a.U += (long)blockIdx.y * 2 * a.V;
    const double beta = par[blockIdx.y].beta;
    double2 acc = make_double2(0.0, 0.0);
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x) {
        const double2 P = plaquette_site(a, n);
        acc.x += P.x;
        acc.y += beta * (1.0 - P.x);
    }
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) ens_kinetic_kernel(long V, const double *P, double2 *partials) {
    __shared__ double2 sh[4];
    P += (long)blockIdx.y * 2 * V;
    double2 acc = make_double2(0.0, 0.0);
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < V; n += (long)gridDim.x * blockDim.x) {
        acc.x += 0.5 * P[n] * P[n];
        acc.x += 0.5 * P[n + V] * P[n + V];
    }
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// sum a conj(b) over a replica's 2V complex (include/variables.h:181-188's terms, this grid's order)
__global__ void __launch_bounds__(256) ens_dot_kernel(long n2, const double2 *a, const double2 *b,
                                                      double2 *partials) {
    __shared__ double2 sh[4];
    a += (long)blockIdx.y * n2;
    b += (long)blockIdx.y * n2;
    double2 acc = make_double2(0.0, 0.0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x)
        acc = cadd(acc, cmul(a[i], cconj(b[i])));
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// out[i] = row i's nparts partials in sum_partials_kernel's order (256 threads)
__global__ void __launch_bounds__(256) ens_sums_kernel(int nparts, const double2 *partials, double2 *out) {
    __shared__ double2 sh[4];
    const double2 s = sum_partials_block(nparts, partials + (long)blockIdx.x * nparts, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- launchers -----------------------------------------------------------------
namespace {
DrawArgs dargs(const Geometry &g, uint64_t seed) {
    DrawArgs a;
    a.seed = seed;
    a.V = g.V;
    a.Nx = g.Nx;
    a.Wt = g.Wt;
    a.t0 = g.t0;
    a.Ntg = g.Ntg;
    return a;
}
}  // namespace

int gauge_reduce_blocks(const Geometry &g) { return reduce_blocks(g.V); }

void launch_plaquette(hipStream_t s, const Geometry &g, int nshard, const double2 *U, const double2 *fU,
                      double beta, double2 *field, double2 *partials) {
    hipLaunchKernelGGL(plaquette_kernel, dim3(gauge_reduce_blocks(g)), dim3(256), 0, s, gargs(g, nshard, U, fU),
                       beta, field, partials);
}

void launch_staple_force(hipStream_t s, const Geometry &g, int nshard, const double2 *U, const double2 *fU,
                         double beta, double *F, double2 *staples) {
    hipLaunchKernelGGL(staple_force_kernel, dim3(grid_for(g.V)), dim3(256), 0, s, gargs(g, nshard, U, fU), beta,
                       F, staples);
}

void launch_md_update(hipStream_t s, const Geometry &g, double2 *U, double *P, const double *F, double eps,
                      int do_p, double coef) {
    hipLaunchKernelGGL(md_update_kernel, dim3(grid_for(2 * g.V)), dim3(256), 0, s, 2 * g.V, U, P, F, eps, do_p,
                       coef);
}

void launch_kinetic(hipStream_t s, const Geometry &g, const double *P, double2 *partials) {
    hipLaunchKernelGGL(kinetic_kernel, dim3(gauge_reduce_blocks(g)), dim3(256), 0, s, g.V, P, partials);
}

void launch_draw_momenta(hipStream_t s, const Geometry &g, uint64_t seed, double *P) {
    hipLaunchKernelGGL(draw_momenta_kernel, dim3(grid_for(g.V)), dim3(256), 0, s, dargs(g, seed), P);
}

void launch_draw_source(hipStream_t s, const Geometry &g, uint64_t seed, double2 *chi) {
    hipLaunchKernelGGL(draw_source_kernel, dim3(grid_for(g.V)), dim3(256), 0, s, dargs(g, seed), chi);
}

void launch_draw_gauge(hipStream_t s, const Geometry &g, uint64_t seed, double sigma, double2 *U) {
    hipLaunchKernelGGL(draw_gauge_kernel, dim3(grid_for(g.V)), dim3(256), 0, s, dargs(g, seed), sigma, U);
}

void launch_ens_draws(hipStream_t s, const Geometry &g, int R, const EnsPar *par, double *P, double2 *chi) {
    hipLaunchKernelGGL(ens_draws_kernel, dim3(grid_for(g.V), R), dim3(256), 0, s, dargs(g, 0), par, P, chi);
}

void launch_ens_md_update(hipStream_t s, const Geometry &g, int R, double2 *U, double *P, const double *F,
                          const EnsPar *par, int do_p, double cfac) {
    hipLaunchKernelGGL(ens_md_update_kernel, dim3(grid_for(2 * g.V), R), dim3(256), 0, s, 2 * g.V, U, P, F, par, do_p,
                       cfac);
}

void launch_ens_staple_force(hipStream_t s, const Geometry &g, int R, const double2 *U, const EnsPar *par, double *F) {
    hipLaunchKernelGGL(ens_staple_force_kernel, dim3(grid_for(g.V), R), dim3(256), 0, s, gargs(g, 1, U, nullptr), par,
                       F);
}

void launch_ens_plaquette(hipStream_t s, const Geometry &g, int R, const double2 *U, const EnsPar *par,
                          double2 *partials) {
    hipLaunchKernelGGL(ens_plaquette_kernel, dim3(gauge_reduce_blocks(g), R), dim3(256), 0, s,
                       gargs(g, 1, U, nullptr), par, partials);
}

void launch_ens_kinetic(hipStream_t s, const Geometry &g, int R, const double *P, double2 *partials) {
    hipLaunchKernelGGL(ens_kinetic_kernel, dim3(gauge_reduce_blocks(g), R), dim3(256), 0, s, g.V, P, partials);
}

void launch_ens_dot(hipStream_t s, const Geometry &g, int R, const double2 *a, const double2 *b, double2 *partials) {
    hipLaunchKernelGGL(ens_dot_kernel, dim3(gauge_reduce_blocks(g), R), dim3(256), 0, s, 2 * g.V, a, b, partials);
}

void launch_ens_sums(hipStream_t s, const Geometry &g, int nrows, const double2 *partials, double2 *out) {
    hipLaunchKernelGGL(ens_sums_kernel, dim3(nrows), dim3(256), 0, s, gauge_reduce_blocks(g), partials, out);
}

}  // namespace sm
