// sm_flow.hip -- gauge observables beyond the plaquette on gfx950: the
// topological charge sums of a field in one pass, and one stage of the Wilson
// (gradient) flow as one fused launch. Host: sm_flow.cpp.
//
//   sums     per site the plaquette U_01 (plaquette_site, sm_gauge_site.h):
//            1 - Re U_01, atan2(Im U_01, Re U_01) and Im U_01, summed with
//            plaquette_kernel's grid and block sums (fixed order, no atomics).
//            A block writes two partials: (action, angle) into row 0 and
//            (Im, 0) into row 1 of its field's pair of rows; topo_sums_kernel
//            sums a row pair in launch_sum_partials' order.
//   stage    Luescher's third-order step in its one-accumulator form,
//              stage 0: A = eps Z(W);                       W <- W exp(i A / 4)
//              stage 1: A = (8/9) eps Z(W) - (17/36) A;     W <- W exp(i A)
//              stage 2: A = (3/4) eps Z(W) - A;             W <- W exp(i A)
//            with Z_mu(n) = -Im(W_mu(n) conj(S_mu(n))) (staples_at: the gauge
//            force at beta = 1) and exp(i y) = cexp_i. One thread per SITE
//            forms both staples, updates both accumulators and rotates both
//            links: the two staples share the loads of U_0(n+x) and U_1(n+t),
//            so a site costs 10 link loads where a thread per link would cost
//            14 per site, and neighbouring threads (t fastest) read
//            neighbouring addresses in every one of them. The stencil reads
//            neighbours, so the rotated links go to ANOTHER buffer.
//            Traffic per site: 32 B of links and 16 B of accumulator read
//            (none at stage 0), 32 B of links and 16 B of accumulator written
//            (none at stage 2, whose A nobody reads): 80 / 96 / 80 B by stage,
//            256 B per step; the eight neighbour links come from L2.
//
// Replica forms: replica r = blockIdx.y, its fields r * 2V elements into each
// array; per replica the one-field kernel's site function over the one-field
// kernel's grid, so values, partials and their order are the one-field launch's.
#include "sm_device.h"
#include "sm_gauge_site.h"
#include "sm_internal.h"

namespace sm {

namespace {

// A = ca (eps Z) - cb A (stage 0: A = eps Z, A not read; stage 2: A not written), W <- W exp(i rot A)
struct FlowStage {
    double eps, ca, cb, rot;
    int stage;
};

struct TopoAcc {
    double2 a;  // (sum 1 - Re U_01, sum atan2(Im U_01, Re U_01))
    double2 b;  // (sum Im U_01, 0)
};

__device__ __forceinline__ void topo_site(const GArgs &a, long n, TopoAcc &acc) {
    const double2 P = plaquette_site(a, n);
    acc.a.x += 1.0 - P.x;
    acc.a.y += atan2(P.y, P.x);
    acc.b.x += P.y;
}

// this block's partials of the field a.U into rows[0 .. nb) and rows[nb .. 2 nb), nb = gridDim.x
__device__ __forceinline__ void topo_block(const GArgs &a, double2 *rows, double2 (*sh)[4]) {
    TopoAcc acc{make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        topo_site(a, n, acc);
    const double2 sa = block_sum(acc.a, sh[0]);
    const double2 sb = block_sum(acc.b, sh[1]);
    if (threadIdx.x == 0) {
        rows[blockIdx.x] = sa;
        rows[gridDim.x + blockIdx.x] = sb;
    }
}

__device__ __forceinline__ void flow_site(const GArgs &a, long n, const FlowStage &s, double *A, double2 *W) {
    const double2 u0 = a.U[n], u1 = a.U[n + a.V];
    double2 S0, S1;
    staples_at(a, n, u0, u1, S0, S1);
    const double ez0 = s.eps * -cmul(u0, cconj(S0)).y;
    const double ez1 = s.eps * -cmul(u1, cconj(S1)).y;
    double a0 = ez0, a1 = ez1;
    if (s.stage > 0) {
        a0 = s.ca * ez0 - s.cb * A[n];
        a1 = s.ca * ez1 - s.cb * A[n + a.V];
    }
    if (s.stage < 2) {
        A[n] = a0;
        A[n + a.V] = a1;
    }
    W[n] = cmul(u0, cexp_i(s.rot * a0));
    W[n + a.V] = cmul(u1, cexp_i(s.rot * a1));
}

// (ca, cb, rot) = (1, 0, 1/4), (8/9, 17/36, 1), (3/4, 1, 1)
FlowStage flow_stage(int stage, double eps) {
    FlowStage s;
    s.eps = eps;
    s.stage = stage;
    s.ca = stage == 1 ? 8.0 / 9.0 : stage == 2 ? 0.75 : 1.0;
    s.cb = stage == 1 ? 17.0 / 36.0 : stage == 2 ? 1.0 : 0.0;
    s.rot = stage == 0 ? 0.25 : 1.0;
    return s;
}

}  // namespace

__global__ void __launch_bounds__(256) topo_kernel(GArgs a, double2 *partials) {
    __shared__ double2 sh[2][4];
    topo_block(a, partials, sh);
}

__global__ void __launch_bounds__(256) ens_topo_kernel(GArgs a, double2 *partials) {
    __shared__ double2 sh[2][4];
    a.U += (long)blockIdx.y * 2 * a.V;
    topo_block(a, partials + (long)blockIdx.y * 2 * gridDim.x, sh);
}

// out[i * ostride + 0, 1, 2] = the three sums of row pair i (256 threads, sum_partials_kernel's order)
__global__ void __launch_bounds__(256) topo_sums_kernel(int nparts, const double2 *partials, double *out,
                                                        long ostride) {
    __shared__ double2 sh[2][4];
    const double2 *rows = partials + (long)blockIdx.x * 2 * nparts;
    const double2 sa = sum_partials_block(nparts, rows, sh[0]);
    const double2 sb = sum_partials_block(nparts, rows + nparts, sh[1]);
    if (threadIdx.x == 0) {
        double *o = out + (long)blockIdx.x * ostride;
        o[0] = sa.x;
        o[1] = sa.y;
        o[2] = sb.x;
    }
}

__global__ void __launch_bounds__(256) flow_stage_kernel(GArgs a, FlowStage s, double *A, double2 *W) {
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        flow_site(a, n, s, A, W);
}

__global__ void __launch_bounds__(256) ens_flow_stage_kernel(GArgs a, FlowStage s, double *A, double2 *W) {
    const long off = (long)blockIdx.y * 2 * a.V;
    a.U += off;
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < a.V; n += (long)gridDim.x * blockDim.x)
        flow_site(a, n, s, A + off, W + off);
}

// ---- launchers -----------------------------------------------------------------
void launch_topo(hipStream_t s, const Geometry &g, int nshard, const double2 *U, const double2 *fU,
                 double2 *partials) {
    hipLaunchKernelGGL(topo_kernel, dim3(gauge_reduce_blocks(g)), dim3(256), 0, s, gargs(g, nshard, U, fU),
                       partials);
}

void launch_ens_topo(hipStream_t s, const Geometry &g, int R, const double2 *U, double2 *partials) {
    hipLaunchKernelGGL(ens_topo_kernel, dim3(gauge_reduce_blocks(g), R), dim3(256), 0, s,
                       gargs(g, 1, U, nullptr), partials);
}

void launch_topo_sums(hipStream_t s, const Geometry &g, int nfields, const double2 *partials, double *out,
                      long ostride) {
    hipLaunchKernelGGL(topo_sums_kernel, dim3(nfields), dim3(256), 0, s, gauge_reduce_blocks(g), partials, out,
                       ostride);
}

void launch_flow_stage(hipStream_t s, const Geometry &g, int stage, double eps, const double2 *Uin, double *A,
                       double2 *Wout) {
    hipLaunchKernelGGL(flow_stage_kernel, dim3(grid_for(g.V)), dim3(256), 0, s, gargs(g, 1, Uin, nullptr),
                       flow_stage(stage, eps), A, Wout);
}

void launch_ens_flow_stage(hipStream_t s, const Geometry &g, int R, int stage, double eps, const double2 *Uin,
                           double *A, double2 *Wout) {
    hipLaunchKernelGGL(ens_flow_stage_kernel, dim3(grid_for(g.V), R), dim3(256), 0, s,
                       gargs(g, 1, Uin, nullptr), flow_stage(stage, eps), A, Wout);
}

}  // namespace sm
