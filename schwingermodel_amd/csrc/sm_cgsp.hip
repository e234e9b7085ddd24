// sm_cgsp.hip -- fp32 two-direction CG pass that recomputes Ad_{j-1}, and the
// helper kernels of the mixed-precision solve (gfx950; driver: sm_cgmp.cpp).
//
// The pass is sm_cgra.hip's S1-S5 march (see its header) on float2 fields,
// one-shard contexts only: no link codes, no t-shard faces, no peer stores,
// no strip variant, forward marches, a separate scalar kernel. Pass j of a
// segment of inner iterations:
//     r_{j-1} = d_{j-1} - beta_{j-2} d_{j-2}
//     r_j     = r_{j-1} - alpha_{j-1} Ad_{j-1}          (Ad_{j-1} recomputed)
//     d_j     = r_j + beta_{j-1} d_{j-1}                (stored)
//     y      <- (y + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}   on the rows of parity j & 1
//     Ad_j    = D D^dag d_j ; partials <d_j,Ad_j>, <r_j,Ad_j>, |r_j|^2, |Ad_j|^2
// It reads d_{j-1}, d_{j-2} and the links (16 B/site each) and writes d_j (16),
// plus y on half the rows (16 on average): 80 B/site against the fp64 pass's
// 145-160.
//
// A segment starts from an INJECTED direction (reliable updates, sm_cgmp.cpp):
// d_0 = r + beta d_prev with r the fp64 true residual rounded to fp32, so
// r_0 != d_0. Pass 0 (FIRST) rebuilds r_0 = d_0 - beta d_prev like any other
// pass rebuilds r_{j-1}, keeps d_0 (no store, no y update) and forms Ad_0 and
// the dots; pass 1 reads the same two buffers again. The very first segment
// has beta = 0 and d_prev = d_0.
//
// Scalars: the hermitian positive operator makes alpha and beta real; every
// dot partial is accumulated in fp64 (the fp32 products are exact in fp64),
// the tiles' partials are summed in a fixed order by the scalar kernel, which
// forms alpha and beta in fp64; the pass uses them rounded to fp32. The scalar
// kernel also keeps M, the largest iterated |r| since the segment began, and
// ends the segment on the device (|r| < delta M, |r| < tol |phi|, the
// iteration limit, or a non-finite scalar): later passes return at once, so
// the host reads the state in chunks, not every iteration.
//
// The links arrive pre-scaled (sp_convert_links_kernel): U_t by -SignR/2 and
// U_x by -1/2, the form sm_cgra.hip's FOLD = 2 stencil takes; powers of two
// and signs commute with the rounding to fp32.
//
// One float2 per lane (an 8-byte access, inside the 8-16 B coalescing range);
// a two-column-per-lane form was not built. The fp32 arithmetic (Spf, the DPP
// float shifts, the float2 helpers, dacc, sp_site) is sm_device.h's, shared
// with sm_eosp.hip and sm_cgbatchsp.hip.
#include <type_traits>

#include "sm_device.h"
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

namespace {

constexpr int SW = kRAWaveCols;  // owned t-columns per wave
constexpr int SH4 = 4;           // halo lanes per side

struct SPArgs {
    const float2 *d1, *d2;  // d_{j-1}, d_{j-2}
    float2 *dn;             // d_j
    float2 *y;
    const float2 *U;        // pre-scaled links, plane 0 = -SignR U_t / 2, plane 1 = -U_x / 2
    const MPScalars *sc;
    double2 *partials;      // 2 per tile: (<d,Ad>, <r,Ad>), (|r|^2, |Ad|^2)
    long V;
    int Nx, Wt;
    int xchunk, NWT, TBk, XB, remap, wpb, xbal;
    int xpar;               // this pass updates y on the rows of parity xpar
    float mass;
};

// The row march of one tile: the wave owns columns [cbase, cbase + SW), its
// lanes cover cbase - 4 + lane, periodic in t (modulo Wt: shapes narrower than
// a wave or than the halo wrap onto themselves) and in x.
template <int FIRST>
__device__ __forceinline__ void sp_march(const SPArgs &a, int cbase, int lane, int x0, int xe, float alpha, float beta,
                                         float alpha2, float beta2, double &acc_dA, double &acc_rA, double &acc_rr,
                                         double &acc_AA) {
    const int Nx = a.Nx, Wt = a.Wt;
    const long V = a.V;
    const int c = cbase - SH4 + lane;
    const bool own = lane >= SH4 && lane < SW + SH4 && c < Wt;
    int cw = c % Wt;
    if (cw < 0) cw += Wt;
    const float mass = a.mass;
    const float2 *S1 = a.d1 + cw, *S2 = a.d2 + cw, *SU = a.U + cw;
    // y is read and written by the owned lanes only: the halo lanes load their
    // wave's nearest owned column
    const int co = min(max(c, cbase), cbase + SW - 1);
    const int cx = co >= Wt ? Wt - 1 : co;
    auto wrap = [Nx](int x) { int w = x % Nx; return w < 0 ? w + Nx : w; };
    // d_{j-1}: rows x0-4 .. xe+3; U: x0-4 .. xe+2; d_{j-2}: x0-2 .. xe+1; y: owned rows
    auto ld1 = [&](int xr, Spf &d) {
        const float2 *p = S1 + (long)wrap(min(xr, xe + 3)) * Wt;
        d.a = p[0];
        d.b = p[V];
    };
    auto ldu = [&](int xr, float2 &ut, float2 &ux) {
        const float2 *p = SU + (long)wrap(min(xr, xe + 2)) * Wt;
        ut = p[0];
        ux = p[V];
    };
    auto ld2 = [&](int xr, Spf &q, Spf &yv) {
        const float2 *p = S2 + (long)wrap(min(max(xr, x0 - 2), xe + 1)) * Wt;
        q.a = p[0];
        q.b = p[V];
        if (!FIRST && (xr & 1) == a.xpar) {  // wave-uniform: only the rows this pass updates
            const long n = (long)wrap(min(max(xr, x0), xe - 1)) * Wt + cx;
            yv.a = a.y[n];
            yv.b = a.y[n + V];
        }
    };
    const float2 z = f2(0.f, 0.f);
    const Spf zs = Spf{z, z};
    // state at the top of iteration y (sm_cgra.hip's header)
    Spf D2, D3, Ld;                                                 // d_{j-1}(y+2), (y+3); in flight (y+4)
    float2 Lut, Lux;                                                // in flight U(y+3)
    Spf Mq, My = zs;                                                // in flight d_{j-2}(y+2), y(y+2)
    float2 Ut0 = z, Ut1 = z, Ut2, Ux0 = z, Ux1 = z, Ux2, Uxm = z;   // U_t(y..y+2), U_x(y-1..y+2)
    Spf P1 = zs, P2 = zs;                                           // T'(y+1), T'(y+2)
    Spf J0 = zs, J1 = zs;                                           // d_j at rows y, y+1
    Spf Q0 = zs, Q1 = zs;                                           // T(y-1), T(y)
    Spf R0 = zs, R1 = zs;                                           // r_j at rows y, y+1 (waits for Ad_j)
    const int y0 = x0 - 6;
    ld1(y0 + 2, D2);
    ld1(y0 + 3, D3);
    ldu(y0 + 2, Ut2, Ux2);
    ld1(y0 + 4, Ld);
    ldu(y0 + 3, Lut, Lux);
    ld2(y0 + 2, Mq, My);
    // stage mask M: bit 0 = S2 + S3, bit 1 = S4, bit 2 = S5 (S1 always)
    auto step = [&](int y, auto mtag) {
        constexpr int M = decltype(mtag)::value;
        const Spf D4 = Ld;
        const float2 Ut3 = Lut, Ux3 = Lux;
        ld1(y + 5, Ld);
        ldu(y + 4, Lut, Lux);
        __builtin_amdgcn_sched_barrier(0);  // keep the next rows' loads issued here
        Spf P3 = zs;
        if (!FIRST) P3 = sp_site<1>(mass, D3, D2, D4, Ut3, Ux3, Ux2);  // S1: T'(y+3)
        Spf J2 = zs, Q2 = zs, R2 = zs;
        if constexpr ((M & 1) != 0) {
            // S3: r_j, d_j at row y+2
            const int xr = y + 2;
            const Spf Q = Mq, Y = My;
            Spf rp;
            rp.a = axpyf(-beta2, Q.a, D2.a);
            rp.b = axpyf(-beta2, Q.b, D2.b);
            if (FIRST) {  // the injected direction: r_0 rebuilt, d_0 kept
                R2 = rp;
                J2 = D2;
            } else {
                const Spf A = sp_site<0>(mass, P2, P1, P3, Ut2, Ux2, Ux1);  // S2: Ad_{j-1}(y+2)
                R2.a = axpyf(-alpha, A.a, rp.a);
                R2.b = axpyf(-alpha, A.b, rp.b);
                J2.a = axpyf(beta, D2.a, R2.a);
                J2.b = axpyf(beta, D2.b, R2.b);
            }
            if (xr >= x0 && xr < xe && own) {
                const long n = (long)xr * Wt + c;
                if (!FIRST) {
                    a.dn[n] = J2.a;
                    a.dn[n + V] = J2.b;
                    if ((xr & 1) == a.xpar) {  // y_j = (y_{j-2} + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}
                        a.y[n] = axpyf(alpha, D2.a, axpyf(alpha2, Q.a, Y.a));
                        a.y[n + V] = axpyf(alpha, D2.b, axpyf(alpha2, Q.b, Y.b));
                    }
                }
                acc_rr = dacc(acc_rr, R2.a, R2.a);
                acc_rr = dacc(acc_rr, R2.b, R2.b);
            }
        }
        ld2(y + 3, Mq, My);  // consumed above: issued now, used next iteration
        if constexpr ((M & 2) != 0) Q2 = sp_site<1>(mass, J1, J0, J2, Ut1, Ux1, Ux0);  // S4: T(y+1)
        if constexpr ((M & 4) != 0) {
            const Spf o = sp_site<0>(mass, Q1, Q0, Q2, Ut0, Ux0, Uxm);  // S5: Ad_j(y)
            if (own) {
                acc_dA = dacc(acc_dA, J0.a, o.a);
                acc_dA = dacc(acc_dA, J0.b, o.b);
                acc_rA = dacc(acc_rA, R0.a, o.a);
                acc_rA = dacc(acc_rA, R0.b, o.b);
                acc_AA = dacc(acc_AA, o.a, o.a);
                acc_AA = dacc(acc_AA, o.b, o.b);
            }
        }
        D2 = D3;
        D3 = D4;
        Uxm = Ux0;
        Ut0 = Ut1;
        Ux0 = Ux1;
        Ut1 = Ut2;
        Ux1 = Ux2;
        Ut2 = Ut3;
        Ux2 = Ux3;
        P1 = P2;
        P2 = P3;
        J0 = J1;
        J1 = J2;
        Q0 = Q1;
        Q1 = Q2;
        R0 = R1;
        R1 = R2;
    };
    int y = y0;
    for (; y < x0 - 4; ++y) step(y, std::integral_constant<int, 0>());
    for (; y < x0 - 2; ++y) step(y, std::integral_constant<int, 1>());
    for (; y < x0; ++y) step(y, std::integral_constant<int, 3>());
    for (; y + 2 < xe; y += 3) {  // period-3 rotations become register renaming
        step(y, std::integral_constant<int, 7>());
        step(y + 1, std::integral_constant<int, 7>());
        step(y + 2, std::integral_constant<int, 7>());
    }
    for (; y < xe; ++y) step(y, std::integral_constant<int, 7>());
}

template <int FIRST>
__global__ void __launch_bounds__(256) cg_sp_kernel(SPArgs a) {
    __shared__ double2 sh[4];
    const MPScalars *sc = a.sc;
    if (sc->done) return;  // grid-uniform: the segment ended in an earlier pass
    // FIRST: alpha = 0, and the injection's beta (kept in sc->beta) rebuilds r_0
    const float alpha = FIRST ? 0.f : (float)sc->alpha;
    const float beta = FIRST ? 0.f : (float)sc->beta;
    const float alpha2 = FIRST ? 0.f : (float)sc->alpha2;
    const float beta2 = FIRST ? (float)sc->beta : (float)sc->beta2;
    int w = blockIdx.x;
    const int n = a.TBk * a.XB;
    if (a.remap) {  // each XCD takes a contiguous range of tiles (sm_cgra.hip)
        const int q = n >> 3, rr = n & 7, xcd = w & 7;
        w = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (w >> 3);
    }
    const int tb = w % a.TBk, xc = w / a.TBk;
    const int lane = threadIdx.x & 63;
    const int g = tb * a.wpb + (threadIdx.x >> 6);
    const int x0 = a.xbal ? (int)((long)xc * a.Nx / a.XB) : xc * a.xchunk;
    const int xe = a.xbal ? (int)((long)(xc + 1) * a.Nx / a.XB) : min(a.Nx, x0 + a.xchunk);
    double acc_dA = 0.0, acc_rA = 0.0, acc_rr = 0.0, acc_AA = 0.0;
    if (g < a.NWT && x0 < xe) sp_march<FIRST>(a, g * SW, lane, x0, xe, alpha, beta, alpha2, beta2, acc_dA, acc_rA, acc_rr, acc_AA);
    const double2 s0 = block_sum(make_double2(acc_dA, acc_rA), sh);
    __syncthreads();
    const double2 s1 = block_sum(make_double2(acc_rr, acc_AA), sh);
    if (threadIdx.x == 0) {
        double2 *p = a.partials + 2 * ((long)tb * a.XB + xc);
        p[0] = s0;
        p[1] = s1;
    }
}

// The scalar step after pass j of a segment (first: j == 0): the stop tests on
// the direct |r_j|^2, then alpha_j and beta_j (sm_device.h cg1_eval, real).
__global__ void __launch_bounds__(256) cg_sp_scalar_kernel(int ntiles, const double2 *part, MPScalars *sc, int first) {
    __shared__ double2 sh[4];
    double2 a0 = make_double2(0.0, 0.0), a1 = a0;
    for (int i = threadIdx.x; i < ntiles; i += blockDim.x) {
        a0 = cadd(a0, part[2 * i]);
        a1 = cadd(a1, part[2 * i + 1]);
    }
    const double2 s0 = block_sum(a0, sh);
    __syncthreads();
    const double2 s1 = block_sum(a1, sh);
    if (threadIdx.x != 0 || sc->done) return;
    mp_scalar_step(sc, first, s0.x, s0.y, s1.x, s1.y);
}

// Links for the fp32 pass: plane 0 = -SignR U_t / 2 (SignR = -1 at t = Nt - 1),
// plane 1 = -U_x / 2, rounded to fp32.
__global__ void __launch_bounds__(256) sp_convert_links_kernel(long V, int Wt, const double2 *U, float2 *U32) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (long)gridDim.x * blockDim.x) {
        const double kt = (int)(i % Wt) == Wt - 1 ? 0.5 : -0.5;
        const double2 ut = U[i], ux = U[i + V];
        U32[i] = make_float2((float)(kt * ut.x), (float)(kt * ut.y));
        U32[i + V] = make_float2((float)(-0.5 * ux.x), (float)(-0.5 * ux.y));
    }
}

// r = phi - Ax (fp64), per block (|r|^2, |phi|^2)
__global__ void __launch_bounds__(256) mp_residual_kernel(long n, const double2 *phi, const double2 *Ax, double2 *r,
                                                          double2 *part) {
    __shared__ double2 sh[4];
    double2 acc = make_double2(0.0, 0.0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double2 p = phi[i];
        const double2 ri = csub(p, Ax[i]);
        r[i] = ri;
        acc.x = nacc<2>(acc.x, ri);
        acc.y = nacc<2>(acc.y, p);
    }
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The true residual's norm into sc and the next segment's start: M = |r|,
// beta = |r|^2 / (the previous iterated |r|^2) for the injection (restart: 0),
// done = 1 when the true residual passes the stop test or no iteration is left.
__global__ void __launch_bounds__(256) mp_update_kernel(int nparts, const double2 *part, MPScalars *sc, int init,
                                                        int restart, double tol, double delta, int max_iter) {
    __shared__ double2 sh[4];
    const double2 s = sum_partials_block(nparts, part, sh);
    if (threadIdx.x != 0) return;
    mp_update_step(sc, s, init, restart, tol, delta, max_iter);
}

// d_0 = r + beta d_prev in fp32 (beta from mp_update_kernel). beta == 0 (the
// first segment, or a restart): d_prev is not read but written, d_prev = d_0,
// so the passes' zero-weighted reads of it find finite values.
__global__ void __launch_bounds__(256) mp_inject_kernel(long n, const double2 *r, float2 *dprev, float2 *d0,
                                                        const MPScalars *sc) {
    const float beta = (float)sc->beta;
    const bool fresh = sc->beta == 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double2 ri = r[i];
        float2 v = make_float2((float)ri.x, (float)ri.y);
        if (fresh) {
            dprev[i] = v;
        } else {
            v = axpyf(beta, dprev[i], v);
        }
        d0[i] = v;
    }
}

// x += y (fp64 += fp32) with the rows still pending folded in, y = 0: after the
// segment's last pass J = sc->k the rows of parity != (J & 1) lack
// alpha_{J-1} d_{J-1} (sm_cgra.hip cg_ra_finish_x_kernel). discard: y = 0 only.
__global__ void __launch_bounds__(256) mp_fold_kernel(long V, int Wt, double2 *x, float2 *y, const float2 *dlast,
                                                      const MPScalars *sc, int discard) {
    const int k = sc->k;
    const double alpha = k >= 1 ? sc->alpha : 0.0;
    const int par = k & 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * V; i += (long)gridDim.x * blockDim.x) {
        if (!discard) {
            const long site = i < V ? i : i - V;
            const float2 yv = y[i];
            double2 add = make_double2((double)yv.x, (double)yv.y);
            if (k >= 1 && (int)((site / Wt) & 1) != par) {
                const float2 d = dlast[i];
                add.x = __builtin_fma(alpha, (double)d.x, add.x);
                add.y = __builtin_fma(alpha, (double)d.y, add.y);
            }
            const double2 xv = x[i];
            x[i] = make_double2(xv.x + add.x, xv.y + add.y);
        }
        y[i] = make_float2(0.f, 0.f);
    }
}

__global__ void __launch_bounds__(256) mp_add_kernel(long n, double2 *x, const double2 *e) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        x[i] = cadd(x[i], e[i]);
}

__global__ void __launch_bounds__(256) mp_zero_kernel(long n, float2 *y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = make_float2(0.f, 0.f);
}

}  // namespace

CGFusedCfg cg_sp_config(const Geometry &g, const CGFusedCfg &ra) {
    CGFusedCfg c = ra;  // the fp64 pass's tile shape (rows per tile, waves per block), without its t-strips
    c.NWT = (g.Wt + SW - 1) / SW;
    cg_ra_set_strip(c, g, 0);
    c.XB = c.xbal ? c.XB : (g.Nx + c.xchunk - 1) / c.xchunk;
    return c;
}

void launch_cg_sp(hipStream_t s, const Geometry &g, const CGFusedCfg &c, const float2 *d1, const float2 *d2, float2 *dn,
                  float2 *y, const float2 *U32, double mass, long pass, MPScalars *sc, double2 *partials) {
    SPArgs a;
    a.d1 = d1; a.d2 = d2; a.dn = dn; a.y = y; a.U = U32;
    a.sc = sc; a.partials = partials;
    a.V = g.V; a.Nx = g.Nx; a.Wt = g.Wt;
    a.xchunk = c.xchunk; a.NWT = c.NWT; a.TBk = c.TBk; a.XB = c.XB; a.remap = c.remap; a.wpb = c.wpb; a.xbal = c.xbal;
    a.xpar = (int)(pass & 1);
    a.mass = (float)mass;
    const dim3 grid(c.TBk * c.XB), block(64 * c.wpb);
    if (pass == 0) hipLaunchKernelGGL(cg_sp_kernel<1>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(cg_sp_kernel<0>, grid, block, 0, s, a);
}

void launch_cg_sp_scalars(hipStream_t s, int ntiles, const double2 *partials, MPScalars *sc, int first) {
    hipLaunchKernelGGL(cg_sp_scalar_kernel, dim3(1), dim3(256), 0, s, ntiles, partials, sc, first);
}

void launch_sp_convert_links(hipStream_t s, const Geometry &g, const double2 *U, float2 *U32) {
    hipLaunchKernelGGL(sp_convert_links_kernel, dim3(reduce_blocks(g.V)), dim3(256), 0, s, g.V, g.Wt, U, U32);
}

int launch_mp_residual(hipStream_t s, long n, const double2 *phi, const double2 *Ax, double2 *r, double2 *partials) {
    const int nb = reduce_blocks(n);
    hipLaunchKernelGGL(mp_residual_kernel, dim3(nb), dim3(256), 0, s, n, phi, Ax, r, partials);
    return nb;
}

void launch_mp_update(hipStream_t s, int nparts, const double2 *partials, MPScalars *sc, int init, int restart,
                      double tol, double delta, int max_iter) {
    hipLaunchKernelGGL(mp_update_kernel, dim3(1), dim3(256), 0, s, nparts, partials, sc, init, restart, tol, delta,
                       max_iter);
}

void launch_mp_inject(hipStream_t s, long n, const double2 *r, float2 *dprev, float2 *d0, const MPScalars *sc) {
    hipLaunchKernelGGL(mp_inject_kernel, dim3(reduce_blocks(n)), dim3(256), 0, s, n, r, dprev, d0, sc);
}

void launch_mp_fold(hipStream_t s, const Geometry &g, double2 *x, float2 *y, const float2 *dlast, const MPScalars *sc,
                    int discard) {
    hipLaunchKernelGGL(mp_fold_kernel, dim3(reduce_blocks(2 * g.V)), dim3(256), 0, s, g.V, g.Wt, x, y, dlast, sc,
                       discard);
}

void launch_mp_add(hipStream_t s, long n, double2 *x, const double2 *e) {
    hipLaunchKernelGGL(mp_add_kernel, dim3(reduce_blocks(n)), dim3(256), 0, s, n, x, e);
}

void launch_mp_zero(hipStream_t s, long n, float2 *y) {
    hipLaunchKernelGGL(mp_zero_kernel, dim3(reduce_blocks(n)), dim3(256), 0, s, n, y);
}

}  // namespace sm
