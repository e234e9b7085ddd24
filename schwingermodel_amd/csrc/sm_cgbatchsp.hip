// sm_cgbatchsp.hip -- the fp32 pass of the batched multi-source CG and the
// batched helper kernels of its mixed-precision solve (gfx950; driver:
// sm_cgbatchmp.cpp). It relates to sm_cgbatch.hip as sm_eosp.hip relates to
// sm_eotd.hip.
//
// The pass is cg_batch_kernel's stored-Ad two-direction march (sm_cgbatch.hip
// has the geometry: one wave per tile, 60 owned t-columns with 2 halo lanes per
// side, DPP shifts, no LDS, no barrier, K x NWT x NCH tiles column-major, the
// tile height from cg_batch_config) on float2 fields, for the columns named in
// a 64-bit mask. Pass j of a segment of inner iterations, per column b with
// that column's own scalars, on the correction y to x:
//     r_{j-1} = d_{j-1} - beta_{j-2} d_{j-2}
//     r_j     = r_{j-1} - alpha_{j-1} Ad_{j-1}          (Ad_{j-1} stored by pass j-1)
//     d_j     = r_j + beta_{j-1} d_{j-1}                (stored)
//     y      <- (y + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}   on even j >= 2
//     Ad_j    = D D^dag d_j                             (in registers; stored)
//     partials <d_j,Ad_j>, <r_j,Ad_j>, |r_j|^2, |Ad_j|^2
// Per site and column it reads d_{j-1}, d_{j-2}, Ad_{j-1} (48 B) and writes d_j,
// Ad_j (32), plus y read and written every other pass (16 mean) and the links
// (16, from cache after the first column): 112 B against the fp64 pass's 224.
//
// A segment starts from an INJECTED direction (reliable updates, sm_cg_host.h):
// d_0 = fp32(r) + beta d_prev. Pass 0 (FIRST) rebuilds r_0 = d_0 - beta d_prev,
// keeps d_0 (no store, no y update, Ad_{-1} not read) and forms and stores Ad_0.
// Columns end their segments after different counts J_b, so the ring slot that
// holds d_{J_b - 1} differs per column: the injection copies it to the slot of
// d_{-1} and writes d_0 to slot 0 (pointwise per site, so in place is safe),
// and every pass of a round uses one rotation for all columns.
//
// Scalars: every dot partial accumulates in fp64 from the fp32 values, per
// GRANULE of G rows as in sm_cgbatch.hip, and a scalar kernel of K blocks
// after each pass sums column b's P slots in slot order (thread i takes slots
// i, i + 256, ...; then block_sum's fixed order), forms alpha and beta in fp64
// (mp_scalar_step, sm_device.h), keeps M and ends the segment on the device.
// The pass uses alpha and beta rounded to fp32. A column's bits depend on its
// own phi, U, m0, tol and max_iter only: not on K, its position, the other
// columns or the tile height. A column whose segment has ended, or that is not
// in the mask, is a block-uniform return at entry: its fields, scalars and
// partials are not touched. No kernel here waits on another block.
//
// Links: one shared float2 copy pre-scaled by sp_convert_links_kernel
// (sm_cgsp.hip): U_t by -SignR / 2, U_x by -1 / 2. The site stencil sp_site and
// the fp32 arithmetic under it are sm_device.h's, shared with sm_cgsp.hip.
#include "sm_device.h"
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

namespace {

constexpr int BW = kFusedWaveCols;  // owned t-columns per wave

struct BSPArgs {
    const float2 *d1, *d2, *aold;  // d_{j-1}, d_{j-2}, Ad_{j-1}: K columns, 2V complex apart
    float2 *dn, *anew, *y;
    const float2 *U;               // pre-scaled links, plane 0 = -SignR U_t / 2, plane 1 = -U_x / 2
    const MPScalars *sc;           // K
    double2 *partials;             // column b at + b * pstride, 2 per slot: (<d,Ad>, <r,Ad>), (|r|^2, |Ad|^2)
    unsigned long long mask;       // the columns of this round
    long pstride;
    long V;
    int Nx, Wt;
    int xchunk, G, NG, NWT, NCH;
    float mass;
};

struct RawF {
    Spf d1, d2, ad, yv;
    float2 ut, ux;
};

// FIRST: pass 0 of a segment. XP: y takes the updates of passes j-1 and j together.
template <int FIRST, int XP>
__global__ void __launch_bounds__(64) cg_batch_sp_kernel(BSPArgs a) {
    const int tiles = a.NWT * a.NCH;
    const int b = blockIdx.x / tiles;
    if (!((a.mask >> b) & 1)) return;  // block-uniform
    const MPScalars *sc = a.sc + b;
    if (sc->done) return;              // block-uniform: the column's segment ended in an earlier pass
    // FIRST: alpha = 0, and the injection's beta (kept in sc->beta) rebuilds r_0
    const float alpha = FIRST ? 0.f : (float)sc->alpha;
    const float beta = FIRST ? 0.f : (float)sc->beta;
    const float alpha2 = FIRST ? 0.f : (float)sc->alpha2;
    const float beta2 = FIRST ? (float)sc->beta : (float)sc->beta2;
    const int w = blockIdx.x - b * tiles;
    const int g = w % a.NWT, xc = w / a.NWT;
    const int lane = threadIdx.x;
    const int Nx = a.Nx, Wt = a.Wt;
    const long V = a.V, col = (long)b * 2 * V;
    const int x0 = xc * a.xchunk;
    const int xe = min(Nx, x0 + a.xchunk);
    const int c = g * BW - 2 + lane;
    const bool own = lane >= 2 && lane < BW + 2 && c < Wt;
    int cw = c % Wt;  // periodic wrap (one shard): narrower shapes than a wave or the halo wrap onto themselves
    if (cw < 0) cw += Wt;
    const float mass = a.mass;
    const float2 *S1 = a.d1 + col + cw, *S2 = a.d2 + col + cw, *Sa = a.aold + col + cw, *Su = a.U + cw;
    float2 *yb = a.y + col, *dn_ = a.dn + col, *an_ = a.anew + col;
    auto wrap = [Nx](int x) { int q = x % Nx; return q < 0 ? q + Nx : q; };
    // d_{j-1}, d_{j-2}, Ad_{j-1}: rows x0-2 .. xe+1; U: x0-2 .. xe; y: owned rows
    auto load = [&](int xr, RawF &R) {
        const long pr = (long)wrap(xr) * Wt;
        R.d1 = Spf{S1[pr], S1[pr + V]};
        R.d2 = Spf{S2[pr], S2[pr + V]};
        if (!FIRST) R.ad = Spf{Sa[pr], Sa[pr + V]};
        const long pu = (long)wrap(min(xr, xe)) * Wt;
        R.ut = Su[pu];
        R.ux = Su[pu + V];
        if (XP) {
            const long ny = (long)wrap(min(max(xr, x0), xe - 1)) * Wt + cw;
            R.yv = Spf{yb[ny], yb[ny + V]};
        }
    };
    // r_j and d_j of row xr; on owned rows store d_j and y_j
    auto form = [&](int xr, const RawF &R, Spf &rj) {
        rj.a = axpyf(-beta2, R.d2.a, R.d1.a);  // r_{j-1} (FIRST: r_0 of the injected direction)
        rj.b = axpyf(-beta2, R.d2.b, R.d1.b);
        Spf d = R.d1;                          // FIRST: d_0 kept
        if (!FIRST) {
            rj.a = axpyf(-alpha, R.ad.a, rj.a);
            rj.b = axpyf(-alpha, R.ad.b, rj.b);
            d.a = axpyf(beta, R.d1.a, rj.a);
            d.b = axpyf(beta, R.d1.b, rj.b);
        }
        if (xr >= x0 && xr < xe && own) {
            const long n = (long)xr * Wt + c;
            if (!FIRST) {
                dn_[n] = d.a;
                dn_[n + V] = d.b;
            }
            if (XP) {  // y_j = (y_{j-2} + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}
                yb[n] = axpyf(alpha, R.d1.a, axpyf(alpha2, R.d2.a, R.yv.a));
                yb[n + V] = axpyf(alpha, R.d1.b, axpyf(alpha2, R.d2.b, R.yv.b));
            }
        }
        return d;
    };
    double acc_dA = 0.0, acc_rA = 0.0, acc_rr = 0.0, acc_AA = 0.0;  // of the running granule
    double2 *part = a.partials + (long)b * a.pstride + 2 * (long)g * a.NG;
    const float2 z = f2(0.f, 0.f);
    RawF R;
    R.ad = Spf{z, z};
    R.yv = Spf{z, z};
    Spf rj;
    load(x0 - 2, R);
    const Spf dm2 = form(x0 - 2, R, rj);
    const float2 uxm2 = R.ux;
    load(x0 - 1, R);
    const Spf dm1 = form(x0 - 1, R, rj);
    const float2 utm1 = R.ut, uxm1 = R.ux;
    load(x0, R);
    Spf rc;
    Spf dc = form(x0, R, rc);
    float2 utc = R.ut, uxc = R.ux;
    load(x0 + 1, R);
    Spf rn;
    Spf dn = form(x0 + 1, R, rn);
    float2 utn = R.ut, uxn = R.ux;
    load(x0 + 2, R);
    Spf Tp = sp_site<1>(mass, dm1, dm2, dc, utm1, uxm1, uxm2);  // D^dag d_j at rows x-1, x
    Spf Tc = sp_site<1>(mass, dc, dm1, dn, utc, uxc, uxm1);
    float2 uxp = uxm1;  // U_x at row x-1
    for (int x = x0; x < xe; ++x) {
        Spf r2;
        const Spf d2 = form(x + 2, R, r2);
        const float2 ut2 = R.ut, ux2 = R.ux;
        load(min(x + 3, xe + 1), R);
        __builtin_amdgcn_sched_barrier(0);  // keep the next row's loads issued here
        const Spf Tn = sp_site<1>(mass, dn, dc, d2, utn, uxn, uxc);
        const Spf o = sp_site<0>(mass, Tc, Tp, Tn, utc, uxc, uxp);
        if (own) {
            const long n = (long)x * Wt + c;
            an_[n] = o.a;
            an_[n + V] = o.b;
            acc_dA = dacc(acc_dA, dc.a, o.a);
            acc_dA = dacc(acc_dA, dc.b, o.b);
            acc_rA = dacc(acc_rA, rc.a, o.a);
            acc_rA = dacc(acc_rA, rc.b, o.b);
            acc_rr = dacc(acc_rr, rc.a, rc.a);
            acc_rr = dacc(acc_rr, rc.b, rc.b);
            acc_AA = dacc(acc_AA, o.a, o.a);
            acc_AA = dacc(acc_AA, o.b, o.b);
        }
        if ((x + 1) % a.G == 0 || x == xe - 1) {  // the granule x / G is complete (x0 is a multiple of G)
            const double2 s0 = wave_sum(make_double2(acc_dA, acc_rA)), s1 = wave_sum(make_double2(acc_rr, acc_AA));
            if (lane == 0) {
                double2 *p = part + 2 * (long)(x / a.G);
                p[0] = s0;
                p[1] = s1;
            }
            acc_dA = acc_rA = acc_rr = acc_AA = 0.0;
        }
        Tp = Tc;
        Tc = Tn;
        dc = dn;
        dn = d2;
        rc = rn;
        rn = r2;
        uxp = uxc;
        utc = utn;
        uxc = uxn;
        utn = ut2;
        uxn = ux2;
    }
}

// The scalar step after pass j of a round (first: j == 0): block b sums column
// b's P slots in slot order and evaluates mp_scalar_step.
__global__ void __launch_bounds__(256) cg_batch_sp_scalar_kernel(int P, const double2 *partials, long pstride,
                                                                 MPScalars *sc, int first, unsigned long long mask) {
    __shared__ double2 sh[4];
    if (!((mask >> blockIdx.x) & 1)) return;
    sc += blockIdx.x;
    if (sc->done) return;  // block-uniform; thread 0 writes it only after the last barrier
    const double2 *part = partials + blockIdx.x * pstride;
    double2 a0 = make_double2(0.0, 0.0), a1 = a0;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        a0 = cadd(a0, part[2 * (long)i]);
        a1 = cadd(a1, part[2 * (long)i + 1]);
    }
    const double2 s0 = block_sum(a0, sh);
    __syncthreads();
    const double2 s1 = block_sum(a1, sh);
    if (threadIdx.x == 0) mp_scalar_step(sc, first, s0.x, s0.y, s1.x, s1.y);
}

// grid K x NBR: block q of column b takes entries q*256 + tid, + NBR*256, ... of 2V
// r = phi - Ax (fp64), per block (|r|^2, |phi|^2)
__global__ void __launch_bounds__(256) batch_mp_residual_kernel(int NBR, long n, const double2 *phi, const double2 *Ax,
                                                                double2 *r, double2 *part, unsigned long long mask) {
    __shared__ double2 sh[4];
    const int b = blockIdx.x / NBR, q = blockIdx.x - b * NBR;
    if (!((mask >> b) & 1)) return;
    const long col = (long)b * n;
    double2 acc = make_double2(0.0, 0.0);
    for (long i = (long)q * 256 + threadIdx.x; i < n; i += (long)NBR * 256) {
        const double2 p = phi[col + i];
        const double2 ri = csub(p, Ax[col + i]);
        r[col + i] = ri;
        acc.x = nacc<2>(acc.x, ri);
        acc.y = nacc<2>(acc.y, p);
    }
    const double2 s = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(long)b * NBR + q] = s;
}

// block b: column b's partials in order, then launch_mp_update's step on its scalars
__global__ void __launch_bounds__(256) batch_mp_update_kernel(int NBR, const double2 *part, MPScalars *sc, int init,
                                                              int restart, double tol, double delta, int max_iter,
                                                              unsigned long long mask) {
    __shared__ double2 sh[4];
    if (!((mask >> blockIdx.x) & 1)) return;
    const double2 s = sum_partials_block(NBR, part + (long)blockIdx.x * NBR, sh);
    if (threadIdx.x == 0) mp_update_step(sc + blockIdx.x, s, init, restart, tol, delta, max_iter);
}

// d_0 = fp32(r) + beta_b d_prev into ring slot 0 and d_prev into slot 2 (the
// slot of d_{-1}); d_prev = the ended segment's d_{k_last - 1}, in slot
// (k_last - 1) mod 3. beta == 0 (the first segment, or a restart): d_prev is
// not read but written, d_prev = d_0. Pointwise per site: in place is safe.
__global__ void __launch_bounds__(256) batch_mp_inject_kernel(int NBR, long n, const double2 *r, float2 *s0, float2 *s1,
                                                              float2 *s2, const MPScalars *sc, unsigned long long mask) {
    const int b = blockIdx.x / NBR, q = blockIdx.x - b * NBR;
    if (!((mask >> b) & 1)) return;
    sc += b;
    const float beta = (float)sc->beta;
    const bool fresh = sc->beta == 0.0;
    const int i3 = fresh ? 0 : (sc->k_last - 1) % 3;
    const long col = (long)b * n;
    const float2 *dlast = (i3 == 0 ? s0 : (i3 == 1 ? s1 : s2)) + col;
    for (long i = (long)q * 256 + threadIdx.x; i < n; i += (long)NBR * 256) {
        const double2 ri = r[col + i];
        float2 v = make_float2((float)ri.x, (float)ri.y);
        float2 p = v;
        if (!fresh) {
            p = dlast[i];
            v = axpyf(beta, p, v);
        }
        s2[col + i] = p;
        s0[col + i] = v;
    }
}

// x += y (fp64 += fp32), plus alpha_{J-1} d_{J-1} when the column's last pass
// J = sc->k is odd (y holds the steps up to the last even pass), y = 0; d_{J-1}
// is in ring slot (J - 1) mod 3. discard bit: y = 0 only.
__global__ void __launch_bounds__(256) batch_mp_fold_kernel(int NBR, long n, double2 *x, float2 *y, const float2 *s0,
                                                            const float2 *s1, const float2 *s2, const MPScalars *sc,
                                                            unsigned long long mask, unsigned long long discard) {
    const int b = blockIdx.x / NBR, q = blockIdx.x - b * NBR;
    if (!((mask >> b) & 1)) return;
    sc += b;
    const int k = sc->k;
    const double alpha = sc->alpha;
    const bool pending = (k & 1) != 0;
    const bool drop = (discard >> b) & 1;
    const int i3 = k >= 1 ? (k - 1) % 3 : 0;
    const long col = (long)b * n;
    const float2 *dlast = (i3 == 0 ? s0 : (i3 == 1 ? s1 : s2)) + col;
    for (long i = (long)q * 256 + threadIdx.x; i < n; i += (long)NBR * 256) {
        if (!drop) {
            const float2 yv = y[col + i];
            double2 add = make_double2((double)yv.x, (double)yv.y);
            if (pending) {
                const float2 d = dlast[i];
                add.x = __builtin_fma(alpha, (double)d.x, add.x);
                add.y = __builtin_fma(alpha, (double)d.y, add.y);
            }
            const double2 xv = x[col + i];
            x[col + i] = make_double2(xv.x + add.x, xv.y + add.y);
        }
        y[col + i] = make_float2(0.f, 0.f);
    }
}

}  // namespace

int batch_mp_blocks(const Geometry &g) {
    const long nb = (2 * g.V + 255) / 256;
    return (int)(nb < 256 ? nb : 256);
}

void launch_cg_batch_sp(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, unsigned long long mask,
                        float2 *const d[3], float2 *const ad[2], float2 *y, const float2 *U32, double mass, long pass,
                        MPScalars *sc, double2 *partials) {
    auto dbuf = [&](long i) { return d[((i % 3) + 3) % 3]; };
    BSPArgs a;
    // passes 0 and 1 both read d_0 and d_{-1}; pass 0 stores no d
    a.d1 = pass == 0 ? dbuf(0) : dbuf(pass - 1);
    a.d2 = pass == 0 ? dbuf(-1) : dbuf(pass - 2);
    a.dn = dbuf(pass);
    a.aold = ad[(pass + 1) & 1];
    a.anew = ad[pass & 1];
    a.y = y; a.U = U32; a.sc = sc; a.partials = partials; a.mask = mask;
    a.pstride = 2L * c.P;
    a.V = g.V; a.Nx = g.Nx; a.Wt = g.Wt;
    a.xchunk = c.xchunk; a.G = c.G; a.NG = c.NG; a.NWT = c.NWT; a.NCH = c.NCH;
    a.mass = (float)mass;
    const dim3 grid((unsigned)(K * c.NWT * c.NCH)), block(64);
    if (pass == 0) hipLaunchKernelGGL((cg_batch_sp_kernel<1, 0>), grid, block, 0, s, a);
    else if (pass >= 2 && (pass & 1) == 0) hipLaunchKernelGGL((cg_batch_sp_kernel<0, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((cg_batch_sp_kernel<0, 0>), grid, block, 0, s, a);
    hipLaunchKernelGGL(cg_batch_sp_scalar_kernel, dim3(K), dim3(256), 0, s, c.P, partials, a.pstride, sc,
                       pass == 0 ? 1 : 0, mask);
}

void launch_batch_mp_residual(hipStream_t s, const Geometry &g, int K, unsigned long long mask, const double2 *phi,
                              const double2 *Ax, double2 *r, double2 *partials, MPScalars *sc, int init, int restart,
                              double tol, double delta, int max_iter) {
    const int NBR = batch_mp_blocks(g);
    hipLaunchKernelGGL(batch_mp_residual_kernel, dim3(K * NBR), dim3(256), 0, s, NBR, 2 * g.V, phi, Ax, r, partials,
                       mask);
    hipLaunchKernelGGL(batch_mp_update_kernel, dim3(K), dim3(256), 0, s, NBR, partials, sc, init, restart, tol, delta,
                       max_iter, mask);
}

void launch_batch_mp_inject(hipStream_t s, const Geometry &g, int K, unsigned long long mask, const double2 *r,
                            float2 *const d[3], const MPScalars *sc) {
    const int NBR = batch_mp_blocks(g);
    hipLaunchKernelGGL(batch_mp_inject_kernel, dim3(K * NBR), dim3(256), 0, s, NBR, 2 * g.V, r, d[0], d[1], d[2], sc,
                       mask);
}

void launch_batch_mp_fold(hipStream_t s, const Geometry &g, int K, unsigned long long mask, unsigned long long discard,
                          double2 *x, float2 *y, float2 *const d[3], const MPScalars *sc) {
    const int NBR = batch_mp_blocks(g);
    hipLaunchKernelGGL(batch_mp_fold_kernel, dim3(K * NBR), dim3(256), 0, s, NBR, 2 * g.V, x, y, d[0], d[1], d[2], sc,
                       mask, discard);
}

}  // namespace sm
