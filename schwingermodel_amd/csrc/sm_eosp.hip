// sm_eosp.hip -- fp32 one-pass even-odd CG iteration on Dhat Dhat^dag and the
// helper kernels of the mixed-precision even-odd solve (gfx950; driver:
// sm_eomp.cpp). It relates to sm_eotd.hip as sm_cgsp.hip relates to sm_cgra.hip.
//
// The pass is sm_eotd.hip's F / H1 / H2 / H3 / H4 march (see its header) on
// float2 checkerboard fields, one-shard contexts only: no face reads, no
// redundant-scalar variant, no peer stores, a separate scalar kernel
// (sm_cgsp.hip's, on MPScalars). Pass j of a segment of inner iterations, on
// the correction y to x:
//     r_{j-1} = d_{j-1} - beta_{j-2} d_{j-2}
//     r_j     = r_{j-1} - alpha_{j-1} Ad_{j-1}          (Ad_{j-1} stored by pass j-1)
//     d_j     = r_j + beta_{j-1} d_{j-1}                (stored)
//     y      <- (y + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}   on even j >= 2
//     W = Dhat^dag d_j,  Ad_j = Dhat W                  (four hops in registers; Ad_j stored)
//     partials |W|^2 (= <d_j, Ad_j>), <r_j, Ad_j>, |r_j|^2, |Ad_j|^2
// A pass reads d_{j-1}, d_{j-2}, Ad_{j-1} (16 B per even site each) and both
// link parities (32) and writes d_j, Ad_j (32), plus y read and written on
// every other pass (16 on average): 128 B per even site against the fp64
// pass's 256.
//
// A segment starts from an INJECTED direction (reliable updates, sm_eomp.cpp):
// d_0 = fp32(r) + beta d_prev with r the fp64 true residual. Pass 0 (FIRST)
// rebuilds r_0 = d_0 - beta d_prev, keeps d_0 (no store, no y update, Ad_{-1}
// not read), forms and stores Ad_0 and the dots; pass 1 reads the same two
// direction buffers again. The very first segment has beta = 0, d_prev = d_0.
//
// Scalars as in sm_cgsp.hip: every dot partial accumulates in fp64 from the
// fp32 values, one partial set per block, summed in a fixed order by
// cg_sp_scalar_kernel, which forms alpha and beta in fp64, keeps M (the largest
// iterated |r| of the segment) and ends the segment on the device; the pass
// uses alpha and beta rounded to fp32.
//
// Links: both parities as float2, pre-scaled by -1/2 with the antiperiodic
// sign of the hop out of t = Nt - 1 folded into U_t (eo_sp_convert_links_kernel;
// powers of two and signs commute with the rounding to fp32). Every bracket
// term carries one link, so a hop's bracket comes out as -H/2: the odd hop
// T = D_oe v is the bracket itself and Dhat v = m v - (1/m) bracket(T).
//
// One float2 per lane; a two-column-per-lane form was not built. The fp32
// arithmetic below the bracket (Spf, the DPP float shifts, the float2 helpers,
// dacc) is sm_device.h's, shared with sm_cgsp.hip and sm_cgbatchsp.hip.
#include <type_traits>

#include "sm_device.h"
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

namespace {

constexpr int EW = kEoTdWaveCols;  // owned k-columns per wave
constexpr int EH = 4;              // halo lanes per side: one per hop

struct EoSPArgs {
    const float2 *d1, *d2, *aold;  // d_{j-1}, d_{j-2}, Ad_{j-1}
    float2 *dn, *anew, *y;
    const float2 *Ue, *Uo;         // pre-scaled checkerboard links: plane 0 U_t, plane 1 U_x
    const MPScalars *sc;
    double2 *partials;             // 2 per block: (|W|^2, <r,Ad>), (|r|^2, |Ad|^2)
    long Vh;
    int Nx, Wh;
    int xchunk, NWT, TBk, XB;
    float mass, imass;             // m, 1 / m
};

// One checkerboard hop's bracket (sm_eotd.hip eo_bracket) with pre-scaled,
// signed links: at a lane whose forward t-neighbour is lane+1 and backward one
// this lane (FWD), or forward this lane and backward lane-1 (!FWD). The shifted
// hop crosses lanes as one complex. Ut / Ux: the target site's links, Ub: the
// source parity's U_t at this lane (the backward hop's link, used by the lane
// that sends), Uxm: the source parity's U_x at row x-1.
template <int DG, bool FWD>
__device__ __forceinline__ Spf eo_bracket_f(const Spf &v, const Spf &vxp, const Spf &vxm, float2 Ut, float2 Ux,
                                            float2 Ub, float2 Uxm) {
    const float2 qf = DG ? addf(v.a, v.b) : subf(v.a, v.b);  // forward-hop combination
    const float2 qb = DG ? subf(v.a, v.b) : addf(v.a, v.b);  // backward-hop combination
    const float2 bp = cmf(f2(Ub.x, -Ub.y), qb);
    float2 A, C;
    if (FWD) {
        A = cmf(Ut, f2(dppf_shl1(qf.x), dppf_shl1(qf.y)));
        C = bp;
    } else {
        A = cmf(Ut, qf);
        C = f2(dppf_shr1(bp.x), dppf_shr1(bp.y));
    }
    const float2 e = f2(Uxm.x, -Uxm.y);
    Spf h;
    if (!DG) {
        const float2 B = cmf(Ux, f2(vxp.a.x - vxp.b.y, vxp.a.y + vxp.b.x));  // px0 + i px1
        const float2 E = cmf(e, f2(vxm.a.x + vxm.b.y, vxm.a.y - vxm.b.x));   // pxm0 - i pxm1
        h.a = addf(addf(addf(A, B), C), E);
        h.b = addf(addf(addf(negf(A), mulmif(B)), C), mulif(E));
    } else {
        const float2 E = cmf(e, f2(vxm.a.x - vxm.b.y, vxm.a.y + vxm.b.x));   // pxm0 + i pxm1
        const float2 B = cmf(Ux, f2(vxp.a.x + vxp.b.y, vxp.a.y - vxp.b.x));  // px0 - i px1
        h.a = addf(addf(addf(C, E), A), B);
        h.b = addf(addf(addf(negf(C), mulmif(E)), A), mulif(B));
    }
    return h;
}

template <int FIRST, int XP>
__global__ void __launch_bounds__(256) eo_sp_kernel(EoSPArgs a) {
    __shared__ double2 sh[4];
    __shared__ float2 rlds[5][2][256];  // r_j of rows y .. y+4
    const MPScalars *sc = a.sc;
    if (sc->done) return;  // grid-uniform: the segment ended in an earlier pass
    // FIRST: alpha = 0, and the injection's beta (kept in sc->beta) rebuilds r_0
    const float alpha = FIRST ? 0.f : (float)sc->alpha;
    const float beta = FIRST ? 0.f : (float)sc->beta;
    const float alpha2 = FIRST ? 0.f : (float)sc->alpha2;
    const float beta2 = FIRST ? (float)sc->beta : (float)sc->beta2;
    const int tb = blockIdx.x % a.TBk, xc = blockIdx.x / a.TBk;
    const int lane = threadIdx.x & 63;
    const int gw = tb * 4 + (threadIdx.x >> 6);
    const int x0 = xc * a.xchunk, xe = min(a.Nx, x0 + a.xchunk);
    double aW = 0.0, aRA = 0.0, aR = 0.0, aA = 0.0;  // |W|^2, <r,Ad>, |r|^2, |Ad|^2
    if (gw < a.NWT && x0 < xe) {
        const int Wh = a.Wh, Nx = a.Nx;
        const long Vh = a.Vh;
        const int k = gw * EW - EH + lane;
        int kw = k % Wh;  // periodic in t: shapes narrower than a wave or than the halo wrap onto themselves
        if (kw < 0) kw += Wh;
        const bool own = lane >= EH && lane < EW + EH && k < Wh;
        const float m = a.mass, im = a.imass;
        auto wrapx = [Nx](int x) { int w = x % Nx; return w < 0 ? w + Nx : w; };
        auto hidx = [&](int y) { return (long)wrapx(y) * Wh + kw; };
        struct Lk {
            float2 et, ex, ot, ox;  // even / odd links at (y, k)
        };
        auto ldl = [&](int y, Lk &L) {
            const long h = hidx(min(max(y, x0 - 4), xe + 2));
            L.et = a.Ue[h];
            L.ex = a.Ue[h + Vh];
            L.ot = a.Uo[h];
            L.ox = a.Uo[h + Vh];
        };
        struct Fr {
            Spf d1, d2, ad, yv;
        };
        auto ldf = [&](int y, Fr &F) {
            const long h = hidx(min(max(y, x0 - 4), xe + 3));
            F.d1 = Spf{a.d1[h], a.d1[h + Vh]};
            F.d2 = Spf{a.d2[h], a.d2[h + Vh]};
            if (!FIRST) F.ad = Spf{a.aold[h], a.aold[h + Vh]};
            if (XP) {
                const long hx = hidx(min(max(y, x0), xe - 1));
                F.yv = Spf{a.y[hx], a.y[hx + Vh]};
            }
        };
        // odd hop at odd site (y, k) from an even field: T = D_oe v (the bracket
        // itself). YE: row y even (backward t-neighbour this lane, forward lane+1).
        auto todd = [&](auto dag, auto ye, const Spf &vc, const Spf &vxm, const Spf &vxp, const Lk &L, float2 ex_m) {
            constexpr int DG = decltype(dag)::value;
            constexpr bool YE = decltype(ye)::value;
            return eo_bracket_f<DG, YE>(vc, vxp, vxm, L.ot, L.ox, L.et, ex_m);
        };
        // even hop at even site (x, k) from an odd field: m v - (1/m) bracket(T).
        // XEV: row x even (backward t-neighbour lane-1, forward this lane).
        auto eout = [&](auto dag, auto xev, const Spf &Tc, const Spf &Txm, const Spf &Txp, const Lk &L, float2 ox_m,
                        const Spf &vc) {
            constexpr int DG = decltype(dag)::value;
            constexpr bool XEV = decltype(xev)::value;
            const Spf h = eo_bracket_f<DG, !XEV>(Tc, Txp, Txm, L.et, L.ex, L.ot, ox_m);
            return Spf{axpyf(-im, h.a, f2(m * vc.a.x, m * vc.a.y)), axpyf(-im, h.b, f2(m * vc.b.x, m * vc.b.y))};
        };
        using DAG1 = std::integral_constant<int, 1>;
        using DAG0 = std::integral_constant<int, 0>;
        const float2 z = f2(0.f, 0.f);
        const Spf zs = Spf{z, z};
        const Lk zl = Lk{z, z, z, z};
        // state at the top of iteration y (links at rows y-1 .. y+2 held, y+3 in flight)
        Fr Fin;                                 // in flight: row y+4
        Lk Lin;                                 // in flight: row y+3
        Lk Lm = zl, L0 = zl, L1 = zl, L2 = zl;  // rows y-1, y, y+1, y+2
        Spf J2 = zs, J3 = zs;                   // d_j rows y+2, y+3
        Spf A1 = zs, A2 = zs;                   // T1 rows y+1, y+2
        Spf W0 = zs, W1 = zs;                   // W rows y, y+1
        Spf B0 = zs, Bm = zs;                   // T2 rows y, y-1
        Fin.ad = zs;
        Fin.yv = zs;
        const int y0 = x0 - 8;
        ldf(y0 + 4, Fin);
        ldl(y0 + 3, Lin);
        int s_w = 4, s_r = 0;                   // r_j ring slots of rows y+4 (written) and y (read)
        // stage mask M: bit 0 H1, bit 1 H2, bit 2 H3, bit 3 H4 (F always)
        // P: parity of row y (x0 is even: Nx and xchunk are)
        auto step = [&](int y, auto mtag, auto ptag) {
            constexpr int M = decltype(mtag)::value;
            constexpr bool E0 = decltype(ptag)::value == 0;  // rows y, y+2, y+4 even
            using PE = std::integral_constant<bool, E0>;
            using PO = std::integral_constant<bool, !E0>;
            const Fr F = Fin;
            const Lk L3 = Lin;
            ldf(y + 5, Fin);
            ldl(y + 4, Lin);
            __builtin_amdgcn_sched_barrier(0);  // keep the next rows' loads issued here
            // F: r_j, d_j at row y+4
            const int xr = y + 4;
            Spf R4, J4;
            R4.a = axpyf(-beta2, F.d2.a, F.d1.a);
            R4.b = axpyf(-beta2, F.d2.b, F.d1.b);
            if (FIRST) {  // the injected direction: r_0 rebuilt, d_0 kept
                J4 = F.d1;
            } else {
                R4.a = axpyf(-alpha, F.ad.a, R4.a);
                R4.b = axpyf(-alpha, F.ad.b, R4.b);
                J4.a = axpyf(beta, F.d1.a, R4.a);
                J4.b = axpyf(beta, F.d1.b, R4.b);
            }
            if (xr >= x0 && xr < xe && own) {
                const long h = (long)xr * Wh + kw;
                if (!FIRST) {
                    a.dn[h] = J4.a;
                    a.dn[h + Vh] = J4.b;
                }
                if (XP) {  // y_j = (y_{j-2} + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}
                    a.y[h] = axpyf(alpha, F.d1.a, axpyf(alpha2, F.d2.a, F.yv.a));
                    a.y[h + Vh] = axpyf(alpha, F.d1.b, axpyf(alpha2, F.d2.b, F.yv.b));
                }
                aR = dacc(aR, R4.a, R4.a);
                aR = dacc(aR, R4.b, R4.b);
            }
            rlds[s_w][0][threadIdx.x] = R4.a;
            rlds[s_w][1][threadIdx.x] = R4.b;
            Spf A3 = zs, W2 = zs, B1 = zs;
            if constexpr ((M & 1) != 0) A3 = todd(DAG1(), PO(), J3, J2, J4, L3, L2.ex);  // H1: T1(y+3)
            if constexpr ((M & 2) != 0) {                                                  // H2: W(y+2)
                W2 = eout(DAG1(), PE(), A2, A1, A3, L2, L1.ox, J2);
                if (y + 2 >= x0 && y + 2 < xe && own) {
                    aW = dacc(aW, W2.a, W2.a);  // |W|^2 = <d_j, Dhat Dhat^dag d_j>
                    aW = dacc(aW, W2.b, W2.b);
                }
            }
            if constexpr ((M & 4) != 0) B1 = todd(DAG0(), PO(), W1, W0, W2, L1, L0.ex);   // H3: T2(y+1)
            if constexpr ((M & 8) != 0) {                                                  // H4: Ad_j(y)
                const Spf o = eout(DAG0(), PE(), B0, Bm, B1, L0, Lm.ox, W0);
                if (own) {
                    const long h = (long)y * Wh + kw;
                    a.anew[h] = o.a;
                    a.anew[h + Vh] = o.b;
                    const Spf R0 = Spf{rlds[s_r][0][threadIdx.x], rlds[s_r][1][threadIdx.x]};
                    aRA = dacc(aRA, R0.a, o.a);
                    aRA = dacc(aRA, R0.b, o.b);
                    aA = dacc(aA, o.a, o.a);
                    aA = dacc(aA, o.b, o.b);
                }
            }
            Lm = L0;
            L0 = L1;
            L1 = L2;
            L2 = L3;
            J2 = J3;
            J3 = J4;
            A1 = A2;
            A2 = A3;
            W0 = W1;
            W1 = W2;
            Bm = B0;
            B0 = B1;
            s_w = s_w == 4 ? 0 : s_w + 1;
            s_r = s_r == 4 ? 0 : s_r + 1;
        };
        using Ev = std::integral_constant<int, 0>;
        using Od = std::integral_constant<int, 1>;
        int y = y0;  // even; every chunk has an even number of rows
        step(y, std::integral_constant<int, 0>(), Ev());
        step(y + 1, std::integral_constant<int, 0>(), Od());
        step(y + 2, std::integral_constant<int, 1>(), Ev());
        step(y + 3, std::integral_constant<int, 1>(), Od());
        step(y + 4, std::integral_constant<int, 3>(), Ev());
        step(y + 5, std::integral_constant<int, 3>(), Od());
        step(y + 6, std::integral_constant<int, 7>(), Ev());
        step(y + 7, std::integral_constant<int, 7>(), Od());
        for (y += 8; y < xe; y += 2) {
            step(y, std::integral_constant<int, 15>(), Ev());
            step(y + 1, std::integral_constant<int, 15>(), Od());
        }
    }
    const double2 s0 = block_sum(make_double2(aW, aRA), sh);
    __syncthreads();
    const double2 s1 = block_sum(make_double2(aR, aA), sh);
    if (threadIdx.x == 0) {
        double2 *p = a.partials + 2 * (long)blockIdx.x;
        p[0] = s0;
        p[1] = s1;
    }
}

// Checkerboard links for the fp32 pass: U_t scaled by -1/2 times the sign of
// the hop out of t = Nt - 1 (t = 2k + ((p + x) & 1), sm_eo.hip), U_x by -1/2.
__global__ void __launch_bounds__(256) eo_sp_convert_links_kernel(long Vh, int Wh, int Nt, const double2 *Ue,
                                                                  const double2 *Uo, float2 *Ue32, float2 *Uo32) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < Vh; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i / Wh), k = (int)(i % Wh);
        const double ke = 2 * k + (x & 1) == Nt - 1 ? 0.5 : -0.5;
        const double ko = 2 * k + ((x + 1) & 1) == Nt - 1 ? 0.5 : -0.5;
        const double2 et = Ue[i], ex = Ue[i + Vh], ot = Uo[i], ox = Uo[i + Vh];
        Ue32[i] = make_float2((float)(ke * et.x), (float)(ke * et.y));
        Ue32[i + Vh] = make_float2((float)(-0.5 * ex.x), (float)(-0.5 * ex.y));
        Uo32[i] = make_float2((float)(ko * ot.x), (float)(ko * ot.y));
        Uo32[i + Vh] = make_float2((float)(-0.5 * ox.x), (float)(-0.5 * ox.y));
    }
}

// x += y (fp64 += fp32), plus alpha_{J-1} d_{J-1} when the segment's last pass
// J = sc->k is odd (y holds the steps up to the last even pass), y = 0.
// discard: y = 0 only.
__global__ void __launch_bounds__(256) eo_mp_fold_kernel(long n, double2 *x, float2 *y, const float2 *dlast,
                                                         const MPScalars *sc, int discard) {
    const int k = sc->k;
    const double alpha = sc->alpha;
    const bool pending = (k & 1) != 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (!discard) {
            const float2 yv = y[i];
            double2 add = make_double2((double)yv.x, (double)yv.y);
            if (pending) {
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

}  // namespace

void launch_eo_sp(hipStream_t s, const Geometry &g, const EoTdCfg &c, const float2 *d1, const float2 *d2,
                  const float2 *aold, float2 *dn, float2 *anew, float2 *y, const float2 *Ue32, const float2 *Uo32,
                  double mass, long pass, const MPScalars *sc, double2 *partials) {
    EoSPArgs a;
    a.d1 = d1; a.d2 = d2; a.aold = aold; a.dn = dn; a.anew = anew; a.y = y;
    a.Ue = Ue32; a.Uo = Uo32; a.sc = sc; a.partials = partials;
    a.Vh = g.V / 2; a.Nx = g.Nx; a.Wh = g.Wt / 2;
    a.xchunk = c.xchunk; a.NWT = c.NWT; a.TBk = c.TBk; a.XB = c.XB;
    a.mass = (float)mass;
    a.imass = (float)(1.0 / mass);
    const dim3 grid(c.TBk * c.XB), block(256);
    if (pass == 0) hipLaunchKernelGGL((eo_sp_kernel<1, 0>), grid, block, 0, s, a);
    else if (pass >= 2 && (pass & 1) == 0) hipLaunchKernelGGL((eo_sp_kernel<0, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((eo_sp_kernel<0, 0>), grid, block, 0, s, a);
}

void launch_eo_sp_convert_links(hipStream_t s, const Geometry &g, const double2 *Ue, const double2 *Uo, float2 *Ue32,
                                float2 *Uo32) {
    hipLaunchKernelGGL(eo_sp_convert_links_kernel, dim3(reduce_blocks(g.V / 2)), dim3(256), 0, s, g.V / 2, g.Wt / 2,
                       g.Wt, Ue, Uo, Ue32, Uo32);
}

void launch_eo_mp_fold(hipStream_t s, long n, double2 *x, float2 *y, const float2 *dlast, const MPScalars *sc,
                       int discard) {
    hipLaunchKernelGGL(eo_mp_fold_kernel, dim3(reduce_blocks(n)), dim3(256), 0, s, n, x, y, dlast, sc, discard);
}

}  // namespace sm
