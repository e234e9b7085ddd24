// sm_eobatch.hip -- one-pass even-odd CG on Dhat Dhat^dag for K columns, one
// launch per iteration (gfx950). Driver: sm_eobatch.cpp.
//
// Arithmetic: sm_eotd.hip's, per column b with that column's own scalars --
// the two-direction recurrence, W = Dhat^dag d_j and Ad_j = Dhat W as four
// checkerboard hops in one march along x (eo_bracket: the folded bracket),
// <d_j, Ad_j> taken as |W|^2, separately rounded complex arithmetic:
//     r_{j-1} = d_{j-1} - d_{j-2} beta_{j-2};  r_j = r_{j-1} - alpha_{j-1} Ad_{j-1}
//     d_j = d_{j-1} beta_{j-1} + r_j;  on even j x <- (x + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}
//     partials (|W|^2, 0), <r_j, Ad_j>, (|r_j|^2, |Ad_j|^2)
// Pass 0 and pass 1 select d_0 / r_0 instead of multiplying by a zero scalar,
// so what an earlier solve left in the ring (a NaN of a zero column included)
// never enters a sum.
//
// Columns: sm_cgbatch.hip's scheme. One block = one wave = one tile of 56
// owned k-columns (64 lanes, 4 halo lanes per side: one per hop) times xchunk
// rows; the grid is K x NWT x NCH tiles, column-major. Column b reads its
// checkerboard links at Ue / Uo + b * ustride and its mass from massv[b]
// (EoBatchLinks): block-uniform, scalar loads. A finished column's tiles return
// at entry. r_j waits four rows for Ad_j in a 5-slot LDS ring that every lane
// reads back itself: no barrier, 10 KiB per tile.
//
// Partials per GRANULE of G rows (2 below Nx = 512, 8 from there; even, since
// the march's row parities are static), a tile is a whole number of granules
// and the column's P = NWT * ceil(Nx / G) slots are summed in slot order. The
// four sums of a granule leave the march at different steps (|r|^2 with row
// y+4, |W|^2 with row y+2, the two Ad sums with row y), each when its own row
// closes the granule. The tile height changes which tile writes a slot, never
// its value: a column's bits do not depend on K, its position, the other
// columns or the tile height.
//
// Scalars: sm_cgbatch.hip's scheme and its kernels (its header has both):
// redundant scalars in the pass up to kBatchRedMaxSlots slots, the scalar
// kernel above; the flush, the start's scalars and finish-x are launched from
// there too (launch_batch_*), on columns of V complex. This file keeps the
// operator: the pass, the hops, the start's residual and the layout kernels.
// No floating-point atomics anywhere.
#include <type_traits>

#include "sm_device.h"
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

namespace {

constexpr int QW = kEoTdWaveCols;  // owned k-columns per wave
constexpr int QH = 4;              // halo lanes per side

struct EOBArgs {
    const double2 *d1, *d2, *aold;  // d_{j-1}, d_{j-2}, Ad_{j-1}: K columns, 2 Vh complex apart
    double2 *dn, *anew, *x;
    const double2 *Ue, *Uo;         // column b's links at + b * ustride
    long ustride;
    const double *massv;            // column b's mass (null: `mass` for all)
    double mass;
    CGScalars *sc;                  // K
    double2 *partials;              // this pass's: column b at + b * pstride, 3 per slot
    const double2 *prev;            // RED: pass j-1's
    long pstride;
    long pass;
    long Vh;
    int Nx, Wh;
    int xchunk, G, NG, NWT, NCH, P;
};

__device__ __forceinline__ double wave_sum1(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// sm_eotd.hip's eo_bracket: one checkerboard hop's bracket at a lane whose
// forward t-neighbour is lane+1 and backward one this lane (FWD), or forward
// this lane and backward lane-1 (!FWD); the shifted hop crosses lanes as one
// complex. Every value equals dirac_bracket_folded's up to the sign of a zero.
template <int DG, bool FWD>
__device__ __forceinline__ void eob_bracket(double sr0, double sl0, const Sp &v, const Sp &vxp, const Sp &vxm,
                                            double2 Ut, double2 Ux, double2 Ub, double2 Uxm, double2 &h0,
                                            double2 &h1) {
    const double2 qf = DG ? cadd(v.a, v.b) : csub(v.a, v.b);
    const double2 qb = DG ? csub(v.a, v.b) : cadd(v.a, v.b);
    const double2 a = make_double2(Ut.x * sr0, Ut.y * sr0);
    double2 A, C;
    if (FWD) {
        A = cmul(a, dpp_shl1(qf));
        C = cmul(make_double2(Ub.x * sl0, -(Ub.y * sl0)), qb);
    } else {
        A = cmul(a, qf);
        const double2 Cs = dpp_shr1(cmul(make_double2(Ub.x, -Ub.y), qb));
        C = make_double2(Cs.x * sl0, Cs.y * sl0);
    }
    const double2 e = make_double2(Uxm.x, -Uxm.y);
    if (!DG) {
        const double2 B = cmul(Ux, make_double2(vxp.a.x - vxp.b.y, vxp.a.y + vxp.b.x));
        const double2 E = cmul(e, make_double2(vxm.a.x + vxm.b.y, vxm.a.y - vxm.b.x));
        h0 = cadd(cadd(cadd(A, B), C), E);
        h1 = cadd(cadd(cadd(cneg(A), mul_mi(B)), C), mul_i(E));
    } else {
        const double2 E = cmul(e, make_double2(vxm.a.x - vxm.b.y, vxm.a.y + vxm.b.x));
        const double2 B = cmul(Ux, make_double2(vxp.a.x + vxp.b.y, vxp.a.y - vxp.b.x));
        h0 = cadd(cadd(cadd(C, E), A), B);
        h1 = cadd(cadd(cadd(cneg(C), mul_mi(E)), A), mul_i(B));
    }
}

// RED: redundant scalars. XP: x takes the updates of passes j-1 and j together.
template <int RED, int XP>
__global__ void __launch_bounds__(64) eo_batch_kernel(EOBArgs a) {
    __shared__ double2 rlds[5][2][64];  // r_j of rows y .. y+4, lane-private
    const int tiles = a.NWT * a.NCH;
    const int b = blockIdx.x / tiles;
    const int w = blockIdx.x - b * tiles;
    const int gw = w % a.NWT, xc = w / a.NWT;
    const int lane = threadIdx.x;
    CGScalars *sc = a.sc + b;
    const double m = a.massv ? a.massv[b] : a.mass;
    const double2 *Ue = a.Ue + (long)b * a.ustride, *Uo = a.Uo + (long)b * a.ustride;
    const bool first = a.pass == 0, rebuild = a.pass >= 2;
    const double2 z2 = make_double2(0.0, 0.0);
    double2 alpha = z2, beta = z2, alpha2 = z2, beta2 = z2;
    if (RED) {
        if (!first) {
            const double2 *prev = a.prev + (long)b * a.pstride;
            double2 acc0 = z2, acc1 = z2, acc2 = z2;
            for (int i = lane; i < a.P; i += 64) {
                acc0 = cadd(acc0, prev[3 * i]);
                acc1 = cadd(acc1, prev[3 * i + 1]);
                acc2 = cadd(acc2, prev[3 * i + 2]);
            }
            CGRed s = sc->red[a.pass & 1];
            if (!s.done) {
                const double2 t0 = wave_sum(acc0), t1 = wave_sum(acc1), t2 = wave_sum(acc2);
                s = cg1_eval(s, sc->tol, sc->phi_norm, sc->max_iter, a.pass == 1, t0, t1, t2);
            }
            if (w == 0 && lane == 0) sc->red[(a.pass - 1) & 1] = s;
            if (s.done) return;  // block-uniform
            alpha = uniform_d2(s.alpha);
            beta = uniform_d2(s.beta);
            alpha2 = uniform_d2(s.alpha2);
            beta2 = uniform_d2(s.beta2);
        }
    } else {
        if (sc->done) return;
        alpha = sc->alpha;
        beta = sc->beta;
        alpha2 = sc->alpha2;
        beta2 = sc->beta2;
    }
    const int Wh = a.Wh, Nx = a.Nx, Ntg = 2 * a.Wh, G = a.G;
    const long Vh = a.Vh, col = (long)b * 2 * Vh;
    const int x0 = xc * a.xchunk, xe = min(Nx, x0 + a.xchunk);
    const int k = gw * QW - QH + lane;
    int kw = k % Wh;
    if (kw < 0) kw += Wh;  // periodic in t; a narrow lattice wraps more than once
    const bool own = lane >= QH && lane < QW + QH && k < Wh;
    const double hm = 0.5 / m;
    const double2 *D1 = a.d1 + col, *D2 = a.d2 + col, *AO = a.aold + col;
    double2 *DN = a.dn + col, *AN = a.anew + col, *X = a.x + col;
    double2 *part = a.partials + (long)b * a.pstride + 3 * (long)gw * a.NG;
    auto wrapx = [Nx](int x) { int q = x % Nx; return q < 0 ? q + Nx : q; };
    auto hidx = [&](int y) { return (long)wrapx(y) * Wh + kw; };
    auto signs = [&](int t, double &sr0, double &sl0) {
        int tg = t % Ntg;
        if (tg < 0) tg += Ntg;
        sr0 = tg == Ntg - 1 ? -1.0 : 1.0;
        sl0 = tg == 0 ? -1.0 : 1.0;
    };
    auto gran_end = [&](int row) { return (row + 1) % G == 0 || row == xe - 1; };  // rows of [x0, xe)
    struct Lk {
        double2 et, ex, ot, ox;  // even / odd links at (y, k)
    };
    auto ldl = [&](int y, Lk &L) {
        const long h = hidx(min(max(y, x0 - 4), xe + 2));
        L.et = Ue[h];
        L.ex = Ue[h + Vh];
        L.ot = Uo[h];
        L.ox = Uo[h + Vh];
    };
    struct Fr {
        Sp d1, d2, ad, xv;
    };
    auto ldf = [&](int y, Fr &F) {
        const long h = hidx(min(max(y, x0 - 4), xe + 3));
        F.d1 = Sp{D1[h], D1[h + Vh]};
        F.d2 = Sp{D2[h], D2[h + Vh]};
        F.ad = Sp{AO[h], AO[h + Vh]};
        if (XP) {
            const long hx = hidx(min(max(y, x0), xe - 1));
            F.xv = Sp{X[hx], X[hx + Vh]};
        }
    };
    // odd hop at odd site (y, k) from an even field: T = -0.5 H_oe v. YE: row y even.
    auto todd = [&](auto dag, auto ye, const Sp &vc, const Sp &vxm, const Sp &vxp, const Lk &L, double2 ex_m) {
        constexpr int DG = decltype(dag)::value;
        constexpr bool YE = decltype(ye)::value;
        double sr0, sl0;
        signs(2 * k + (YE ? 1 : 0), sr0, sl0);
        double2 h0, h1;
        eob_bracket<DG, YE>(sr0, sl0, vc, vxp, vxm, L.ot, L.ox, L.et, ex_m, h0, h1);
        return Sp{rmul(-0.5, h0), rmul(-0.5, h1)};
    };
    // even hop at even site (x, k) from an odd field: m v + (0.5/m) H_eo T. XEV: row x even.
    auto eout = [&](auto dag, auto xev, const Sp &Tc, const Sp &Txm, const Sp &Txp, const Lk &L, double2 ox_m,
                    const Sp &vc) {
        constexpr int DG = decltype(dag)::value;
        constexpr bool XEV = decltype(xev)::value;
        double sr0, sl0;
        signs(2 * k + (XEV ? 0 : 1), sr0, sl0);
        double2 h0, h1;
        eob_bracket<DG, !XEV>(sr0, sl0, Tc, Txp, Txm, L.et, L.ex, L.ot, ox_m, h0, h1);
        return Sp{cadd(rmul(m, vc.a), rmul(hm, h0)), cadd(rmul(m, vc.b), rmul(hm, h1))};
    };
    using DAG1 = std::integral_constant<int, 1>;
    using DAG0 = std::integral_constant<int, 0>;
    const Sp zs = Sp{z2, z2};
    const Lk zl = Lk{z2, z2, z2, z2};
    double aW = 0.0, aR = 0.0, aA = 0.0;  // |W|^2, |r|^2, |Ad|^2 of the running granules
    double2 aRA = z2;                      // <r, Ad>
    Fr Fin;                                 // in flight: row y+4
    Lk Lin;                                 // in flight: row y+3
    Lk Lm = zl, L0 = zl, L1 = zl, L2 = zl;  // rows y-1, y, y+1, y+2
    Sp J2 = zs, J3 = zs;                    // d_j rows y+2, y+3
    Sp A1 = zs, A2 = zs;                    // T1 rows y+1, y+2
    Sp W0 = zs, W1 = zs;                    // W rows y, y+1
    Sp B0 = zs, Bm = zs;                    // T2 rows y, y-1
    Fin.xv = zs;
    const int y0 = x0 - 8;
    ldf(y0 + 4, Fin);
    ldl(y0 + 3, Lin);
    int s_w = 4, s_r = 0;                   // ring slots of rows y+4 (written) and y (read)
    // stage mask M: bit 0 H1, bit 1 H2, bit 2 H3, bit 3 H4 (F always); P: parity of row y (x0 is even)
    auto step = [&](int y, auto mtag, auto ptag) {
        constexpr int M = decltype(mtag)::value;
        constexpr bool E0 = decltype(ptag)::value == 0;
        using PE = std::integral_constant<bool, E0>;
        using PO = std::integral_constant<bool, !E0>;
        const Fr F = Fin;
        const Lk L3 = Lin;
        ldf(y + 5, Fin);
        ldl(y + 4, Lin);
        __builtin_amdgcn_sched_barrier(0);
        // F: r_j, d_j at row y+4
        const int xr = y + 4;
        Sp rp, R4, J4;
        rp.a = rebuild ? csub(F.d1.a, cmul(F.d2.a, beta2)) : F.d1.a;
        rp.b = rebuild ? csub(F.d1.b, cmul(F.d2.b, beta2)) : F.d1.b;
        R4.a = first ? rp.a : csub(rp.a, cmul(alpha, F.ad.a));
        R4.b = first ? rp.b : csub(rp.b, cmul(alpha, F.ad.b));
        J4.a = first ? F.d1.a : cadd(cmul(F.d1.a, beta), R4.a);
        J4.b = first ? F.d1.b : cadd(cmul(F.d1.b, beta), R4.b);
        if (xr >= x0 && xr < xe) {
            if (own) {
                const long h = (long)xr * Wh + kw;
                st_nt(DN + h, J4.a);
                st_nt(DN + h + Vh, J4.b);
                if (XP) {
                    st_nt(X + h, cadd(cadd(F.xv.a, cmul(alpha2, F.d2.a)), cmul(alpha, F.d1.a)));
                    st_nt(X + h + Vh, cadd(cadd(F.xv.b, cmul(alpha2, F.d2.b)), cmul(alpha, F.d1.b)));
                }
                aR += cmul(R4.a, cconj(R4.a)).x;
                aR += cmul(R4.b, cconj(R4.b)).x;
            }
            if (gran_end(xr)) {  // wave-uniform
                const double s = wave_sum1(aR);
                if (lane == 0) part[3 * (long)(xr / G) + 2].x = s;
                aR = 0.0;
            }
        }
        rlds[s_w][0][lane] = R4.a;
        rlds[s_w][1][lane] = R4.b;
        Sp A3 = zs, W2 = zs, B1 = zs;
        if constexpr ((M & 1) != 0) A3 = todd(DAG1(), PO(), J3, J2, J4, L3, L2.ex);  // H1: T1(y+3)
        if constexpr ((M & 2) != 0) {                                                  // H2: W(y+2)
            W2 = eout(DAG1(), PE(), A2, A1, A3, L2, L1.ox, J2);
            const int xw = y + 2;
            if (xw >= x0 && xw < xe) {
                if (own) {
                    aW += cmul(W2.a, cconj(W2.a)).x;  // |W|^2 = <d_j, Dhat Dhat^dag d_j>
                    aW += cmul(W2.b, cconj(W2.b)).x;
                }
                if (gran_end(xw)) {
                    const double s = wave_sum1(aW);
                    if (lane == 0) part[3 * (long)(xw / G)] = make_double2(s, 0.0);
                    aW = 0.0;
                }
            }
        }
        if constexpr ((M & 4) != 0) B1 = todd(DAG0(), PO(), W1, W0, W2, L1, L0.ex);   // H3: T2(y+1)
        if constexpr ((M & 8) != 0) {                                                  // H4: Ad_j(y), y in [x0, xe)
            const Sp o = eout(DAG0(), PE(), B0, Bm, B1, L0, Lm.ox, W0);
            if (own) {
                const long h = (long)y * Wh + kw;
                st_nt(AN + h, o.a);
                st_nt(AN + h + Vh, o.b);
                const Sp R0 = Sp{rlds[s_r][0][lane], rlds[s_r][1][lane]};
                aRA = cadd(aRA, cmul(R0.a, cconj(o.a)));  // dot(r, Ad)
                aRA = cadd(aRA, cmul(R0.b, cconj(o.b)));
                aA += cmul(o.a, cconj(o.a)).x;
                aA += cmul(o.b, cconj(o.b)).x;
            }
            if (gran_end(y)) {
                const double2 s1 = wave_sum(aRA);
                const double s2 = wave_sum1(aA);
                if (lane == 0) {
                    double2 *p = part + 3 * (long)(y / G);
                    p[1] = s1;
                    p[2].y = s2;
                }
                aRA = z2;
                aA = 0.0;
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
    int y = y0;  // even; every tile has an even number of rows
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

// ---- layout: full <-> checkerboard, column / replica b = blockIdx.y ----------
// (to_cb_kernel's / from_cb_kernel's site map, sm_eo.hip; either parity may be null)
__global__ void __launch_bounds__(256) eob_to_cb_kernel(int Wt, long V, const double2 *full, double2 *e, double2 *o) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= V) return;
    const int Wh = Wt / 2;
    const long Vh = V / 2;
    const int x = (int)(n / Wt), t = (int)(n - (long)x * Wt);
    const long h = (long)x * Wh + (t >> 1);
    double2 *dst = ((x + t) & 1) ? o : e;
    if (!dst) return;
    dst += b * V;
    full += b * 2 * V;
    dst[h] = full[n];
    dst[h + Vh] = full[n + V];
}

__global__ void __launch_bounds__(256) eob_from_cb_kernel(int Wt, long V, const double2 *e, const double2 *o,
                                                          double2 *full) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= V) return;
    const int Wh = Wt / 2;
    const long Vh = V / 2;
    const int x = (int)(n / Wt), t = (int)(n - (long)x * Wt);
    const long h = (long)x * Wh + (t >> 1);
    const double2 *src = ((x + t) & 1) ? o : e;
    double2 v0 = make_double2(0.0, 0.0), v1 = v0;
    if (src) {
        v0 = src[b * V + h];
        v1 = src[b * V + h + Vh];
    }
    full[b * 2 * V + n] = v0;
    full[b * 2 * V + n + V] = v1;
}

// One checkerboard hop of every column (eo_hop_kernel's site arithmetic, one
// shard): out_p = H in_q scaled by column b's mass m,
//   mode 0: -0.5 H in;  mode 1: m aux + (0.5/m) H in;  mode 2: (0.5/m) H in.
template <int DAG>
__global__ void __launch_bounds__(256) eob_hop_kernel(int Nx, int Wh, long Vh, int p, int mode, const double2 *in,
                                                      const double2 *aux, EoBatchLinks l, double2 *out) {
    const long b = blockIdx.y, h = (long)blockIdx.x * 256 + threadIdx.x;
    const double m = l.massv ? l.massv[b] : l.mass;
    if (h >= Vh) return;
    const double2 *Up = (p ? l.Uo : l.Ue) + b * l.ustride, *Uq = (p ? l.Ue : l.Uo) + b * l.ustride;
    in += b * 2 * Vh;
    out += b * 2 * Vh;
    const int x = (int)(h / Wh), k = (int)(h - (long)x * Wh);
    const int s = (p + x) & 1;
    const int t = 2 * k + s;
    int kp = k + s, km = k + s - 1;
    if (kp == Wh) kp = 0;
    if (km < 0) km = Wh - 1;
    const int xp = x + 1 == Nx ? 0 : x + 1, xm = x == 0 ? Nx - 1 : x - 1;
    const long row = (long)x * Wh;
    const long ixp = (long)xp * Wh + k, ixm = (long)xm * Wh + k;
    const double sr0 = t == 2 * Wh - 1 ? -1.0 : 1.0;
    const double sl0 = t == 0 ? -1.0 : 1.0;
    double2 h0, h1;
    dirac_bracket<DAG>(sr0, sl0, in[row + kp], in[row + kp + Vh], in[ixp], in[ixp + Vh], in[row + km],
                       in[row + km + Vh], in[ixm], in[ixm + Vh], Up[h], Up[h + Vh], Uq[row + km], Uq[ixm + Vh], h0,
                       h1);
    const double bs = mode == 0 ? -0.5 : 0.5 / m;
    double2 o0 = rmul(bs, h0), o1 = rmul(bs, h1);
    if (mode == 1) {
        aux += b * 2 * Vh;
        o0 = cadd(rmul(m, aux[h]), o0);
        o1 = cadd(rmul(m, aux[h + Vh]), o1);
    }
    out[h] = o0;
    out[h + Vh] = o1;
}

// ---- the start: x = phi, d_0 = r_0 = phi - A (A = Dhat Dhat^dag phi), init sums
// grid K x NB0: block q of column b takes entries q*256 + tid, + NB0*256, ... of the column's 2 Vh
__global__ void __launch_bounds__(256) eob_init_kernel(int NB0, long n2, const double2 *phi, const double2 *A,
                                                       double2 *x, double2 *d0, double2 *partials, long pstride) {
    __shared__ double2 sh[4];
    const int b = blockIdx.x / NB0, q = blockIdx.x - b * NB0;
    const long col = (long)b * n2;
    double2 arr = make_double2(0.0, 0.0), app = make_double2(0.0, 0.0);
    for (long i = (long)q * 256 + threadIdx.x; i < n2; i += (long)NB0 * 256) {
        const double2 ph = phi[col + i];
        const double2 r = csub(ph, A[col + i]);
        x[col + i] = ph;
        d0[col + i] = r;
        arr = cadd(arr, cmul(r, cconj(r)));
        app = cadd(app, cmul(ph, cconj(ph)));
    }
    const double2 s1 = block_sum(arr, sh);
    __syncthreads();
    const double2 s2 = block_sum(app, sh);
    if (threadIdx.x == 0) {
        double2 *pp = partials + (long)b * pstride + 2 * q;
        pp[0] = s1;
        pp[1] = s2;
    }
}

}  // namespace

BatchCfg eo_batch_config(const Geometry &g, int K, int target_tiles) {
    return batch_config(g, K, QW, g.Wt / 2, 2, target_tiles < 1 ? kEoBatchTargetTiles : target_tiles);
}

void launch_eob_to_cb(hipStream_t s, const Geometry &g, int K, const double2 *full, double2 *e, double2 *o) {
    hipLaunchKernelGGL(eob_to_cb_kernel, dim3((unsigned)((g.V + 255) / 256), (unsigned)K), dim3(256), 0, s, g.Wt, g.V,
                       full, e, o);
}

void launch_eob_from_cb(hipStream_t s, const Geometry &g, int K, const double2 *e, const double2 *o, double2 *full) {
    hipLaunchKernelGGL(eob_from_cb_kernel, dim3((unsigned)((g.V + 255) / 256), (unsigned)K), dim3(256), 0, s, g.Wt,
                       g.V, e, o, full);
}

void launch_eob_hop(hipStream_t s, const Geometry &g, int K, int dagger, int p, int mode, const double2 *in,
                    const double2 *aux, double2 *out, const EoBatchLinks &l) {
    const long Vh = g.V / 2;
    const dim3 grid((unsigned)((Vh + 255) / 256), (unsigned)K);
    const int Wh = g.Wt / 2;
    if (dagger) hipLaunchKernelGGL(eob_hop_kernel<1>, grid, dim3(256), 0, s, g.Nx, Wh, Vh, p, mode, in, aux, l, out);
    else hipLaunchKernelGGL(eob_hop_kernel<0>, grid, dim3(256), 0, s, g.Nx, Wh, Vh, p, mode, in, aux, l, out);
}

void launch_eob_dhat(hipStream_t s, const Geometry &g, int K, int dagger, const double2 *v, double2 *T, double2 *out,
                     const EoBatchLinks &l) {
    launch_eob_hop(s, g, K, dagger, 1, 0, v, nullptr, T, l);  // T = D_oe v
    launch_eob_hop(s, g, K, dagger, 0, 1, T, v, out, l);      // m v + (0.5/m) H_eo T
}

void launch_eo_batch_init(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *phi, double2 *x,
                          double2 *T, double2 *W, double2 *A, double2 *d0, const EoBatchLinks &l, double tol,
                          int max_iter, double2 *partials, CGScalars *sc) {
    launch_eob_dhat(s, g, K, 1, phi, T, W, l);
    launch_eob_dhat(s, g, K, 0, W, T, A, l);
    hipLaunchKernelGGL(eob_init_kernel, dim3(K * c.NB0), dim3(256), 0, s, c.NB0, g.V, phi, A, x, d0, partials,
                       c.pstride);
    launch_batch_init_scalars(s, c, K, partials, sc, tol, max_iter);
}

void launch_eo_batch_pass(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *d1,
                          const double2 *d2, const double2 *aold, double2 *dn, double2 *anew, double2 *x,
                          const EoBatchLinks &l, long pass, CGScalars *sc, double2 *partials) {
    EOBArgs a;
    a.d1 = d1; a.d2 = d2; a.aold = aold; a.dn = dn; a.anew = anew; a.x = x;
    a.Ue = l.Ue; a.Uo = l.Uo; a.ustride = l.ustride; a.massv = l.massv; a.mass = l.mass;
    a.Vh = g.V / 2; a.Nx = g.Nx; a.Wh = g.Wt / 2;
    void (*const kern[2][2])(EOBArgs) = {{eo_batch_kernel<0, 0>, eo_batch_kernel<0, 1>},
                                         {eo_batch_kernel<1, 0>, eo_batch_kernel<1, 1>}};
    launch_batch_pass(s, c, K, pass, sc, partials, a, kern);
}

}  // namespace sm
