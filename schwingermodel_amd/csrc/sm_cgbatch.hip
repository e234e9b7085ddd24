// sm_cgbatch.hip -- CG on D D^dag for K right-hand sides on one gauge field, one
// launch per iteration (gfx950), and the pion correlator's kernels on top of it.
// Driver: sm_cgbatch.cpp.
//
// Why: below 256^2 one CG iteration of sm_cgfused.hip costs 11-12 us whatever
// the lattice (launch, then each block's dependent loads); K independent
// systems share the launch, the prologue and the scalar step.
//
// Mathematics: the stored-Ad two-direction pass of sm_cgfused.hip (its header
// has the recurrences), per column b with that column's own scalars:
//     r_{j-1} = d_{j-1} - d_{j-2} beta_{j-2} ;  r_j = r_{j-1} - alpha_{j-1} Ad_{j-1}
//     d_j = d_{j-1} beta_{j-1} + r_j ;  x <- (x + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1} on even j
//     Ad_j = D D^dag d_j ; partials of <d_j,Ad_j>, <r_j,Ad_j>, |r_j|^2, |Ad_j|^2
// with the reference's separately rounded complex arithmetic (no contraction).
//
// Geometry. One block = one wave = one tile: 60 owned t-columns (64 lanes, 2
// halo lanes per side, t-neighbours by DPP shifts) times xchunk rows marched
// along x. No LDS, no barrier. The grid is K x NWT x NCH tiles, column-major
// (all tiles of column 0, then column 1, ...).
//
// Links. Column b reads its links at U + b * ustride and uses its own mass
// (BatchLinks, sm_internal.h): both come from scalar loads at the head of the
// block and stay in SGPRs, no row reads them again. ustride = 0 with one mass
// is the shared field of sm_cg_batch and the correlator (the arithmetic it had
// before per-column links existed); a replica ensemble (sm_ens.cpp) gives
// every column its own field and mass. Neither enters another column's
// arithmetic.
//
// A column's sums must not depend on K, yet the tile height should: few
// columns want one row per tile (parallelism), many columns want taller tiles
// (4 halo rows are recomputed per tile). So partials are kept per GRANULE of G
// rows (G depends on the lattice only: 1 below Nx = 512, 8 from there), a tile
// is a whole number of granules, and the column's P = NWT * ceil(Nx / G) slots
// are summed in slot order: lane l takes slots l, l + 64, ..., then one
// butterfly. The tile height changes which block writes a slot, never the
// slot's value or the order of the sum, so column b computes the same bits
// alone, in any position of any batch, and at any tile height.
//
// Scalars. P <= kBatchRedMaxSlots (64^2: 128, 128^2: 384): redundant scalars --
// every tile of pass j sums its OWN column's partials of pass j-1 (by pass
// parity) and evaluates S_{j-1} itself; the column's first tile keeps it in
// red[(j-1) & 1] (cg1_redundant's scheme). The loads of the state and of the
// partials are issued together (the partial loads do not wait for `done`): one
// L2 round trip ahead of the march instead of two. Larger P: a scalar kernel of
// K blocks after each pass. A finished column's tiles return at entry, its
// fields, scalars and partials are never touched again.
//
// Everything of this scheme outside the pass kernel -- the slot-order sum, the
// scalar kernel, the flush for the host, the start's scalars and finish-x, with
// BatchCfg and its arithmetic (batch_config) -- is written for a column of n
// complex and P slots, not for this operator: the even-odd solver
// (sm_eobatch.hip) launches the same kernels through launch_batch_scalars,
// launch_batch_flush, launch_batch_init_scalars and launch_batch_finish_x, and
// both pass launchers end in sm_device.h's launch_batch_pass. A column's bits
// depend on the slot-order sum and on cg1_eval / cg1_update; there is one copy
// of each.
#include "sm_device.h"
#include "sm_internal.h"

#pragma clang fp contract(off)

namespace sm {

constexpr int BW = kFusedWaveCols;  // owned t-columns per wave

struct CGBArgs {
    const double2 *dold, *rold, *aold;  // d_{j-1}, d_{j-2}, Ad_{j-1}: K columns, 2V complex apart
    double2 *dnew, *anew;               // d_j, Ad_j
    double2 *x;
    const double2 *U;                   // column b's links at U + b * ustride (0: one field for all)
    long ustride;
    const double *massv;                // column b's mass (null: `mass` for all)
    CGScalars *sc;                      // K
    double2 *partials;                  // this pass's: column b at + b * pstride, 3 per slot
    const double2 *prev;                // RED: pass j-1's
    long pstride;
    long pass;                          // j
    long V;
    int Nx, Wt;
    int xchunk, G, NG, NWT, NCH, P;
    double mass;
};

struct RawB {
    double2 d0, d1, r0, r1, a0, a1, ut, ux, x0, x1;
};

// RED: redundant scalars. XP: x takes the updates of passes j-1 and j together.
template <int RED, int XP>
__global__ void __launch_bounds__(64) cg_batch_kernel(CGBArgs a) {
    const int tiles = a.NWT * a.NCH;
    const int b = blockIdx.x / tiles;
    const int w = blockIdx.x - b * tiles;
    const int g = w % a.NWT, xc = w / a.NWT;
    const int lane = threadIdx.x;
    CGScalars *sc = a.sc + b;
    // the column's mass and link base: block-uniform, scalar loads issued ahead of everything else
    const double mass = a.massv ? a.massv[b] : a.mass;
    const double2 *Ub = a.U + (long)b * a.ustride;
    const bool first = a.pass == 0;
    const double2 zz = make_double2(0.0, 0.0);
    double2 alpha = zz, beta = zz, alpha2 = zz, beta2 = zz;  // alpha_{j-1}, beta_{j-1}, alpha_{j-2}, beta_{j-2}
    if (RED) {
        if (!first) {
            const double2 *prev = a.prev + (long)b * a.pstride;
            double2 acc0 = zz, acc1 = zz, acc2 = zz;
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
    const int Nx = a.Nx, Wt = a.Wt;
    const long V = a.V, col = (long)b * 2 * V;
    const int x0 = xc * a.xchunk;
    const int xe = min(Nx, x0 + a.xchunk);
    const int c = g * BW - 2 + lane;
    const bool own = lane >= 2 && lane < BW + 2 && c < Wt;
    int cw = c % Wt;  // periodic wrap (one shard)
    if (cw < 0) cw += Wt;
    const double sr0 = cw == Wt - 1 ? -1.0 : 1.0;  // SignR[2n], include/dirac_operator.h:53-55
    const double sl0 = cw == 0 ? -1.0 : 1.0;       // SignL[2n], :56-58
    const double2 *Sd = a.dold + col + cw, *Sr = a.rold + col + cw, *Sa = a.aold + col + cw;
    const double2 *Su = Ub + cw;
    double2 *xb = a.x + col, *dn_ = a.dnew + col, *an_ = a.anew + col;
    auto wrap = [Nx](int x) { int q = x % Nx; return q < 0 ? q + Nx : q; };
    auto load = [&](int xr, RawB &R) {
        const long pr = (long)wrap(xr) * Wt;
        R.d0 = Sd[pr];
        R.d1 = Sd[pr + V];
        R.r0 = Sr[pr];
        R.r1 = Sr[pr + V];
        R.a0 = Sa[pr];
        R.a1 = Sa[pr + V];
        const long pu = (long)wrap(min(xr, xe)) * Wt;
        R.ut = Su[pu];
        R.ux = Su[pu + V];
        if (XP) {
            const long nx = (long)wrap(min(max(xr, x0), xe - 1)) * Wt + cw;
            R.x0 = xb[nx];
            R.x1 = xb[nx + V];
        }
    };
    const bool rebuild = a.pass >= 2;  // pass 1 has r_0 = d_0 (no d_{-1})
    // r_j and d_j of row xr; on owned rows store d_j and x_j
    auto form = [&](int xr, const RawB &R, Sp &rj) {
        Sp rp;  // r_{j-1}: d_{j-1} = d_{j-2} beta_{j-2} + r_{j-1}
        rp.a = rebuild ? csub(R.d0, cmul(R.r0, beta2)) : R.d0;
        rp.b = rebuild ? csub(R.d1, cmul(R.r1, beta2)) : R.d1;
        rj.a = first ? rp.a : csub(rp.a, cmul(alpha, R.a0));
        rj.b = first ? rp.b : csub(rp.b, cmul(alpha, R.a1));
        Sp d;
        d.a = first ? R.d0 : cadd(cmul(R.d0, beta), rj.a);
        d.b = first ? R.d1 : cadd(cmul(R.d1, beta), rj.b);
        if (xr >= x0 && xr < xe && own) {
            const long n = (long)xr * Wt + c;
            st_nt(dn_ + n, d.a);
            st_nt(dn_ + n + V, d.b);
            if (XP) {  // x_j = (x_{j-2} + alpha_{j-2} d_{j-2}) + alpha_{j-1} d_{j-1}
                st_nt(xb + n, cadd(cadd(R.x0, cmul(alpha2, R.r0)), cmul(alpha, R.d0)));
                st_nt(xb + n + V, cadd(cadd(R.x1, cmul(alpha2, R.r1)), cmul(alpha, R.d1)));
            }
        }
        return d;
    };
    auto ddag = [&](const Sp &p, const Sp &pxm, const Sp &pxp, double2 ut, double2 ux, double2 uxm,
                    double2 &utm_out) {
        const Sp pm = shr(p), pp = shl(p);
        utm_out = dpp_shr1(ut);
        Sp o;
        dirac_site<1>(mass, sr0, sl0, p.a, p.b, pp.a, pp.b, pxp.a, pxp.b, pm.a, pm.b, pxm.a, pxm.b, ut, ux,
                      utm_out, uxm, o.a, o.b);
        return o;
    };
    double2 acc_dA = zz, acc_rA = zz, acc_n = zz;  // <d,Ad>, <r,Ad>, (|r|^2, |Ad|^2) of the running granule
    double2 *part = a.partials + (long)b * a.pstride + 3 * (long)g * a.NG;
    RawB R;
    Sp rj;
    load(x0 - 2, R);
    Sp dm2 = form(x0 - 2, R, rj);
    double2 uxm2 = R.ux;
    load(x0 - 1, R);
    Sp dm1 = form(x0 - 1, R, rj);
    double2 utm1 = R.ut, uxm1 = R.ux;
    load(x0, R);
    Sp rc;
    Sp dc = form(x0, R, rc);
    double2 utc = R.ut, uxc = R.ux;
    load(x0 + 1, R);
    Sp rn;
    Sp dn = form(x0 + 1, R, rn);
    double2 utn = R.ut, uxn = R.ux;
    load(x0 + 2, R);
    double2 dummy;
    Sp Tp = ddag(dm1, dm2, dc, utm1, uxm1, uxm2, dummy);
    double2 utmc;
    Sp Tc = ddag(dc, dm1, dn, utc, uxc, uxm1, utmc);
    double2 uxp = uxm1;
    for (int x = x0; x < xe; ++x) {
        Sp r2;
        const Sp d2 = form(x + 2, R, r2);
        const double2 ut2 = R.ut, ux2 = R.ux;
        load(min(x + 3, xe + 1), R);
        __builtin_amdgcn_sched_barrier(0);
        double2 utmn;
        const Sp Tn = ddag(dn, dc, d2, utn, uxn, uxc, utmn);
        const Sp Tm = shr(Tc), Tq = shl(Tc);
        Sp o;
        dirac_site<0>(mass, sr0, sl0, Tc.a, Tc.b, Tq.a, Tq.b, Tn.a, Tn.b, Tm.a, Tm.b, Tp.a, Tp.b, utc, uxc, utmc,
                      uxp, o.a, o.b);
        if (own) {
            const long n = (long)x * Wt + c;
            st_nt(an_ + n, o.a);
            st_nt(an_ + n + V, o.b);
            acc_dA = cadd(acc_dA, cmul(dc.a, cconj(o.a)));  // dot(d, Ad)
            acc_dA = cadd(acc_dA, cmul(dc.b, cconj(o.b)));
            acc_rA = cadd(acc_rA, cmul(rc.a, cconj(o.a)));  // dot(r, Ad)
            acc_rA = cadd(acc_rA, cmul(rc.b, cconj(o.b)));
            acc_n.x += cmul(rc.a, cconj(rc.a)).x;           // Re dot(r, r), include/variables.h:185-188
            acc_n.x += cmul(rc.b, cconj(rc.b)).x;
            acc_n.y += cmul(o.a, cconj(o.a)).x;             // |Ad|^2
            acc_n.y += cmul(o.b, cconj(o.b)).x;
        }
        if ((x + 1) % a.G == 0 || x == xe - 1) {  // the granule x / G is complete (x0 is a multiple of G)
            const double2 s0 = wave_sum(acc_dA), s1 = wave_sum(acc_rA), s2 = wave_sum(acc_n);
            if (lane == 0) {
                double2 *p = part + 3 * (long)(x / a.G);
                p[0] = s0;
                p[1] = s1;
                p[2] = s2;
            }
            acc_dA = acc_rA = acc_n = zz;
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
        utmc = utmn;
        utn = ut2;
        uxn = ux2;
    }
}

// A column's three sums in slot order, by one block of 256 threads: thread i
// takes slots i, i + 256, ...; block_sum's fixed order after that.
__device__ __forceinline__ void batch_sum3(int P, const double2 *part, double2 *sh, double2 t[3]) {
    const double2 zz = make_double2(0.0, 0.0);
    double2 acc[3] = {zz, zz, zz};
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        acc[0] = cadd(acc[0], part[3 * (long)i]);
        acc[1] = cadd(acc[1], part[3 * (long)i + 1]);
        acc[2] = cadd(acc[2], part[3 * (long)i + 2]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        t[q] = block_sum(acc[q], sh);
        __syncthreads();
    }
}

// Scalar step of the non-redundant path: block b evaluates column b.
__global__ void __launch_bounds__(256) batch_scalar_kernel(int P, const double2 *partials, long pstride, CGScalars *sc,
                                                           int first) {
    __shared__ double2 sh[4];
    sc += blockIdx.x;
    if (sc->done) return;
    double2 t[3];
    batch_sum3(P, partials + blockIdx.x * pstride, sh, t);
    if (threadIdx.x == 0) cg1_update(sc, first, t[0], t[1], t[2]);
}

// Redundant path: S_J of the last issued pass J for the host, one wave per
// column, summed as the pass's tiles sum (the next pass recomputes the same S_J).
__global__ void __launch_bounds__(64) batch_flush_kernel(int P, const double2 *partials, long pstride, CGScalars *sc,
                                                         long J) {
    sc += blockIdx.x;
    const double2 *prev = partials + blockIdx.x * pstride;
    const double2 zz = make_double2(0.0, 0.0);
    double2 acc0 = zz, acc1 = zz, acc2 = zz;
    for (int i = threadIdx.x; i < P; i += 64) {
        acc0 = cadd(acc0, prev[3 * i]);
        acc1 = cadd(acc1, prev[3 * i + 1]);
        acc2 = cadd(acc2, prev[3 * i + 2]);
    }
    CGRed s = sc->red[(J + 1) & 1];  // S_{J-1}
    if (!s.done) {
        const double2 t0 = wave_sum(acc0), t1 = wave_sum(acc1), t2 = wave_sum(acc2);
        s = cg1_eval(s, sc->tol, sc->phi_norm, sc->max_iter, J == 0, t0, t1, t2);
    }
    if (threadIdx.x == 0) {
        sc->red[J & 1] = s;
        store_state(sc, s);
    }
}

// ---- the start of a solve: x = phi, r_0 = phi - D D^dag phi, d_0 = r_0 -------
// One thread per site, periodic neighbours (one shard): site_apply, sm_device.h.

// out_b = D in_b (DAG = 0) or D^dag in_b (1) on column b's links and mass;
// grid NBA x K: block (q, b) takes sites q*256 + tid of column b
template <int DAG>
__global__ void __launch_bounds__(256) batch_apply_kernel(int Nx, int Wt, long V, const double2 *in, BatchLinks l,
                                                          double2 *out) {
    const long b = blockIdx.y, n = (long)blockIdx.x * 256 + threadIdx.x;
    const double mass = l.massv ? l.massv[b] : l.mass;
    if (n >= V) return;
    const int x = (int)(n / Wt), t = (int)(n - (long)x * Wt);
    double2 o0, o1;
    site_apply<DAG>(in + b * 2 * V, l.U + b * l.ustride, Nx, Wt, V, mass, x, t, o0, o1);
    out[b * 2 * V + n] = o0;
    out[b * 2 * V + n + V] = o1;
}

// grid K x NB0: block q of column b takes sites q*256 + tid, + NB0*256, ...
__global__ void __launch_bounds__(256) batch_init_kernel(int NB0, int Nx, int Wt, long V, const double2 *phi,
                                                         const double2 *T, BatchLinks l, double2 *x, double2 *d0,
                                                         double2 *partials, long pstride) {
    __shared__ double2 sh[4];
    const int b = blockIdx.x / NB0, q = blockIdx.x - b * NB0;
    const long col = (long)b * 2 * V;
    const double mass = l.massv ? l.massv[b] : l.mass;
    const double2 *U = l.U + (long)b * l.ustride;
    double2 arr = make_double2(0.0, 0.0), app = make_double2(0.0, 0.0);
    for (long n = (long)q * 256 + threadIdx.x; n < V; n += (long)NB0 * 256) {
        const int xx = (int)(n / Wt), t = (int)(n - (long)xx * Wt);
        double2 A0, A1;
        site_apply<0>(T + col, U, Nx, Wt, V, mass, xx, t, A0, A1);
        const double2 p0 = phi[col + n], p1 = phi[col + n + V];
        const double2 r0 = csub(p0, A0), r1 = csub(p1, A1);
        x[col + n] = p0;
        x[col + n + V] = p1;
        d0[col + n] = r0;
        d0[col + n + V] = r1;
        arr = cadd(arr, cmul(r0, cconj(r0)));
        arr = cadd(arr, cmul(r1, cconj(r1)));
        app = cadd(app, cmul(p0, cconj(p0)));
        app = cadd(app, cmul(p1, cconj(p1)));
    }
    const double2 s1 = block_sum(arr, sh);
    __syncthreads();
    const double2 s2 = block_sum(app, sh);
    if (threadIdx.x == 0) {
        double2 *p = partials + (long)b * pstride + 2 * q;
        p[0] = s1;
        p[1] = s2;
    }
}

__global__ void __launch_bounds__(256) batch_init_scalars_kernel(int NB0, const double2 *partials, long pstride,
                                                                 CGScalars *sc, double tol, int max_iter) {
    __shared__ double2 sh[4];
    sc += blockIdx.x;
    const double2 *p = partials + blockIdx.x * pstride;
    double2 arr = make_double2(0.0, 0.0), app = make_double2(0.0, 0.0);
    for (int i = threadIdx.x; i < NB0; i += 256) {
        arr = cadd(arr, p[2 * i]);
        app = cadd(app, p[2 * i + 1]);
    }
    const double2 rr = block_sum(arr, sh);
    __syncthreads();
    const double2 pp = block_sum(app, sh);
    if (threadIdx.x == 0) {
        const double2 zz = make_double2(0.0, 0.0);
        sc->rn = rr;
        sc->phi_norm = sqrt(pp.x);
        sc->tol = tol;
        sc->err = 0.0;
        sc->k = 0;
        sc->done = 0;
        sc->converged = 0;
        sc->max_iter = max_iter;
        sc->alpha = sc->beta = sc->alpha2 = sc->beta2 = sc->sum = zz;
        CGRed s0;  // S_-1
        s0.rn = rr;
        s0.alpha = s0.beta = s0.alpha2 = s0.beta2 = zz;
        s0.err = 0.0;
        s0.k = s0.done = s0.converged = s0.pad = 0;
        sc->red[0] = s0;
        sc->red[1] = s0;
    }
}

// After the last pass: a column (n complex) whose iteration count k is odd still
// lacks alpha_{k-1} d_{k-1} in x (cg_td_finish_x_kernel's rule, per column).
__global__ void __launch_bounds__(256) batch_finish_x_kernel(int NBF, long n, double2 *x, const double2 *d0,
                                                             const double2 *d1, const double2 *d2,
                                                             const CGScalars *sc) {
    const int b = blockIdx.x / NBF, q = blockIdx.x - b * NBF;
    sc += b;
    const int k = sc->k;
    if (k < 1 || !(k & 1)) return;
    const double2 alpha = sc->done ? sc->alpha : sc->alpha2;
    const int i3 = (k - 1) % 3;
    const long col = (long)b * n;
    const double2 *d = (i3 == 0 ? d0 : (i3 == 1 ? d1 : d2)) + col;
    for (long i = (long)q * 256 + threadIdx.x; i < n; i += (long)NBF * 256)
        x[col + i] = cadd(x[col + i], cmul(alpha, d[i]));
}

BatchCfg batch_config(const Geometry &g, int K, int width, int extent, int small_G, int target_tiles) {
    BatchCfg c;
    c.NWT = (extent + width - 1) / width;
    c.G = g.Nx >= 512 ? 8 : small_G;
    c.NG = (g.Nx + c.G - 1) / c.G;
    c.P = c.NWT * c.NG;
    c.red = c.P <= kBatchRedMaxSlots ? 1 : 0;
    long nch = target_tiles / ((long)K * c.NWT);
    if (nch > c.NG) nch = c.NG;
    if (nch < 1) nch = 1;
    const int m = (int)((c.NG + nch - 1) / nch);  // granules per tile
    c.xchunk = m * c.G;
    c.NCH = (g.Nx + c.xchunk - 1) / c.xchunk;
    const long nb = (g.V + 255) / 256;
    c.NB0 = (int)(nb < 1024 ? nb : 1024);
    c.pstride = 6L * c.P > 2L * c.NB0 ? 6L * c.P : 2L * c.NB0;  // partials by pass parity / the start's
    return c;
}

BatchCfg cg_batch_config(const Geometry &g, int K, int target_tiles) {
    return batch_config(g, K, BW, g.Wt, 1, target_tiles < 1 ? kBatchTargetTiles : target_tiles);
}

void launch_batch_apply(hipStream_t s, const Geometry &g, int K, int dagger, const double2 *in, double2 *out,
                        const BatchLinks &l) {
    const dim3 grid((unsigned)((g.V + 255) / 256), (unsigned)K);
    if (dagger) hipLaunchKernelGGL(batch_apply_kernel<1>, grid, dim3(256), 0, s, g.Nx, g.Wt, g.V, in, l, out);
    else hipLaunchKernelGGL(batch_apply_kernel<0>, grid, dim3(256), 0, s, g.Nx, g.Wt, g.V, in, l, out);
}

void launch_cg_batch_init(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *phi, double2 *x,
                          double2 *T, double2 *d0, const BatchLinks &l, double tol, int max_iter, double2 *partials,
                          CGScalars *sc) {
    launch_batch_apply(s, g, K, 1, phi, T, l);
    hipLaunchKernelGGL(batch_init_kernel, dim3(K * c.NB0), dim3(256), 0, s, c.NB0, g.Nx, g.Wt, g.V, phi, T, l, x, d0,
                       partials, c.pstride);
    launch_batch_init_scalars(s, c, K, partials, sc, tol, max_iter);
}

void launch_cg_batch_pass(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *dold,
                          const double2 *rold, const double2 *aold, double2 *dnew, double2 *anew, double2 *x,
                          const BatchLinks &l, long pass, CGScalars *sc, double2 *partials) {
    CGBArgs a;
    a.dold = dold; a.rold = rold; a.aold = aold;
    a.dnew = dnew; a.anew = anew;
    a.x = x; a.U = l.U; a.ustride = l.ustride; a.massv = l.massv;
    a.V = g.V; a.Nx = g.Nx; a.Wt = g.Wt;
    a.mass = l.mass;
    void (*const kern[2][2])(CGBArgs) = {{cg_batch_kernel<0, 0>, cg_batch_kernel<0, 1>},
                                         {cg_batch_kernel<1, 0>, cg_batch_kernel<1, 1>}};
    launch_batch_pass(s, c, K, pass, sc, partials, a, kern);
}

void launch_batch_scalars(hipStream_t s, const BatchCfg &c, int K, const double2 *partials, CGScalars *sc, long pass) {
    hipLaunchKernelGGL(batch_scalar_kernel, dim3(K), dim3(256), 0, s, c.P, partials, c.pstride, sc, pass == 0 ? 1 : 0);
}

void launch_batch_flush(hipStream_t s, const BatchCfg &c, int K, const double2 *partials, CGScalars *sc, long pass) {
    if (!c.red) return;  // the scalar kernel has already evaluated the pass
    hipLaunchKernelGGL(batch_flush_kernel, dim3(K), dim3(64), 0, s, c.P, partials + (pass & 1) * 3L * c.P, c.pstride,
                       sc, pass);
}

void launch_batch_init_scalars(hipStream_t s, const BatchCfg &c, int K, const double2 *partials, CGScalars *sc,
                               double tol, int max_iter) {
    hipLaunchKernelGGL(batch_init_scalars_kernel, dim3(K), dim3(256), 0, s, c.NB0, partials, c.pstride, sc, tol,
                       max_iter);
}

void launch_batch_finish_x(hipStream_t s, int K, long n, double2 *x, const double2 *d0, const double2 *d1,
                           const double2 *d2, const CGScalars *sc) {
    const long nb = (n + 255) / 256;
    const int NBF = (int)(nb < 256 ? nb : 256);
    hipLaunchKernelGGL(batch_finish_x_kernel, dim3(K * NBF), dim3(256), 0, s, NBF, n, x, d0, d1, d2, sc);
}

// ---- pion correlator -------------------------------------------------------
// Column 2 s + a of phi (zeroed by the caller) = the unit vector at site
// (src_x[s], src_t[s]) of plane a.
__global__ void point_sources_kernel(int K, int Wt, long V, const int *sx, const int *st, double2 *phi) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int s = k >> 1, al = k & 1;
    phi[(long)k * 2 * V + (long)al * V + (long)sx[s] * Wt + st[s]] = make_double2(1.0, 0.0);
}

void launch_point_sources(hipStream_t s, const Geometry &g, int K, const int *sx, const int *st, double2 *phi) {
    hipLaunchKernelGGL(point_sources_kernel, dim3((K + 63) / 64), dim3(64), 0, s, K, g.Wt, g.V, sx, st, phi);
}

// C[s * Wt + t] = sum_x sum_a (|S_a,0(x,t)|^2 + |S_a,1(x,t)|^2), S_a = column
// 2 s + a of S. Block (64 t-values, 4 x-groups): thread (tl, xg) sums rows
// xg, xg + 4, ... in that order, a = 0 then 1, plane 0 then 1; the four groups
// are then added in order. No atomics: the same bits on every call.
__global__ void __launch_bounds__(256) pion_slices_kernel(int Nx, int Wt, long V, const double2 *S, double *C) {
    __shared__ double sh[4][64];
    const int tl = threadIdx.x & 63, xg = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl;
    const int s = blockIdx.y;
    double acc = 0.0;
    if (t < Wt) {
        const double2 *S0 = S + (long)(2 * s) * 2 * V + t, *S1 = S0 + 2 * V;
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
    if (xg == 0 && t < Wt) C[(long)s * Wt + t] = ((sh[0][tl] + sh[1][tl]) + sh[2][tl]) + sh[3][tl];
}

void launch_pion_slices(hipStream_t s, const Geometry &g, int nsrc, const double2 *S, double *C) {
    hipLaunchKernelGGL(pion_slices_kernel, dim3((g.Wt + 63) / 64, nsrc), dim3(256), 0, s, g.Nx, g.Wt, g.V, S, C);
}

}  // namespace sm
