// sm_eomp.cpp -- mixed-precision CG on Dhat Dhat^dagger (the even-odd
// action's solver): fp32 inner iterations (sm_eosp.hip, the stored-Ad one-pass
// kernel on half-lattice vectors) held to the fp64 stop test by reliable
// updates. The scheme and its driver are sm_cg_host.h's cg_mixed_drive, which
// this solver enters as one column (MixedColumn); here are the even-odd
// operations for it: the true residual through eo_dhat, the
// fp32 pass with its two Ad buffers, the fold (which adds alpha_{J-1} d_{J-1}
// after an odd last pass J) and eo_cg as the finish.
//
// One-shard contexts only (sm_eo_cg_precision refuses the others). The fp32
// side owns everything it writes: directions, Ad, y, links, partials, scalars
// and the fp64 work vectors of the true residual. The fp64 even-odd vectors
// are used only by the fp64 code itself (eo_dhat's scratch, the fallback's
// eo_cg), which overwrites them at every start.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

// The mode's buffers, at the first mixed even-odd solve; the fp32 links again
// after every change of U (from the checkerboard links eo_ready just made).
static int eo_mixed_ready(sm_ctx *c) {
    MixedWs &w = c->eomp;
    const size_t n = (size_t)c->g.V;  // complex entries of a one-parity field
    if (BufGroup &b = w.bufs; b.empty()) {
        for (float2 *&d : w.d) TRY(b.add(&d, n, BufKind::streamed, "direction buffer"));
        for (float2 *&a : w.a) TRY(b.add(&a, n, BufKind::streamed, "Ad buffer"));
        for (float2 *&u : w.U) TRY(b.add(&u, n, BufKind::streamed, "links"));
        TRY(b.add(&w.y, n, BufKind::streamed, "correction"));
        TRY(b.add(&w.w, 3 * n, BufKind::device, "fp64 work vectors"));
        TRY(b.add(&w.partials, 2 * (size_t)kMaxPartials, BufKind::device, "partials"));
        TRY(b.add(&w.h_sc, 1, BufKind::pinned, "pinned scalars"));
        TRY(b.add(&w.sc, 1, BufKind::device, "scalars"));
        HIP_TRY(hipMemsetAsync(w.sc, 0, sizeof(MPScalars), c->stream));
        launch_mp_zero(c->stream, (long)n, w.y);
        w.U_valid = false;
    }
    if (!w.U_valid) {
        launch_eo_sp_convert_links(c->stream, c->g, eo_links(c, 0), eo_links(c, 1), w.U[0], w.U[1]);
        w.U_valid = true;
    }
    HIP_TRY(hipGetLastError());
    return SM_OK;
}

namespace {
struct EoOps : MixedDev {
    EoTdCfg cfg;
    int ntiles;
    double mass;
    int true_residual(const double2 *x, double2 *r, bool init, bool restart) {
        double2 *t = w.w + n, *Ax = w.w + 2 * n;
        TRY(eo_dhat(c, 1, x, t, mass));
        TRY(eo_dhat(c, 0, t, Ax, mass));
        return residual(Ax, r, init, restart);
    }
    void pass(long j, const float2 *d1, const float2 *d2, float2 *dn) {  // pass 0 reads no Ad
        launch_eo_sp(c->stream, c->g, cfg, d1, d2, w.a[(j + 1) & 1], dn, w.a[j & 1], w.y, w.U[0], w.U[1], mass, j, w.sc,
                     w.partials);
        launch_cg_sp_scalars(c->stream, ntiles, w.partials, w.sc, j == 0);
    }
    void fold(double2 *x, const float2 *dlast, int discard) { launch_eo_mp_fold(c->stream, n, x, w.y, dlast, w.sc, discard); }
    int solve64(const double2 *rhs, double2 *e, double tol64, int iters, sm_cg_result *r64) {
        return eo_cg(c, rhs, e, mass, tol64, iters, r64);
    }
};
}  // namespace

// b, x: even vectors on the device (x may be b); eo_ready has run for the current U.
int eo_cg_mixed(sm_ctx *c, const double2 *phi, double2 *x, double mass, double tol, int max_iter, sm_cg_result *res) {
    if (c->sharded() || c->peer) return fail(SM_ERR_STATE, "the mixed-precision even-odd CG runs on one-shard contexts");
    const EoTdCfg cfg = eo_td_config(c->g);
    const int ntiles = eo_td_blocks(cfg);
    if (ntiles > kMaxPartials) return fail(SM_ERR_ARG, "too many tiles for the mixed-precision even-odd pass");
    TRY(eo_mixed_ready(c));
    EoOps ops{{c, c->eomp, c->g.V, phi, tol, max_iter, "sm eo_cg mixed",
               "mixed-precision even-odd CG: the segment did not end at max_iter"},
              cfg, ntiles, mass};
    return cg_mixed_drive(ops, phi, x, c->eomp.w, res);  // r: the first of the three work vectors
}

}  // namespace sm_host
