// sm_cgmp.cpp -- mixed-precision CG on D D^dagger: fp32 inner iterations
// (sm_cgsp.hip, two-direction passes) held to the fp64 stop test by reliable
// updates. The scheme and its driver are sm_cg_host.h's cg_mixed_drive, which
// this solver enters as one column (MixedColumn); here are the full lattice's
// operations for it: the true residual through the existing fp64 apply, the
// fp32 pass, the fold and cg_dev_fp64 as the finish.
//
// One-shard contexts only (sm_cg_precision refuses the others). Everything the
// fp32 side touches is its own -- directions, y, links, partials, scalars --
// so the fp64 paths find their state as they left it.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

// The fp32 buffers, at the first mixed solve (placed like the fp64 pass's
// streamed buffers); the fp32 links again after every change of U.
static int mixed_ready(sm_ctx *c) {
    MixedWs &w = c->mp;
    const size_t n = 2 * (size_t)c->g.V;
    if (BufGroup &b = w.bufs; b.empty()) {
        for (float2 *&d : w.d) TRY(b.add(&d, n, BufKind::streamed, "direction buffer"));
        TRY(b.add(&w.y, n, BufKind::streamed, "correction"));
        TRY(b.add(&w.U[0], n, BufKind::streamed, "links"));
        TRY(b.add(&w.partials, 2 * (size_t)kMaxPartials, BufKind::device, "partials"));
        TRY(b.add(&w.h_sc, 1, BufKind::pinned, "pinned scalars"));
        TRY(b.add(&w.sc, 1, BufKind::device, "scalars"));
        HIP_TRY(hipMemsetAsync(w.sc, 0, sizeof(MPScalars), c->stream));
        launch_mp_zero(c->stream, 2 * c->g.V, w.y);
        w.U_valid = false;
    }
    if (!w.U_valid) {
        launch_sp_convert_links(c->stream, c->g, c->U, w.U[0]);
        w.U_valid = true;
    }
    HIP_TRY(hipGetLastError());
    return SM_OK;
}

namespace {
struct FullOps : MixedDev {
    CGFusedCfg cfg;
    int ntiles;
    double m0;
    double mass = m0 + 2;
    int true_residual(const double2 *x, double2 *r, bool init, bool restart) {
        double2 *t = c->field(F_T), *Ax = c->field(F_AD);
        TRY(apply(c, x, t, mass, 1, nullptr, nullptr, nullptr));
        TRY(apply(c, t, Ax, mass, 0, nullptr, nullptr, nullptr));
        return residual(Ax, r, init, restart);
    }
    void pass(long j, const float2 *d1, const float2 *d2, float2 *dn) {
        launch_cg_sp(c->stream, c->g, cfg, d1, d2, dn, w.y, w.U[0], mass, j, w.sc, w.partials);
        launch_cg_sp_scalars(c->stream, ntiles, w.partials, w.sc, j == 0);
    }
    void fold(double2 *x, const float2 *dlast, int discard) { launch_mp_fold(c->stream, c->g, x, w.y, dlast, w.sc, discard); }
    int solve64(const double2 *rhs, double2 *e, double tol64, int iters, sm_cg_result *r64) {
        return cg_dev_fp64(c, (const double *)rhs, (double *)e, m0, tol64, iters, r64);
    }
};
}  // namespace

int cg_dev_mixed(sm_ctx *c, const double *phi_, double *x_, double m0, double tol, int max_iter, sm_cg_result *res) {
    TRY(check_ready(c));
    if (!phi_ || !x_) return fail(SM_ERR_ARG, "null argument");
    if (c->sharded()) return fail(SM_ERR_STATE, "the mixed-precision CG runs on one-shard contexts");
    const CGFusedCfg cfg = cg_sp_config(c->g, c->racfg);
    const int ntiles = cfg.TBk * cfg.XB;
    if (ntiles > kMaxPartials) return fail(SM_ERR_ARG, "too many tiles for the mixed-precision pass");
    TRY(mixed_ready(c));
    FullOps ops{{c, c->mp, 2 * c->g.V, (const double2 *)phi_, tol, max_iter, "sm cg mixed",
                 "mixed-precision CG: the segment did not end at max_iter"},
                cfg, ntiles, m0};
    // r: F_R (the finish keeps its copy apart: the fp64 solver's own buffers include F_R)
    return cg_mixed_drive(ops, ops.phi, (double2 *)x_, c->field(F_R), res);
}

}  // namespace sm_host
