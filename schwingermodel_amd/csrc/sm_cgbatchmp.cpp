// sm_cgbatchmp.cpp -- mixed-precision batched CG on D D^dagger: fp32 inner
// iterations for K columns in one launch per pass (sm_cgbatchsp.hip) held to
// the fp64 stop test, column by column, by reliable updates. The scheme and its
// driver are sm_cg_host.h's cg_mixed_drive, the one the one-column solvers
// enter with K = 1; here are the batch's operations for it: the true residual
// through two launch_batch_apply, the fp32 pass, the injection into the ring's
// fixed slots, the fold, and the fp64 batched solver with K = 1 as a column's
// finish.
//
// One-shard contexts only (sm_cg_batch_precision refuses the others).
// Everything the fp32 side touches is its own (btmp of sm_ctx), so the fp64
// batch, the ensemble and the other solvers find their state as they left it;
// the finish runs on the fp64 batch's workspace, which keeps nothing between
// solves. The fp32 links are converted from c->U at the start of every solve:
// nothing derived from the gauge field is kept here either.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

static size_t partials_per_column(const sm_ctx *c) {
    const BatchCfg cfg = cg_batch_config(c->g, 1, c->bt_tiles);  // P does not depend on K
    const size_t nbr = (size_t)batch_mp_blocks(c->g);
    return 2 * (size_t)cfg.P > nbr ? 2 * (size_t)cfg.P : nbr;
}

// The workspace for K columns: kept while K fits, regrown else.
static int mixed_ready(sm_ctx *c, int K) {
    CGBatchMixedWs &w = c->btmp;
    if (w.K >= K) return SM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    BufGroup &b = w.bufs;
    b.release();
    w.K = 0;
    const size_t n = 2 * (size_t)c->g.V, nK = n * (size_t)K, f32 = sizeof(float2) * nK;
    const size_t pn = partials_per_column(c) * (size_t)K, pb = sizeof(double2) * pn, sb = sizeof(MPScalars) * (size_t)K;
    for (float2 *&d : w.d) TRY(b.add(&d, nK, BufKind::device, "direction buffer"));
    for (float2 *&a : w.a) TRY(b.add(&a, nK, BufKind::device, "Ad buffer"));
    TRY(b.add(&w.y, nK, BufKind::device, "correction"));
    TRY(b.add(&w.U, n, BufKind::device, "links"));
    TRY(b.add(&w.r, nK, BufKind::device, "residual"));
    TRY(b.add(&w.t, nK, BufKind::device, "D^dag x"));
    TRY(b.add(&w.ax, nK, BufKind::device, "D D^dag x"));
    TRY(b.add(&w.partials, pn, BufKind::device, "partials"));
    TRY(b.add(&w.sc, (size_t)K, BufKind::device, "scalars"));
    TRY(b.add(&w.h_sc, (size_t)K, BufKind::pinned, "pinned scalars"));
    // the passes' halo lanes and rows read every buffer before its first write: defined values
    for (float2 *d : w.d) HIP_TRY(hipMemsetAsync(d, 0, f32, c->stream));
    for (float2 *a : w.a) HIP_TRY(hipMemsetAsync(a, 0, f32, c->stream));
    HIP_TRY(hipMemsetAsync(w.y, 0, f32, c->stream));
    HIP_TRY(hipMemsetAsync(w.partials, 0, pb, c->stream));
    HIP_TRY(hipMemsetAsync(w.sc, 0, sb, c->stream));
    w.K = K;
    return SM_OK;
}

namespace {
struct BatchOps {
    sm_ctx *c;
    CGBatchMixedWs &w;
    int K;
    const double2 *phi;
    double2 *x;
    double m0, tol;
    int max_iter;
    BatchCfg cfg;
    const char *tag = "sm cg batch mixed";
    const char *stuck = "mixed-precision batched CG: a segment did not end at max_iter";
    double delta = c->mp_delta;
    int force_fallback = c->mp_force_fallback, debug = c->debug_cg;
    long n = 2 * c->g.V;  // complex entries of a column
    BatchLinks links = shared_links(c->U, m0 + 2);

    const MPScalars &h(int b) const { return w.h_sc[b]; }
    sm_cg_mixed_info &info(int b) { return c->bt_info[(size_t)b]; }
    void start() { launch_copy(c->stream, n * K, phi, x); }
    int check() {
        HIP_TRY(hipGetLastError());
        return SM_OK;
    }
    int read() {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w.h_sc, w.sc, sizeof(MPScalars) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SM_OK;
    }
    int true_residual(ColMask m, bool init, bool restart) {
        if ((m & (m - 1)) == 0 && K > 1) {  // one column (a finish's): apply to that column alone
            int b = 0;
            while (!(m >> b & 1)) ++b;
            launch_batch_apply(c->stream, c->g, 1, 1, x + b * n, w.t + b * n, links);
            launch_batch_apply(c->stream, c->g, 1, 0, w.t + b * n, w.ax + b * n, links);
        } else {
            launch_batch_apply(c->stream, c->g, K, 1, x, w.t, links);
            launch_batch_apply(c->stream, c->g, K, 0, w.t, w.ax, links);
        }
        launch_batch_mp_residual(c->stream, c->g, K, m, phi, w.ax, w.r, w.partials, w.sc, init ? 1 : 0, restart ? 1 : 0,
                                 tol, delta, max_iter);
        return read();
    }
    void inject(ColMask m) { launch_batch_mp_inject(c->stream, c->g, K, m, w.r, w.d, w.sc); }
    void pass(long j, ColMask m) {
        launch_cg_batch_sp(c->stream, c->g, cfg, K, m, w.d, w.a, w.y, w.U, m0 + 2, j, w.sc, w.partials);
    }
    void fold(ColMask m, ColMask discard) { launch_batch_mp_fold(c->stream, c->g, K, m, discard, x, w.y, w.d, w.sc); }
    // A e = r_b through the fp64 batched solver with K = 1 (its own x0 = r convention), x_b += e
    int finish(int b, double tol64, int iters, sm_cg_result *r64) {
        if (c->bt.K < 1) TRY(batch_ws_alloc(c, c->bt, 1, n, cg_batch_config(c->g, 1, c->bt_tiles).pstride));
        double2 *e = w.t + b * n;
        TRY(cg_batch_solve(c, c->bt, 1, w.r + b * n, e, links, tol64, iters, r64));
        launch_mp_add(c->stream, n, x + b * n, e);
        return check();
    }
};
}  // namespace

int cg_batch_mixed(sm_ctx *c, int K, const double2 *phi, double2 *x, double m0, double tol, int max_iter,
                   sm_cg_result *res) {
    if (c->sharded() || c->hosted || c->peer)
        return fail(SM_ERR_STATE, "the mixed-precision batched CG runs on one-shard contexts");
    HIP_TRY(hipSetDevice(c->device));
    TRY(mixed_ready(c, K));
    launch_sp_convert_links(c->stream, c->g, c->U, c->btmp.U);
    HIP_TRY(hipGetLastError());
    BatchOps ops{c, c->btmp, K, phi, x, m0, tol, max_iter, cg_batch_config(c->g, K, c->bt_tiles)};
    return cg_mixed_drive(ops, K, res);
}

}  // namespace sm_host

using namespace sm_host;

extern "C" {

int sm_cg_batch_precision(sm_ctx *c, int mode, int *mode_out) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    int rc = SM_OK;
    if (mode > 1) rc = fail(SM_ERR_ARG, "batched CG precision must be 0 (fp64) or 1 (mixed)");
    else if (mode == 1 && (c->sharded() || c->hosted || c->peer || c->nshard != 1))
        rc = fail(SM_ERR_ARG, "the mixed-precision batched CG runs on one-shard contexts");
    else if (mode >= 0) c->bt_precision = mode;
    if (mode_out) *mode_out = c->bt_precision;
    return rc;
}

int sm_cg_batch_mixed_last(const sm_ctx *c, int K, sm_cg_mixed_info *out) {
    if (!c || !out) return fail(SM_ERR_ARG, "null argument");
    if (K < 1 || (size_t)K != c->bt_info.size())
        return fail(SM_ERR_ARG, "the context's last batched solve had %zu columns, not %d", c->bt_info.size(), K);
    for (int b = 0; b < K; ++b) out[b] = c->bt_info[(size_t)b];
    return SM_OK;
}

}  // extern "C"
