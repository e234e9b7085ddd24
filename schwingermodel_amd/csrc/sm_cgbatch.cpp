// sm_cgbatch.cpp -- batched multi-source CG on D D^dagger (K right-hand sides
// on the context's gauge field, one launch per iteration; kernels in
// sm_cgbatch.hip) and the pion correlator built on it.
//
//   start   x_b = phi_b, r_0 = phi_b - D D^dag phi_b, d_0 = r_0, the column's
//           scalars (3 launches for the whole batch)
//   pass j  the stored-Ad two-direction iteration of every column that is not
//           done, column b with its own alpha, beta, stop test and partials
//   finish  x_b += alpha_{k-1} d_{k-1} where column b's iteration count is odd
// The host of these steps is sm_ctx.h's batch_cg_solve, which the even-odd
// solver (sm_eobatch.cpp) runs too: cg_batch_solve below hands it this
// operator's two launchers. The workspace of both solvers (batch_ws_alloc,
// batch_ws_free) is defined here; its buffers, like the staging's and the
// correlator's, belong to BufGroups (sm_buf.h) that sm_ctx holds.
//
// One-shard contexts only. fp64 unless sm_cg_batch_precision switched the entry
// points below to the mixed-precision solver (sm_cgbatchmp.cpp), which shares
// nothing with this one; sm_cg_precision does not reach either.
// Everything it writes is its own (bt_* of sm_ctx): the stepwise solver, the
// one behind sm_cg_dev, the mixed and the even-odd solvers find their buffers
// and scalars as they left them. The gauge field is read from c->U at every
// call and nothing derived from it is kept, so uploads and HMC trajectories
// between two batched solves need no call.
// sm_pion_solver = 1 hands sm_pion_correlator's body to the even-odd path of
// sm_pion.cpp after the argument checks; mode 0 is the code below.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

void batch_ws_free(BatchWs &w) {
    w.bufs.release();
    w.K = 0;
    w.n = 0;
}

// Three d buffers, two Ad buffers (K x 16 n bytes each), partials and scalars.
int batch_ws_alloc(sm_ctx *c, BatchWs &w, int K, long n, long pstride) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    batch_ws_free(w);
    const size_t fn = (size_t)n * (size_t)K, fb = sizeof(double2) * fn;
    const size_t pn = (size_t)pstride * (size_t)K, pb = sizeof(double2) * pn;
    BufGroup &b = w.bufs;
    for (double2 *&d : w.d) TRY(b.add(&d, fn, BufKind::device, "direction buffer"));
    for (double2 *&a : w.a) TRY(b.add(&a, fn, BufKind::device, "Ad buffer"));
    TRY(b.add(&w.partials, pn, BufKind::device, "partials"));
    TRY(b.add(&w.sc, (size_t)K, BufKind::device, "scalars"));
    TRY(b.add(&w.h_sc, (size_t)K, BufKind::pinned, "pinned scalars"));
    // every buffer is read by halo lanes / rows before its first write: defined values
    for (double2 *d : w.d) HIP_TRY(hipMemsetAsync(d, 0, fb, c->stream));
    for (double2 *a : w.a) HIP_TRY(hipMemsetAsync(a, 0, fb, c->stream));
    HIP_TRY(hipMemsetAsync(w.partials, 0, pb, c->stream));
    HIP_TRY(hipMemsetAsync(w.sc, 0, sizeof(CGScalars) * (size_t)K, c->stream));
    w.K = K;
    w.n = n;
    return SM_OK;
}

// The context's own workspace: kept while K fits, regrown else.
static int batch_ready(sm_ctx *c, int K) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->bt.K >= K) return SM_OK;
    return batch_ws_alloc(c, c->bt, K, 2 * c->g.V, cg_batch_config(c->g, K, c->bt_tiles).pstride);
}

// Device staging for the host-pointer entry and the correlator: phi and x, K columns.
int batch_staging_ready(sm_ctx *c, int K) {
    if (c->bt_pion_K >= K) return SM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    BufGroup &b = c->bt_stage_bufs;
    b.release();
    c->bt_pion_K = 0;
    const size_t fn = 2 * (size_t)c->g.V * (size_t)K;
    TRY(b.add(&c->bt_phi, fn, BufKind::device, "sources"));
    TRY(b.add(&c->bt_x, fn, BufKind::device, "solutions"));
    c->bt_pion_K = K;
    return SM_OK;
}

static int batch_check(sm_ctx *c, int K) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    if (c->sharded() || c->hosted || c->peer || c->nshard != 1)
        return fail(SM_ERR_ARG, "the batched CG runs on one-shard contexts (no loopback, peer or host-staged transport)");
    if (K < 1 || K > kBatchMax) return fail(SM_ERR_ARG, "batched CG: K = %d outside 1..%d", K, kBatchMax);
    return SM_OK;
}

int cg_batch_solve(sm_ctx *c, const BatchWs &w, int K, const double2 *phi, double2 *x, const BatchLinks &l,
                   double tol, int max_iter, sm_cg_result *res) {
    const BatchCfg cfg = cg_batch_config(c->g, K, c->bt_tiles);
    return batch_cg_solve(
        c, w, cfg, K, x, tol, max_iter, res, "sm cg batch",
        [&](auto dbuf) {  // d_0 goes where pass 0 expects d_{-1}: it copies it to dbuf(0) while forming Ad_0
            launch_cg_batch_init(c->stream, c->g, cfg, K, phi, x, w.a[0], dbuf(-1), l, tol, max_iter, w.partials, w.sc);
        },
        [&](long j, const double2 *d1, const double2 *d2, const double2 *aold, double2 *dn, double2 *anew) {
            launch_cg_batch_pass(c->stream, c->g, cfg, K, d1, d2, aold, dn, anew, x, l, j, w.sc, w.partials);
        });
}

// Every batched solve of the entry points below: this file's fp64 solver on the
// context's workspace, or the mixed-precision one (sm_cg_batch_precision).
int batch_solve(sm_ctx *c, int K, const double2 *phi, double2 *x, double m0, double tol, int max_iter,
                       sm_cg_result *res) {
    c->bt_info.assign((size_t)K, sm_cg_mixed_info{});
    if (c->bt_precision == 1) return cg_batch_mixed(c, K, phi, x, m0, tol, max_iter, res);
    TRY(batch_ready(c, K));
    return cg_batch_solve(c, c->bt, K, phi, x, shared_links(c->U, m0 + 2), tol, max_iter, res);
}

}  // namespace sm_host

using namespace sm_host;

extern "C" {

int sm_cg_batch_max(void) { return kBatchMax; }

int sm_cg_batch_dev(sm_ctx *c, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                    sm_cg_result *res) {
    TRY(batch_check(c, K));
    if (!phi || !x || !res) return fail(SM_ERR_ARG, "null argument");
    if ((const double *)x == phi) return fail(SM_ERR_ARG, "batched CG: x must not alias phi");
    if (max_iter < 0) return fail(SM_ERR_ARG, "batched CG: max_iter < 0");
    TRY(check_ready(c));
    return batch_solve(c, K, (const double2 *)phi, (double2 *)x, m0, tol, max_iter, res);
}

int sm_cg_batch(sm_ctx *c, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                sm_cg_result *res) {
    TRY(batch_check(c, K));
    if (!phi || !x || !res) return fail(SM_ERR_ARG, "null argument");
    if (max_iter < 0) return fail(SM_ERR_ARG, "batched CG: max_iter < 0");
    TRY(check_ready(c));
    HIP_TRY(hipSetDevice(c->device));
    TRY(batch_staging_ready(c, K));
    const size_t fb = sizeof(double2) * 2 * (size_t)c->g.V * (size_t)K;
    HIP_TRY(hipMemcpyAsync(c->bt_phi, phi, fb, hipMemcpyHostToDevice, c->stream));
    TRY(batch_solve(c, K, c->bt_phi, c->bt_x, m0, tol, max_iter, res));
    HIP_TRY(hipMemcpyAsync(x, c->bt_x, fb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

int sm_pion_correlator(sm_ctx *c, double m0, double tol, int max_iter, int nsrc, const int *src_x, const int *src_t,
                       double *C, sm_cg_result *res) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    if (nsrc < 1 || 2 * (long)nsrc > kBatchMax)
        return fail(SM_ERR_ARG, "pion correlator: nsrc = %d outside 1..%d", nsrc, kBatchMax / 2);
    const int K = 2 * nsrc;
    TRY(batch_check(c, K));
    if (!src_x || !src_t || !C) return fail(SM_ERR_ARG, "null argument");
    if (max_iter < 0) return fail(SM_ERR_ARG, "pion correlator: max_iter < 0");
    for (int s = 0; s < nsrc; ++s)
        if (src_x[s] < 0 || src_x[s] >= c->g.Nx || src_t[s] < 0 || src_t[s] >= c->g.Wt)
            return fail(SM_ERR_ARG, "pion correlator: source %d at (%d, %d) outside the %d x %d lattice", s, src_x[s],
                        src_t[s], c->g.Nx, c->g.Wt);
    const bool eo = c->pion_solver == 1;  // sm_pion_solver: the even-odd path (sm_pion.cpp)
    if (eo && (c->g.Nx % 2 || c->g.Wt % 2))
        return fail(SM_ERR_ARG, "pion correlator: the even-odd solve (sm_pion_solver = 1) needs even Nx and Nt (%d x %d): "
                    "an odd periodic lattice has no checkerboard", c->g.Nx, c->g.Wt);
    TRY(check_ready(c));
    HIP_TRY(hipSetDevice(c->device));
    if (!eo) TRY(batch_staging_ready(c, K));
    if (BufGroup &b = c->bt_corr_bufs; b.empty()) {
        TRY(b.add(&c->bt_src, (size_t)kBatchMax, BufKind::device, "source coordinates"));
        TRY(b.add(&c->bt_C, (kBatchMax / 2) * (size_t)c->g.Wt, BufKind::device, "correlator"));
    }
    const size_t fb = sizeof(double2) * 2 * (size_t)c->g.V * (size_t)K;
    int *sx = c->bt_src, *st = c->bt_src + kBatchMax / 2;
    // pageable host memory: the copies have left the caller's arrays when they return
    HIP_TRY(hipMemcpyAsync(sx, src_x, sizeof(int) * (size_t)nsrc, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(st, src_t, sizeof(int) * (size_t)nsrc, hipMemcpyHostToDevice, c->stream));
    if (eo) return pion_correlator_eo(c, m0, tol, max_iter, nsrc, sx, st, C, res);
    HIP_TRY(hipMemsetAsync(c->bt_phi, 0, fb, c->stream));
    launch_point_sources(c->stream, c->g, K, sx, st, c->bt_phi);
    HIP_TRY(hipGetLastError());
    std::vector<sm_cg_result> own((size_t)K);
    sm_cg_result *r = res ? res : own.data();
    TRY(batch_solve(c, K, c->bt_phi, c->bt_x, m0, tol, max_iter, r));
    // S_a = D^dag y_a (the existing apply) into the solver's first Ad buffer (mixed: its D^dag x), free after the solve
    double2 *S = c->bt_precision == 1 ? c->btmp.t : c->bt.a[0];
    const long n = 2 * c->g.V;
    for (int k = 0; k < K; ++k) TRY(apply(c, c->bt_x + k * n, S + k * n, m0 + 2, 1, nullptr, nullptr, nullptr));
    launch_pion_slices(c->stream, c->g, nsrc, S, c->bt_C);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(C, c->bt_C, sizeof(double) * (size_t)nsrc * (size_t)c->g.Wt, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

}  // extern "C"
