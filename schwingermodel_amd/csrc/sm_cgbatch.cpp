// sm_cgbatch.cpp -- batched multi-source CG on D D^dagger (K right-hand sides
// on the context's gauge field, one launch per iteration; kernels in
// sm_cgbatch.hip) and the pion correlator built on it.
//
//   start   x_b = phi_b, r_0 = phi_b - D D^dag phi_b, d_0 = r_0, the column's
//           scalars (3 launches for the whole batch)
//   pass j  the stored-Ad two-direction iteration of every column that is not
//           done, column b with its own alpha, beta, stop test and partials;
//           passes are enqueued in chunks (CgChunker per column, the longest
//           wish wins) and all K states are read once per chunk
//   finish  x_b += alpha_{k-1} d_{k-1} where column b's iteration count is odd
//
// One-shard contexts only. fp64 unless sm_cg_batch_precision switched the entry
// points below to the mixed-precision solver (sm_cgbatchmp.cpp), which shares
// nothing with this one; sm_cg_precision does not reach either.
// Everything it writes is its own (bt_* of sm_ctx): the stepwise solver, the
// one behind sm_cg_dev, the mixed and the even-odd solvers find their buffers
// and scalars as they left them. The gauge field is read from c->U at every
// call and nothing derived from it is kept, so uploads and HMC trajectories
// between two batched solves need no call.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

static void free_dev(void *p) {
    if (p) (void)hipFree(p);
}

void cg_batch_ws_free(CGBatchWs &w) {
    for (double2 *&d : w.d) {
        free_dev(d);
        d = nullptr;
    }
    for (double2 *&a : w.a) {
        free_dev(a);
        a = nullptr;
    }
    free_dev(w.partials);
    free_dev(w.sc);
    if (w.h_sc) (void)hipHostFree(w.h_sc);
    w.partials = nullptr;
    w.sc = w.h_sc = nullptr;
    w.K = 0;
}

void cg_batch_free(sm_ctx *c) {
    cg_batch_ws_free(c->bt);
    free_dev(c->bt_phi);
    free_dev(c->bt_x);
    free_dev(c->bt_src);
    free_dev(c->bt_C);
    c->bt_phi = c->bt_x = nullptr;
    c->bt_src = nullptr;
    c->bt_C = nullptr;
    c->bt_pion_K = 0;
}

// hipMalloc that reports the request on failure and leaves no sticky error
static int alloc_dev(void **p, size_t bytes, const char *what) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return SM_OK;
    *p = nullptr;
    (void)hipGetLastError();
    return fail(SM_ERR_HIP, "batched CG: allocating %zu bytes (%s) failed: %s", bytes, what, hipGetErrorString(e));
}

// The solver's workspace for K columns: three d buffers, two Ad buffers
// (K x 32 V bytes each), partials and scalars.
int cg_batch_ws_alloc(sm_ctx *c, CGBatchWs &w, int K) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    cg_batch_ws_free(w);
    const size_t fb = sizeof(double2) * 2 * (size_t)c->g.V * (size_t)K;
    const CGBatchCfg cfg = cg_batch_config(c->g, K, c->bt_tiles);  // pstride does not depend on K
    const size_t pb = sizeof(double2) * (size_t)cfg.pstride * (size_t)K;
    int rc = SM_OK;
    for (double2 *&d : w.d)
        if (rc == SM_OK) rc = alloc_dev((void **)&d, fb, "direction buffer");
    for (double2 *&a : w.a)
        if (rc == SM_OK) rc = alloc_dev((void **)&a, fb, "Ad buffer");
    if (rc == SM_OK) rc = alloc_dev((void **)&w.partials, pb, "partials");
    if (rc == SM_OK) rc = alloc_dev((void **)&w.sc, sizeof(CGScalars) * (size_t)K, "scalars");
    if (rc == SM_OK && hipHostMalloc((void **)&w.h_sc, sizeof(CGScalars) * (size_t)K) != hipSuccess) {
        w.h_sc = nullptr;
        (void)hipGetLastError();
        rc = fail(SM_ERR_HIP, "batched CG: allocating %zu pinned bytes (scalars) failed", sizeof(CGScalars) * (size_t)K);
    }
    if (rc != SM_OK) {
        cg_batch_ws_free(w);
        return rc;
    }
    // every buffer is read by halo lanes / rows before its first write: defined values
    for (double2 *d : w.d) HIP_TRY(hipMemsetAsync(d, 0, fb, c->stream));
    for (double2 *a : w.a) HIP_TRY(hipMemsetAsync(a, 0, fb, c->stream));
    HIP_TRY(hipMemsetAsync(w.partials, 0, pb, c->stream));
    HIP_TRY(hipMemsetAsync(w.sc, 0, sizeof(CGScalars) * (size_t)K, c->stream));
    w.K = K;
    return SM_OK;
}

// The context's own workspace: kept while K fits, regrown else.
static int batch_ready(sm_ctx *c, int K) {
    HIP_TRY(hipSetDevice(c->device));
    return c->bt.K >= K ? SM_OK : cg_batch_ws_alloc(c, c->bt, K);
}

// Device staging for the host-pointer entry and the correlator: phi and x, K columns.
static int staging_ready(sm_ctx *c, int K) {
    if (c->bt_pion_K >= K) return SM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_dev(c->bt_phi);
    free_dev(c->bt_x);
    c->bt_phi = c->bt_x = nullptr;
    c->bt_pion_K = 0;
    const size_t fb = sizeof(double2) * 2 * (size_t)c->g.V * (size_t)K;
    int rc = alloc_dev((void **)&c->bt_phi, fb, "sources");
    if (rc == SM_OK) rc = alloc_dev((void **)&c->bt_x, fb, "solutions");
    if (rc != SM_OK) {
        free_dev(c->bt_phi);
        c->bt_phi = nullptr;
        return rc;
    }
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

int cg_batch_solve(sm_ctx *c, const CGBatchWs &w, int K, const double2 *phi, double2 *x, const BatchLinks &l,
                   double tol, int max_iter, sm_cg_result *res) {
    HIP_TRY(hipSetDevice(c->device));
    const CGBatchCfg cfg = cg_batch_config(c->g, K, c->bt_tiles);
    auto dbuf = [&](long i) { return w.d[((i % 3) + 3) % 3]; };
    // d_0 goes where pass 0 expects d_{-1}: it copies it to dbuf(0) while forming Ad_0
    launch_cg_batch_init(c->stream, c->g, cfg, K, phi, x, w.a[0], dbuf(-1), l, tol, max_iter, w.partials, w.sc);
    HIP_TRY(hipGetLastError());
    const long passes = (long)max_iter + 1;  // pass 0 forms Ad_0; a column stops itself at k == max_iter
    std::vector<CgChunker> plan((size_t)K);
    long issued = 0;
    int chunk = 4;
    const CGScalars *h = w.h_sc;
    for (;;) {
        const long nb = passes - issued < chunk ? passes - issued : chunk;
        for (long i = 0; i < nb; ++i, ++issued) {
            const long j = issued;
            launch_cg_batch_pass(c->stream, c->g, cfg, K, dbuf(j - 1), dbuf(j - 2), w.a[(j + 1) & 1], dbuf(j),
                                 w.a[j & 1], x, l, j, w.sc, w.partials);
        }
        if (nb > 0) launch_cg_batch_flush(c->stream, cfg, K, w.partials, w.sc, issued - 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w.h_sc, w.sc, sizeof(CGScalars) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        int open = 0, wish = 2;
        for (int b = 0; b < K; ++b) {
            if (h[b].done) continue;
            ++open;
            const int w = plan[(size_t)b].next(h[b].k, h[b].err, tol * h[b].phi_norm);
            if (w > wish) wish = w;
        }
        if (c->debug_cg) fprintf(stderr, "[sm cg batch] passes %ld open %d of %d next chunk %d\n", issued, open, K, wish);
        if (!open || issued >= passes) break;
        chunk = wish;
    }
    launch_cg_batch_finish_x(c->stream, c->g, K, x, w.d[0], w.d[1], w.d[2], w.sc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int b = 0; b < K; ++b) {
        res[b].converged = h[b].converged;
        res[b].iterations = h[b].k;
        res[b].residual = h[b].err;
        res[b].phi_norm = h[b].phi_norm;
    }
    return SM_OK;
}

// Every batched solve of the entry points below: this file's fp64 solver on the
// context's workspace, or the mixed-precision one (sm_cg_batch_precision).
static int batch_solve(sm_ctx *c, int K, const double2 *phi, double2 *x, double m0, double tol, int max_iter,
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
    TRY(staging_ready(c, K));
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
    TRY(check_ready(c));
    HIP_TRY(hipSetDevice(c->device));
    TRY(staging_ready(c, K));
    if (!c->bt_src) TRY(alloc_dev((void **)&c->bt_src, sizeof(int) * kBatchMax, "source coordinates"));
    if (!c->bt_C) TRY(alloc_dev((void **)&c->bt_C, sizeof(double) * (kBatchMax / 2) * (size_t)c->g.Wt, "correlator"));
    const size_t fb = sizeof(double2) * 2 * (size_t)c->g.V * (size_t)K;
    int *sx = c->bt_src, *st = c->bt_src + kBatchMax / 2;
    // pageable host memory: the copies have left the caller's arrays when they return
    HIP_TRY(hipMemcpyAsync(sx, src_x, sizeof(int) * (size_t)nsrc, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(st, src_t, sizeof(int) * (size_t)nsrc, hipMemcpyHostToDevice, c->stream));
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
