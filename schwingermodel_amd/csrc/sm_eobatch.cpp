// sm_eobatch.cpp -- batched one-pass even-odd CG: K half-lattice systems
// Dhat Dhat^dag x_b = phi_b, one launch per iteration for all of them (kernels
// in sm_eobatch.hip), and sm_eo_cg_batch(_dev) on the context's gauge field.
//
//   start   x_b = phi_b, r_0 = phi_b - Dhat Dhat^dag phi_b, d_0 = r_0, the
//           column's scalars (6 launches for the whole batch)
//   pass j  sm_eotd.hip's iteration of every column that is not done, column b
//           with its own links, mass, alpha, beta, stop test and partials
//   finish  x_b += alpha_{k-1} d_{k-1} where column b's iteration count is odd
// The host of these steps is sm_ctx.h's batch_cg_solve, shared with
// sm_cgbatch.cpp; eo_batch_solve below hands it this operator's two launchers.
//
// One-shard contexts, always fp64: none of the precision switches reaches it.
// The workspace (a BatchWs of V complex per column: three direction and two Ad
// buffers on the half lattice, partials, scalars; batch_ws_alloc in
// sm_cgbatch.cpp) is its own and is allocated at first use; the entry
// points add the checkerboard copy of c->U and the columns' even parts. Nothing
// is shared with the context's even-odd solver (c->eo, c->Ucb), the mixed
// solvers, sm_cg_batch or the stepwise solver. The checkerboard links are
// rebuilt from c->U at every call and nothing derived from the gauge field is
// kept, so uploads and HMC trajectories between two solves need no call.

#include <hip/hip_runtime.h>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

int eo_batch_solve(sm_ctx *c, const BatchWs &w, int K, const double2 *phi, double2 *x, const EoBatchLinks &l,
                   double tol, int max_iter, sm_cg_result *res) {
    const BatchCfg cfg = eo_batch_config(c->g, K, c->eob_tiles);
    return batch_cg_solve(
        c, w, cfg, K, x, tol, max_iter, res, "sm eo cg batch",
        [&](auto dbuf) {  // the start's work fields are free until pass 0 writes them; d_0 goes where pass 0 expects d_{-1}
            launch_eo_batch_init(c->stream, c->g, cfg, K, phi, x, w.a[0], w.a[1], dbuf(0), dbuf(-1), l, tol, max_iter,
                                 w.partials, w.sc);
        },
        [&](long j, const double2 *d1, const double2 *d2, const double2 *aold, double2 *dn, double2 *anew) {
            launch_eo_batch_pass(c->stream, c->g, cfg, K, d1, d2, aold, dn, anew, x, l, j, w.sc, w.partials);
        });
}

// The context's own workspace and half-lattice staging: kept while K fits, regrown else.
int eob_ready(sm_ctx *c, int K) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->eob.K < K)
        TRY(batch_ws_alloc(c, c->eob, K, c->g.V, eo_batch_config(c->g, K, c->eob_tiles).pstride));
    if (c->eob_U_bufs.empty())
        TRY(c->eob_U_bufs.add(&c->eob_U, 2 * (size_t)c->g.V, BufKind::device, "checkerboard links"));
    if (c->eob_K >= K) return SM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    BufGroup &b = c->eob_half_bufs;
    b.release();
    c->eob_K = 0;
    const size_t hn = (size_t)c->g.V * (size_t)K;
    TRY(b.add(&c->eob_phi, hn, BufKind::device, "even sources"));
    TRY(b.add(&c->eob_x, hn, BufKind::device, "even solutions"));
    c->eob_K = K;
    return SM_OK;
}

// Full-layout device staging of the host-pointer entry: phi and x, K columns.
static int eob_staging_ready(sm_ctx *c, int K) {
    if (c->eob_fK >= K) return SM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    BufGroup &b = c->eob_full_bufs;
    b.release();
    c->eob_fK = 0;
    const size_t fn = 2 * (size_t)c->g.V * (size_t)K;
    TRY(b.add(&c->eob_fphi, fn, BufKind::device, "sources"));
    TRY(b.add(&c->eob_fx, fn, BufKind::device, "solutions"));
    c->eob_fK = K;
    return SM_OK;
}

static int eob_check(sm_ctx *c, int K, const void *phi, const void *x, const void *res, int max_iter) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    if (c->sharded() || c->hosted || c->peer || c->nshard != 1)
        return fail(SM_ERR_ARG,
                    "the batched even-odd CG runs on one-shard contexts (no loopback, peer or host-staged transport)");
    if (K < 1 || K > kBatchMax) return fail(SM_ERR_ARG, "batched even-odd CG: K = %d outside 1..%d", K, kBatchMax);
    if (!phi || !x || !res) return fail(SM_ERR_ARG, "null argument");
    if (x == phi) return fail(SM_ERR_ARG, "batched even-odd CG: x must not alias phi");
    if (max_iter < 0) return fail(SM_ERR_ARG, "batched even-odd CG: max_iter < 0");
    if (c->g.Nx % 2 || c->g.Wt % 2)
        return fail(SM_ERR_ARG, "batched even-odd CG: the checkerboard needs even Nx and Nt (%d x %d)", c->g.Nx,
                    c->g.Wt);
    return check_ready(c);
}

// K full-layout device columns: even parts in, the solve, (x_e, 0) out.
static int eob_solve_full(sm_ctx *c, int K, const double2 *phi, double2 *x, double m0, double tol, int max_iter,
                          sm_cg_result *res) {
    TRY(eob_ready(c, K));
    double2 *Ue = c->eob_U, *Uo = c->eob_U + c->g.V;
    launch_eob_to_cb(c->stream, c->g, 1, c->U, Ue, Uo);
    launch_eob_to_cb(c->stream, c->g, K, phi, c->eob_phi, nullptr);
    HIP_TRY(hipGetLastError());
    const EoBatchLinks l{Ue, Uo, 0, m0 + 2, nullptr};
    TRY(eo_batch_solve(c, c->eob, K, c->eob_phi, c->eob_x, l, tol, max_iter, res));
    launch_eob_from_cb(c->stream, c->g, K, c->eob_x, nullptr, x);
    HIP_TRY(hipGetLastError());
    return SM_OK;
}

}  // namespace sm_host

using namespace sm_host;

extern "C" {

int sm_eo_cg_batch_dev(sm_ctx *c, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                       sm_cg_result *res) {
    TRY(eob_check(c, K, phi, x, res, max_iter));
    TRY(eob_solve_full(c, K, (const double2 *)phi, (double2 *)x, m0, tol, max_iter, res));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

int sm_eo_cg_batch(sm_ctx *c, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                   sm_cg_result *res) {
    TRY(eob_check(c, K, phi, x, res, max_iter));
    HIP_TRY(hipSetDevice(c->device));
    TRY(eob_staging_ready(c, K));
    const size_t fb = sizeof(double2) * 2 * (size_t)c->g.V * (size_t)K;
    HIP_TRY(hipMemcpyAsync(c->eob_fphi, phi, fb, hipMemcpyHostToDevice, c->stream));
    TRY(eob_solve_full(c, K, c->eob_fphi, c->eob_fx, m0, tol, max_iter, res));
    HIP_TRY(hipMemcpyAsync(x, c->eob_fx, fb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

}  // extern "C"
