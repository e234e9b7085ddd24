// sm_pion.cpp -- the pion correlator beyond the context's default path
// (sm_cgbatch.cpp): for every replica of an ensemble in one call
// (sm_ens_pion_correlator), and through the even-odd system (solver 1 there,
// sm_pion_solver = 1 for the context's sm_pion_correlator). Kernels:
// sm_pion.hip, and the batched solvers' own (sm_cgbatch.hip, sm_eobatch.hip).
//
//   ensemble   for each (source s, spin a): ONE batched solve of R columns,
//              column r on replica r's links and mass m0[r] + 2, then the
//              propagator S_a of all R columns, and after spin 1 one slice
//              launch for the R replicas. Solver 0: y = (D D^dag)^-1 phi
//              (cg_batch_solve), S = D^dag y (launch_batch_apply): replica r's
//              bits are sm_pion_correlator's on a lone context with its field.
//              The sources live in e->phi, y in e->x, S_0 in e->chi and S_1 in
//              the solver's first Ad buffer (solver 1: in e->phi), all free
//              between trajectories; new memory is the source coordinates
//              and C on the device.
//   even-odd   pion_eo_propagators: D = m - H/2 split by parity gives
//                  phihat_e = phi_e + (1/2m) H_eo phi_o
//                  X = (Dhat Dhat^dag)^-1 phihat_e,  S_e = Dhat^dag X
//                  S_o = (1/m) phi_o + (1/2m) H_oe S_e
//              with Dhat = m - (1/4m) H_eo H_oe; every stage one launch for all
//              K columns. Everything after the sources is eo_propagators, which
//              the quark loops (sm_loops.cpp) run on noise sources.
//              The ensemble calls it with K = R (its checkerboard
//              links, rebuilt once per measurement, and five of its six
//              half-lattice fields), the context with K = 2 nsrc on the shared
//              links of sm_eo_cg_batch's workspace.
// One-shard contexts, always fp64, synchronous. Nothing of the HMC state (U, its
// backup, momenta, the trajectory's parameters, which every trajectory uploads
// anew) is written; the context's U and solvers are not touched by the
// ensemble's call. Index arithmetic and argument checks: sm_pion_host.h.
#include <hip/hip_runtime.h>

#include <vector>

#include "sm_ctx.h"
#include "sm_ens.h"
#include "sm_internal.h"
#include "sm_pion_host.h"

using namespace sm;

namespace sm_host {

int eo_propagators(sm_ctx *c, const BatchWs &w, int K, double2 *eh, const EoBatchLinks &l, double tol, int max_iter,
                   sm_cg_result *res, double2 *S) {
    const Geometry &g = c->g;
    hipStream_t s = c->stream;
    const size_t hv = (size_t)K * (size_t)g.V;
    // slots: phi_e (later S_o), phi_o, phihat_e (later Dhat^dag's odd work field), X, S_e
    double2 *pe = eh, *po = eh + hv, *ph = eh + 2 * hv, *X = eh + 3 * hv, *Se = eh + 4 * hv;
    launch_eob_hop(s, g, K, 0, 0, 2, po, nullptr, ph, l);  // (1/2m) H_eo phi_o
    launch_pion_eo_add(s, g, K, 0, pe, ph, l);
    HIP_TRY(hipGetLastError());
    TRY(eo_batch_solve(c, w, K, ph, X, l, tol, max_iter, res));
    launch_eob_dhat(s, g, K, 1, X, ph, Se, l);
    double2 *So = pe;
    launch_eob_hop(s, g, K, 0, 1, 2, Se, nullptr, So, l);  // (1/2m) H_oe S_e
    launch_pion_eo_add(s, g, K, 1, po, So, l);
    launch_eob_from_cb(s, g, K, Se, So, S);
    HIP_TRY(hipGetLastError());
    return SM_OK;
}

int pion_eo_propagators(sm_ctx *c, const BatchWs &w, int K, const PionCols &src, double2 *eh, const EoBatchLinks &l,
                        double tol, int max_iter, sm_cg_result *res, double2 *S) {
    const size_t hv = (size_t)K * (size_t)c->g.V;
    HIP_TRY(hipMemsetAsync(eh, 0, sizeof(double2) * 2 * hv, c->stream));
    launch_pion_sources(c->stream, c->g, K, src, nullptr, eh, eh + hv);
    return eo_propagators(c, w, K, eh, l, tol, max_iter, res, S);
}

int pion_eo_ready(sm_ctx *c, int K) {
    TRY(eob_ready(c, K));
    if (c->pn_K < K) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->pn_bufs.release();
        c->pn_K = 0;
        TRY(c->pn_bufs.add(&c->pn_buf, 7 * (size_t)c->g.V * (size_t)K, BufKind::device, "pion correlator fields"));
        c->pn_K = K;
    }
    return SM_OK;
}

int pion_correlator_eo(sm_ctx *c, double m0, double tol, int max_iter, int nsrc, const int *sx, const int *st,
                       double *C, sm_cg_result *res) {
    const int K = 2 * nsrc;
    const Geometry &g = c->g;
    TRY(pion_eo_ready(c, K));
    double2 *Ue = c->eob_U, *Uo = c->eob_U + g.V;
    launch_eob_to_cb(c->stream, g, 1, c->U, Ue, Uo);
    HIP_TRY(hipGetLastError());
    const EoBatchLinks l{Ue, Uo, 0, m0 + 2, nullptr};
    std::vector<sm_cg_result> own((size_t)K);
    c->bt_info.assign((size_t)K, sm_cg_mixed_info{});  // the columns ran fp64
    double2 *S = c->pn_buf + 5 * (size_t)g.V * (size_t)K;
    TRY(pion_eo_propagators(c, c->eob, K, PionCols{sx, st, 0, 0, 1}, c->pn_buf, l, tol, max_iter,
                            res ? res : own.data(), S));
    launch_pion_slices(c->stream, g, nsrc, S, c->bt_C);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(C, c->bt_C, sizeof(double) * (size_t)nsrc * (size_t)g.Wt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

}  // namespace sm_host

using namespace sm_host;

extern "C" {

int sm_pion_solver(sm_ctx *c, int mode, int *mode_out) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    int rc = SM_OK;
    if (mode > 1) rc = fail(SM_ERR_ARG, "pion solver must be 0 (D D^dag) or 1 (even-odd)");
    else if (mode == 1 && (c->sharded() || c->hosted || c->peer || c->nshard != 1))
        rc = fail(SM_ERR_ARG, "the pion correlator's even-odd solve runs on one-shard contexts");
    else if (mode >= 0) c->pion_solver = mode;
    if (mode_out) *mode_out = c->pion_solver;
    return rc;
}

int sm_ens_pion_correlator(sm_ens *e, const double *m0, double tol, int max_iter, int solver, int nsrc,
                           const int *src_x, const int *src_t, double *C, sm_cg_result *res) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    sm_ctx *c = e->c;
    const Geometry &g = c->g;
    int bad = 0;
    switch (sm_pion_host::args_refusal(m0, src_x, src_t, C, solver, nsrc, kBatchMax, max_iter, g.Nx, g.Wt, &bad)) {
    case sm_pion_host::PION_OK: break;
    case sm_pion_host::PION_NULL: return fail(SM_ERR_ARG, "null argument");
    case sm_pion_host::PION_SOLVER:
        return fail(SM_ERR_ARG, "ensemble pion correlator: solver = %d, expected 0 (D D^dag) or 1 (even-odd)", solver);
    case sm_pion_host::PION_NSRC:
        return fail(SM_ERR_ARG, "ensemble pion correlator: nsrc = %d outside 1..%d", nsrc, kBatchMax / 2);
    case sm_pion_host::PION_MAX_ITER: return fail(SM_ERR_ARG, "ensemble pion correlator: max_iter < 0");
    case sm_pion_host::PION_COORD:
        return fail(SM_ERR_ARG, "ensemble pion correlator: source %d at (%d, %d) outside the %d x %d lattice", bad,
                    src_x[bad], src_t[bad], g.Nx, g.Wt);
    case sm_pion_host::PION_CHECKERBOARD:
        return fail(SM_ERR_ARG, "ensemble pion correlator: solver 1 needs even Nx and Nt (%d x %d): an odd periodic "
                    "lattice has no checkerboard", g.Nx, g.Wt);
    }
    TRY(all_have(e));
    HIP_TRY(hipSetDevice(c->device));
    const int R = e->R, Nt = g.Wt;
    if (solver == 1) TRY(eo_fields_ready(e));
    if (BufGroup &b = e->pn_bufs; b.empty()) {
        TRY(b.add(&e->pn_src, (size_t)kBatchMax, BufKind::device, "source coordinates"));
        TRY(b.add(&e->pn_C, (size_t)R * (kBatchMax / 2) * (size_t)Nt, BufKind::device, "correlators"));
    }
    hipStream_t s = c->stream;
    int *sx = e->pn_src, *st = e->pn_src + kBatchMax / 2;
    for (int r = 0; r < R; ++r) e->h_mass[r] = m0[r] + 2;
    HIP_TRY(hipMemcpyAsync(e->massv, e->h_mass, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, s));
    // pageable host memory: the copies have left the caller's arrays when they return
    HIP_TRY(hipMemcpyAsync(sx, src_x, sizeof(int) * (size_t)nsrc, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(st, src_t, sizeof(int) * (size_t)nsrc, hipMemcpyHostToDevice, s));
    const size_t fb = sizeof(double2) * slab_complex(e) * (size_t)R;
    const BatchLinks L = links(e);
    const EoBatchLinks EL = eo_links(e);
    if (solver == 1) launch_eob_to_cb(s, g, R, e->U, e->Ucb, e->Ucb + (size_t)R * g.V);
    HIP_TRY(hipGetLastError());
    std::vector<sm_cg_result> col((size_t)R);
    for (int sidx = 0; sidx < nsrc; ++sidx) {
        for (int a = 0; a < 2; ++a) {
            const PionCols src{sx, st, sidx, a, 0};
            double2 *S = a == 0 ? e->chi : (solver == 1 ? e->phi : e->ws.a[0]);
            if (solver == 1) {
                TRY(pion_eo_propagators(c, e->eows, R, src, e->eh, EL, tol, max_iter, col.data(), S));
            } else {
                HIP_TRY(hipMemsetAsync(e->phi, 0, fb, s));
                launch_pion_sources(s, g, R, src, e->phi, nullptr, nullptr);
                HIP_TRY(hipGetLastError());
                TRY(cg_batch_solve(c, e->ws, R, e->phi, e->x, L, tol, max_iter, col.data()));
                launch_batch_apply(s, g, R, 1, e->x, S, L);  // S = D^dag y; the Ad buffer is free after the solve
            }
            if (res)
                for (int r = 0; r < R; ++r) res[sm_pion_host::res_index(nsrc, r, sidx, a)] = col[(size_t)r];
            if (a == 1)
                launch_ens_pion_slices(s, g, R, e->chi, S, e->pn_C + (size_t)sidx * Nt, (long)nsrc * Nt);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipMemcpyAsync(C, e->pn_C, sizeof(double) * (size_t)R * (size_t)nsrc * (size_t)Nt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SM_OK;
}

}  // extern "C"
