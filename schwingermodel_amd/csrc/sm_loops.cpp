// sm_loops.cpp -- stochastic quark loops: per noise vector k and time slice t
//     S_k(t) = sum_x eta_k^dag D^-1 eta_k,   P_k(t) = sum_x eta_k^dag gamma5 D^-1 eta_k
// whose averages over k estimate Tr_t D^-1 (the chiral condensate) and
// Tr_t gamma5 D^-1 (the disconnected piece of the flavour-singlet correlator).
// For a context's field (sm_quark_loops) and for every replica of an ensemble
// (sm_ens_quark_loops). Kernels: sm_loops.hip, and the batched solvers' own.
//
//   context    the nnoise vectors in chunks of at most kBatchMax columns: the
//              noise into the batched CG's staging (bt_phi), the context's
//              batched solve (batch_solve: fp64, or mixed under
//              sm_cg_batch_precision, as sm_pion_correlator), then ONE
//              contraction launch that forms D^dag y in registers and sums.
//              A column's bits do not depend on its batch (sm_cgbatch.hip), the
//              contraction's order not on K: vector k's loops and report depend
//              on the field, m0, tol, max_iter, seed and k only.
//   ensemble   for each k ONE batched solve of R columns, column r on replica
//              r's links and mass with seed[r], in the ensemble's phi / x and
//              solver workspace, then one contraction launch for all replicas.
//              Replica r's bits are sm_quark_loops' on a lone context.
//   solver 1   the noise on the checkerboard, eo_propagators (sm_pion.cpp: the
//              stage the pion correlator runs after its point sources), then the
//              contraction's load-psi form on the full-layout propagator. The
//              context works in the even-odd batch workspace and pn_buf of
//              sm_pion_solver = 1, the ensemble in its even-odd fields and chi.
// One-shard contexts, synchronous. Nothing of the HMC state is written; new
// memory is the columns' (seed, k) and the loops on the device. Index
// arithmetic and argument checks: sm_loops_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sm_ctx.h"
#include "sm_ens.h"
#include "sm_internal.h"
#include "sm_loops_host.h"

using namespace sm;

using namespace sm_host;

namespace {

constexpr const char *kLoopsWho = "quark loops";

int refuse(const char *who, sm_loops_host::Refusal r, int solver, int nnoise, int Nx, int Nt) {
    switch (r) {
    case sm_loops_host::LOOPS_OK: return SM_OK;
    case sm_loops_host::LOOPS_NULL: return fail(SM_ERR_ARG, "%s: null argument", who);
    case sm_loops_host::LOOPS_SOLVER:
        return fail(SM_ERR_ARG, "%s: solver = %d, expected 0 (D D^dag) or 1 (even-odd)", who, solver);
    case sm_loops_host::LOOPS_NNOISE: return fail(SM_ERR_ARG, "%s: nnoise = %d, expected >= 1", who, nnoise);
    case sm_loops_host::LOOPS_MAX_ITER: return fail(SM_ERR_ARG, "%s: max_iter < 0", who);
    case sm_loops_host::LOOPS_CHECKERBOARD:
        return fail(SM_ERR_ARG, "%s: solver 1 needs even Nx and Nt (%d x %d): an odd periodic lattice has no "
                    "checkerboard", who, Nx, Nt);
    }
    return fail(SM_ERR_ARG, "%s: bad arguments", who);
}

// columns b of a launch: seed[b] and k[b] from the host arrays (pageable: the copies have left them on return)
int upload_noise_ids(hipStream_t s, uint64_t *sk, int K, const uint64_t *seed, const uint64_t *k) {
    HIP_TRY(hipMemcpyAsync(sk, seed, sizeof(uint64_t) * (size_t)K, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sk + kBatchMax, k, sizeof(uint64_t) * (size_t)K, hipMemcpyHostToDevice, s));
    return SM_OK;
}

// The (seed, k) arrays from the first call on; the loops of `cols` columns (`doubles` in all), kept while
// they fit, regrown else. A context's or an ensemble's.
int loops_ready(hipStream_t s, BufGroup &sk_bufs, uint64_t **sk, BufGroup &out_bufs, double **out, size_t *have,
                size_t cols, size_t doubles) {
    if (sk_bufs.empty()) TRY(sk_bufs.add(sk, 2 * (size_t)kBatchMax, BufKind::device, "noise seeds"));
    if (*have >= cols) return SM_OK;
    HIP_TRY(hipStreamSynchronize(s));
    out_bufs.release();
    *have = 0;
    TRY(out_bufs.add(out, doubles, BufKind::device, "loops"));
    *have = cols;
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_quark_loops(sm_ctx *c, double m0, double tol, int max_iter, int solver, int nnoise, uint64_t seed,
                   double *loops, sm_cg_result *res) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    const Geometry &g = c->g;
    TRY(refuse(kLoopsWho, sm_loops_host::args_refusal(loops, loops, loops, solver, nnoise, max_iter, g.Nx, g.Wt),
               solver, nnoise, g.Nx, g.Wt));
    if (c->sharded() || c->hosted || c->peer || c->nshard != 1)
        return fail(SM_ERR_ARG, "quark loops run on one-shard contexts (no loopback, peer or host-staged transport)");
    TRY(check_ready(c));
    HIP_TRY(hipSetDevice(c->device));
    const int Nt = g.Wt, Kmax = std::min(nnoise, kBatchMax);
    hipStream_t s = c->stream;
    if (solver == 1) TRY(pion_eo_ready(c, Kmax));
    else TRY(batch_staging_ready(c, Kmax));
    TRY(loops_ready(s, c->lp_sk_bufs, &c->lp_sk, c->lp_out_bufs, &c->lp_out, &c->lp_cols, (size_t)nnoise,
                    sm_loops_host::loops_doubles(1, nnoise, Nt)));
    const LoopNoise nz{c->lp_sk, c->lp_sk + kBatchMax};
    const BatchLinks L = shared_links(c->U, m0 + 2);
    double2 *Ue = c->eob_U, *Uo = c->eob_U + g.V;
    const EoBatchLinks EL{Ue, Uo, 0, m0 + 2, nullptr};
    if (solver == 1) {
        launch_eob_to_cb(s, g, 1, c->U, Ue, Uo);
        HIP_TRY(hipGetLastError());
    }
    std::vector<sm_cg_result> own((size_t)Kmax);
    std::vector<uint64_t> hs((size_t)Kmax, seed), hk((size_t)Kmax);
    for (int i = 0; i < sm_loops_host::chunk_count(nnoise, kBatchMax); ++i) {
        const int k0 = sm_loops_host::chunk_first(kBatchMax, i), K = sm_loops_host::chunk_size(nnoise, kBatchMax, i);
        for (int b = 0; b < K; ++b) hk[(size_t)b] = (uint64_t)(k0 + b);
        TRY(upload_noise_ids(s, c->lp_sk, K, hs.data(), hk.data()));
        sm_cg_result *r = res ? res + k0 : own.data();
        double *out = c->lp_out + sm_loops_host::loops_index(nnoise, Nt, 0, k0, 0, 0);
        if (solver == 1) {
            const size_t hv = (size_t)K * (size_t)g.V;
            double2 *S = c->pn_buf + 5 * hv;
            c->bt_info.assign((size_t)K, sm_cg_mixed_info{});  // the columns ran fp64
            launch_loops_noise(s, g, K, nz, nullptr, c->pn_buf, c->pn_buf + hv);
            HIP_TRY(hipGetLastError());
            TRY(eo_propagators(c, c->eob, K, c->pn_buf, EL, tol, max_iter, r, S));
            launch_loops_contract(s, g, K, 1, S, L, nz, out, 4L * Nt);
        } else {
            launch_loops_noise(s, g, K, nz, c->bt_phi, nullptr, nullptr);
            HIP_TRY(hipGetLastError());
            TRY(batch_solve(c, K, c->bt_phi, c->bt_x, m0, tol, max_iter, r));
            launch_loops_contract(s, g, K, 0, c->bt_x, L, nz, out, 4L * Nt);  // D^dag y in registers
        }
        HIP_TRY(hipGetLastError());
        // the next chunk rewrites the (seed, k) arrays and the host's copies of them
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(hipMemcpyAsync(loops, c->lp_out, sizeof(double) * sm_loops_host::loops_doubles(1, nnoise, Nt),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SM_OK;
}

int sm_ens_quark_loops(sm_ens *e, const double *m0, double tol, int max_iter, int solver, int nnoise,
                       const uint64_t *seed, double *loops, sm_cg_result *res) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    sm_ctx *c = e->c;
    const Geometry &g = c->g;
    TRY(refuse("ensemble quark loops", sm_loops_host::args_refusal(m0, seed, loops, solver, nnoise, max_iter, g.Nx, g.Wt),
               solver, nnoise, g.Nx, g.Wt));
    TRY(all_have(e));
    HIP_TRY(hipSetDevice(c->device));
    const int R = e->R, Nt = g.Wt;
    hipStream_t s = c->stream;
    if (solver == 1) TRY(eo_fields_ready(e));
    TRY(loops_ready(s, e->lp_sk_bufs, &e->lp_sk, e->lp_out_bufs, &e->lp_out, &e->lp_cols, (size_t)R * (size_t)nnoise,
                    sm_loops_host::loops_doubles(R, nnoise, Nt)));
    for (int r = 0; r < R; ++r) e->h_mass[r] = m0[r] + 2;
    HIP_TRY(hipMemcpyAsync(e->massv, e->h_mass, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, s));
    const LoopNoise nz{e->lp_sk, e->lp_sk + kBatchMax};
    const BatchLinks L = links(e);
    const EoBatchLinks EL = eo_links(e);
    if (solver == 1) launch_eob_to_cb(s, g, R, e->U, e->Ucb, e->Ucb + (size_t)R * g.V);
    HIP_TRY(hipGetLastError());
    const size_t hv = (size_t)R * (size_t)g.V;
    std::vector<sm_cg_result> col((size_t)R);
    std::vector<uint64_t> hk((size_t)R);
    for (int k = 0; k < nnoise; ++k) {
        std::fill(hk.begin(), hk.end(), (uint64_t)k);
        TRY(upload_noise_ids(s, e->lp_sk, R, seed, hk.data()));
        double *out = e->lp_out + sm_loops_host::loops_index(nnoise, Nt, 0, k, 0, 0);
        const long ostride = 4L * nnoise * Nt;  // replica r's vector k lies r * nnoise vectors further
        if (solver == 1) {
            launch_loops_noise(s, g, R, nz, nullptr, e->eh, e->eh + hv);
            HIP_TRY(hipGetLastError());
            TRY(eo_propagators(c, e->eows, R, e->eh, EL, tol, max_iter, col.data(), e->chi));
            launch_loops_contract(s, g, R, 1, e->chi, L, nz, out, ostride);
        } else {
            launch_loops_noise(s, g, R, nz, e->phi, nullptr, nullptr);
            HIP_TRY(hipGetLastError());
            TRY(cg_batch_solve(c, e->ws, R, e->phi, e->x, L, tol, max_iter, col.data()));
            launch_loops_contract(s, g, R, 0, e->x, L, nz, out, ostride);  // D^dag y in registers
        }
        HIP_TRY(hipGetLastError());
        if (res)
            for (int r = 0; r < R; ++r) res[sm_loops_host::res_index(nnoise, r, k)] = col[(size_t)r];
        // the next vector rewrites the k array and the host's copy of it
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(hipMemcpyAsync(loops, e->lp_out, sizeof(double) * sm_loops_host::loops_doubles(R, nnoise, Nt),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SM_OK;
}

}  // extern "C"
