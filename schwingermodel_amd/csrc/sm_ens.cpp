// sm_ens.cpp -- an ensemble of R independent HMC chains in one context, evolved
// in lockstep: every CG iteration and every MD kernel is ONE launch for all
// replicas (include/sm_hip.h, "replica ensemble").
//
// Why: below 256^2 a lone chain is launch-latency bound (a CG iteration costs
// 11-12 us whatever the lattice); the batched CG of sm_cgbatch.hip already runs
// K columns per launch, here column r reads replica r's links and mass.
//
//   fields   U, its backup, P, F, chi / T, phi, x: R slabs each, replica r at
//            + r * 2V; the batched CG's workspace for R columns. All its own:
//            the context's U, solvers and buffers are never touched.
//   links    per-column base U + r * ustride (block-uniform, in SGPRs). The
//            leapfrog evolves U in place after one device copy of all slabs to
//            the backup; a rejected replica is copied back (that replica only),
//            an accepted one costs nothing.
//   sums     kinetic, plaquette and <x, phi> partials per replica with the
//            one-field kernels' block decomposition and order, summed by one
//            launch and read with one synchronisation per Hamiltonian.
//   draws    replica r's are those of a lone chain with p[r].seed.
//
//   even-odd the action phi_e^dag (Dhat Dhat^dag)^-1 phi_e of sm_eo.cpp when every
//            replica asks for it: the checkerboard links of all slabs are
//            rebuilt before every solve (one launch), X comes from one batched
//            even-odd solve (sm_eobatch.cpp), Dhat chi, Dhat^dag X and the odd
//            parts of l and r from batched checkerboard hops. Its fields are
//            allocated at the first even-odd trajectory.
//
// One-shard contexts, always fp64. Kernels: sm_gauge.hip, sm_kernels.hip
// (ens_*), sm_cgbatch.hip, sm_eobatch.hip. Host bookkeeping that needs no
// device: sm_ens_host.h. The state itself (struct sm_ens) is in sm_ens.h, which
// the measurements of sm_pion.cpp share; they work in chi, phi, x and the solver
// workspaces between trajectories and write nothing a trajectory reads before
// writing it.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "sm_ctx.h"
#include "sm_ens.h"
#include "sm_ens_host.h"
#include "sm_fields.h"
#include "sm_internal.h"

using namespace sm;
using namespace sm_host;

namespace sm_host {

int all_have(const sm_ens *e) {
    for (int r = 0; r < e->R; ++r)
        if (!e->have[(size_t)r])
            return fail(SM_ERR_STATE, "ensemble: replica %d has no gauge field (sm_ens_upload_gauge / sm_ens_fill_gauge)",
                        r);
    return SM_OK;
}

// The even-odd action's fields: 32 B per site and replica of checkerboard
// links, 96 of half-lattice fields and 80 of the batched solver's workspace.
int eo_fields_ready(sm_ens *e) {
    BufGroup &b = e->eo_bufs;
    if (!b.empty()) return SM_OK;
    sm_ctx *c = e->c;
    const size_t hn = (size_t)c->g.V * (size_t)e->R;
    int rc = b.add(&e->Ucb, 2 * hn, BufKind::device, "checkerboard links");
    if (rc == SM_OK) rc = batch_ws_alloc(c, e->eows, e->R, c->g.V, eo_batch_config(c->g, e->R, c->eob_tiles).pstride);
    if (rc == SM_OK) rc = b.add(&e->eh, EH_N * hn, BufKind::device, "even-odd fields");
    if (rc != SM_OK) {  // each owner emptied itself; here the other one
        b.release();
        batch_ws_free(e->eows);
    }
    return rc;
}

}  // namespace sm_host

namespace {

struct HTerms {
    double H, sp, action;
    int iterations, converged;
};

int ens_check(const sm_ens *e, int r) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    if (r < 0 || r >= e->R) return fail(SM_ERR_ARG, "ensemble: replica %d outside 0..%d", r, e->R - 1);
    return SM_OK;
}

// X = (Dhat Dhat^dag)^-1 phi_e of every replica on its current links
int eo_solve(sm_ens *e, double tol, int max_iter, sm_cg_result *res) {
    sm_ctx *c = e->c;
    const EoBatchLinks L = eo_links(e);
    launch_eob_to_cb(c->stream, c->g, e->R, e->U, e->Ucb, e->Ucb + (size_t)e->R * c->g.V);
    HIP_TRY(hipGetLastError());
    return eo_batch_solve(c, e->eows, e->R, eh(e, EH_PHI), eh(e, EH_X), L, tol, max_iter, res);
}

int upload_params(sm_ens *e) {
    sm_ctx *c = e->c;
    HIP_TRY(hipMemcpyAsync(e->par, e->h_par, sizeof(EnsPar) * (size_t)e->R, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(e->massv, e->h_mass, sizeof(double) * (size_t)e->R, hipMemcpyHostToDevice, c->stream));
    return SM_OK;
}

// rows [0, nrows) of e->part summed into e->h_sums: the one synchronisation of a reduction stage
int read_sums(sm_ens *e, int nrows) {
    sm_ctx *c = e->c;
    launch_ens_sums(c->stream, c->g, nrows, e->part, e->sums);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e->h_sums, e->sums, sizeof(double2) * (size_t)nrows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

// HMC::Hamiltonian + HMC::Action (src/hmc.cpp:104-148) of every replica: rows
// [0, R) kinetic, [R, 2R) plaquette, [2R, 3R) <x, phi>
int hamiltonian(sm_ens *e, bool eo, double tol, int max_iter, std::vector<sm_cg_result> &res,
                std::vector<HTerms> &h) {
    sm_ctx *c = e->c;
    const int R = e->R;
    const size_t row = (size_t)gauge_reduce_blocks(c->g);
    launch_ens_kinetic(c->stream, c->g, R, e->P, e->part);
    launch_ens_plaquette(c->stream, c->g, R, e->U, e->par, e->part + (size_t)R * row);
    HIP_TRY(hipGetLastError());
    if (eo) {  // Re <X, phi_e>: e->x = (X, 0) against e->phi = (phi_e, 0)
        TRY(eo_solve(e, tol, max_iter, res.data()));
        launch_eob_from_cb(c->stream, c->g, R, eh(e, EH_X), nullptr, e->x);
    } else {
        TRY(cg_batch_solve(c, e->ws, R, e->phi, e->x, links(e), tol, max_iter, res.data()));
    }
    launch_ens_dot(c->stream, c->g, R, e->x, e->phi, e->part + 2 * (size_t)R * row);
    TRY(read_sums(e, 3 * R));
    for (int r = 0; r < R; ++r) {
        const double k = e->h_sums[r].x, z = e->h_sums[2 * R + r].x;
        const double2 pl = e->h_sums[R + r];
        HTerms &t = h[(size_t)r];
        t.sp = pl.x;
        t.action = pl.y;
        t.H = k + (t.action + z);
        t.iterations = res[(size_t)r].iterations;
        t.converged = res[(size_t)r].converged;
    }
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_ens_max(void) { return kBatchMax; }

int sm_ens_create(sm_ctx *c, int R, sm_ens **out) {
    if (!c || !out) return fail(SM_ERR_ARG, "null argument");
    *out = nullptr;
    if (c->sharded() || c->hosted || c->peer || c->nshard != 1)
        return fail(SM_ERR_ARG, "the replica ensemble runs on one-shard contexts (no loopback, peer or host-staged transport)");
    if (R < 1 || R > kBatchMax) return fail(SM_ERR_ARG, "ensemble: R = %d outside 1..%d", R, kBatchMax);
    HIP_TRY(hipSetDevice(c->device));
    sm_ens *e = new sm_ens;
    e->c = c;
    e->R = R;
    e->have.assign((size_t)R, 0);
    const size_t fn = slab_complex(e) * (size_t)R;  // complex of R fields = doubles of R momenta
    const size_t nsum = 3 * (size_t)R, np = nsum * (size_t)gauge_reduce_blocks(c->g);
    const int rc = [&] {
        BufGroup &b = e->bufs;
        TRY(b.add(&e->U, fn, BufKind::device, "gauge fields"));
        TRY(b.add(&e->Ubak, fn, BufKind::device, "kept gauge fields"));
        TRY(b.add(&e->chi, fn, BufKind::device, "chi"));
        TRY(b.add(&e->phi, fn, BufKind::device, "phi"));
        TRY(b.add(&e->x, fn, BufKind::device, "solutions"));
        TRY(b.add(&e->P, fn, BufKind::device, "momenta"));
        TRY(b.add(&e->F, fn, BufKind::device, "forces"));
        TRY(b.add(&e->par, (size_t)R, BufKind::device, "parameters"));
        TRY(b.add(&e->massv, (size_t)R, BufKind::device, "masses"));
        TRY(b.add(&e->part, np, BufKind::device, "partials"));
        TRY(b.add(&e->sums, nsum, BufKind::device, "sums"));
        TRY(b.add(&e->h_par, (size_t)R, BufKind::pinned, "pinned parameters"));
        TRY(b.add(&e->h_mass, (size_t)R, BufKind::pinned, "pinned masses"));
        TRY(b.add(&e->h_sums, nsum, BufKind::pinned, "pinned sums"));
        return batch_ws_alloc(c, e->ws, R, 2 * c->g.V, cg_batch_config(c->g, R, c->bt_tiles).pstride);
    }();
    if (rc != SM_OK) {
        delete e;
        return rc;
    }
    *out = e;
    return SM_OK;
}

int sm_ens_destroy(sm_ens *e) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    (void)hipSetDevice(e->c->device);
    (void)hipStreamSynchronize(e->c->stream);
    delete e;  // the BufGroups free here
    return SM_OK;
}

int sm_ens_size(const sm_ens *e, int *R) {
    if (!e || !R) return fail(SM_ERR_ARG, "null argument");
    *R = e->R;
    return SM_OK;
}

int sm_ens_upload_gauge(sm_ens *e, int r, const double *U0, const double *U1) {
    TRY(ens_check(e, r));
    if (!U0 || !U1) return fail(SM_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->c->device));
    TRY(upload_plane_pair(e->c, e->U + (size_t)r * slab_complex(e), U0, U1));
    HIP_TRY(hipStreamSynchronize(e->c->stream));
    e->have[(size_t)r] = 1;
    return SM_OK;
}

int sm_ens_download_gauge(sm_ens *e, int r, double *U0, double *U1) {
    TRY(ens_check(e, r));
    if (!U0 || !U1) return fail(SM_ERR_ARG, "null argument");
    if (!e->have[(size_t)r]) return fail(SM_ERR_STATE, "ensemble: replica %d has no gauge field", r);
    HIP_TRY(hipSetDevice(e->c->device));
    return download_plane_pair(e->c, e->U + (size_t)r * slab_complex(e), U0, U1);
}

int sm_ens_fill_gauge(sm_ens *e, int r, uint64_t seed, double sigma) {
    TRY(ens_check(e, r));
    HIP_TRY(hipSetDevice(e->c->device));
    launch_draw_gauge(e->c->stream, e->c->g, seed, sigma, e->U + (size_t)r * slab_complex(e));
    HIP_TRY(hipGetLastError());
    e->have[(size_t)r] = 1;
    return SM_OK;
}

int sm_ens_plaquette(sm_ens *e, const double *beta, double *sp, double *gauge_action) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    if (!beta || !sp || !gauge_action) return fail(SM_ERR_ARG, "null argument");
    TRY(all_have(e));
    sm_ctx *c = e->c;
    HIP_TRY(hipSetDevice(c->device));
    for (int r = 0; r < e->R; ++r) {
        e->h_par[r] = EnsPar{beta[r], 0.0, 0};
        e->h_mass[r] = 0.0;
    }
    TRY(upload_params(e));
    launch_ens_plaquette(c->stream, c->g, e->R, e->U, e->par, e->part);
    TRY(read_sums(e, e->R));
    for (int r = 0; r < e->R; ++r) {
        sp[r] = e->h_sums[r].x;
        gauge_action[r] = e->h_sums[r].y;
    }
    return SM_OK;
}

int sm_ens_hmc_trajectory(sm_ens *e, const sm_hmc_params *p, uint64_t traj, sm_hmc_result *out) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    if (!p || !out) return fail(SM_ERR_ARG, "null argument");
    if (const char *f = sm_ens_host::params_refusal(p, e->R))
        return fail(SM_ERR_ARG,
                    "ensemble: bad or differing %s (md_steps, cg_tol, cg_max_iter and even_odd = 0 or 1 are common to "
                    "the replicas, tau > 0)", f);
    TRY(all_have(e));
    sm_ctx *c = e->c;
    const bool eo = p[0].even_odd == 1;
    if (eo && (c->g.Nx % 2 || c->g.Wt % 2))
        return fail(SM_ERR_ARG, "ensemble: even_odd = 1 needs even Nx and Nt (%d x %d): an odd periodic lattice has no "
                    "checkerboard", c->g.Nx, c->g.Wt);
    const int R = e->R, md_steps = p[0].md_steps, max_iter = p[0].cg_max_iter;
    const double tol = p[0].cg_tol;
    const Geometry &g = c->g;
    HIP_TRY(hipSetDevice(c->device));
    if (eo) TRY(eo_fields_ready(e));
    // HMC::HMC_Update, src/hmc.cpp:151-178, for every replica
    for (int r = 0; r < R; ++r) {
        e->h_par[r] = EnsPar{p[r].beta, p[r].tau / (md_steps * 1.0), sm_traj_seed(p[r].seed, traj)};
        e->h_mass[r] = p[r].m0 + 2;
    }
    TRY(upload_params(e));
    const BatchLinks L = links(e);
    launch_ens_draws(c->stream, g, R, e->par, e->P, e->chi);    // RandomPI, RandomCHI
    if (eo) {  // phi = (Dhat chi_e, 0) on the replicas' checkerboard links
        const EoBatchLinks EL = eo_links(e);
        launch_eob_to_cb(c->stream, g, R, e->U, e->Ucb, e->Ucb + (size_t)R * g.V);
        launch_eob_to_cb(c->stream, g, R, e->chi, eh(e, EH_LO), nullptr);
        launch_eob_dhat(c->stream, g, R, 0, eh(e, EH_LO), eh(e, EH_T), eh(e, EH_PHI), EL);
        launch_eob_from_cb(c->stream, g, R, eh(e, EH_PHI), nullptr, e->phi);
    } else {
        launch_batch_apply(c->stream, g, R, 0, e->chi, e->phi, L);  // phi = D chi
    }
    HIP_TRY(hipGetLastError());
    std::vector<sm_cg_result> res((size_t)R);
    std::vector<HTerms> h0((size_t)R), h1((size_t)R);
    TRY(hamiltonian(e, eo, tol, max_iter, res, h0));  // H[U][Pi]
    const size_t fb = sizeof(double2) * slab_complex(e);
    HIP_TRY(hipMemcpyAsync(e->Ubak, e->U, fb * (size_t)R, hipMemcpyDeviceToDevice, c->stream));
    // HMC::Leapfrog, src/hmc.cpp:63-101, its loop bound included: md_steps - 1 forces
    std::vector<long> lf_iters((size_t)R, 0);
    std::vector<int> lf_fails((size_t)R, 0);
    double2 *T = e->chi;
    auto force = [&]() -> int {  // HMC::Force, src/hmc.cpp:44-60
        if (eo) {  // eo_md_force (sm_eo.cpp): l = (X, (1/2m) H'_oe X), r = (Y, (1/2m) H_oe Y), Y = Dhat^dag X
            TRY(eo_solve(e, tol, max_iter, res.data()));
            const EoBatchLinks EL = eo_links(e);
            launch_eob_dhat(c->stream, g, R, 1, eh(e, EH_X), eh(e, EH_T), eh(e, EH_Y), EL);
            launch_eob_hop(c->stream, g, R, 1, 1, 2, eh(e, EH_X), nullptr, eh(e, EH_LO), EL);
            launch_eob_hop(c->stream, g, R, 0, 1, 2, eh(e, EH_Y), nullptr, eh(e, EH_RO), EL);
            launch_eob_from_cb(c->stream, g, R, eh(e, EH_X), eh(e, EH_LO), e->x);
            launch_eob_from_cb(c->stream, g, R, eh(e, EH_Y), eh(e, EH_RO), T);
        } else {
            TRY(cg_batch_solve(c, e->ws, R, e->phi, e->x, L, tol, max_iter, res.data()));
            launch_batch_apply(c->stream, g, R, 1, e->x, T, L);
        }
        launch_ens_force(c->stream, g, R, e->U, e->x, T, e->F);
        launch_ens_staple_force(c->stream, g, R, e->U, e->par, e->F);
        HIP_TRY(hipGetLastError());
        for (int r = 0; r < R; ++r) {
            lf_iters[(size_t)r] += res[(size_t)r].iterations;
            lf_fails[(size_t)r] += res[(size_t)r].converged ? 0 : 1;
        }
        return SM_OK;
    };
    launch_ens_md_update(c->stream, g, R, e->U, e->P, e->F, e->par, 0, 0.5);
    TRY(force());
    for (int step = 1; step < md_steps - 1; step++) {
        launch_ens_md_update(c->stream, g, R, e->U, e->P, e->F, e->par, 1, 1.0);
        TRY(force());
    }
    launch_ens_md_update(c->stream, g, R, e->U, e->P, e->F, e->par, 1, 0.5);
    HIP_TRY(hipGetLastError());
    TRY(hamiltonian(e, eo, tol, max_iter, res, h1));  // H[U'][Pi']
    for (int r = 0; r < R; ++r) {
        sm_hmc_result &o = out[r];
        const HTerms &a = h0[(size_t)r], &b = h1[(size_t)r];
        o.H_old = a.H;
        o.H_new = b.H;
        o.dH = b.H - a.H;
        o.r = sm_uniform(e->h_par[r].seed, SM_STREAM_ACCEPT, 0);
        o.accepted = sm_ens_host::metropolis(o.r, o.dH);
        if (!o.accepted)  // back to the previous configuration: this replica's slab only
            HIP_TRY(hipMemcpyAsync(e->U + (size_t)r * slab_complex(e), e->Ubak + (size_t)r * slab_complex(e), fb,
                                   hipMemcpyDeviceToDevice, c->stream));
        const HTerms &kept = o.accepted ? b : a;
        o.sp = kept.sp;
        o.gauge_action = kept.action;
        o.cg_iterations = (long)a.iterations + lf_iters[(size_t)r] + b.iterations;
        o.cg_failures = (a.converged ? 0 : 1) + lf_fails[(size_t)r] + (b.converged ? 0 : 1);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

int sm_ens_hmc_run(sm_ens *e, const sm_hmc_params *p, int hot_start, uint64_t first_traj, int Ntherm, int Nmeas,
                   int Nsteps, const char *save_prefix, sm_hmc_summary *out, double *sp_series, double *gs_series) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    if (!p || !out) return fail(SM_ERR_ARG, "null argument");
    if (Ntherm < 0 || Nmeas < 1 || Nsteps < 0)
        return fail(SM_ERR_ARG, "Ntherm=%d Nmeas=%d Nsteps=%d", Ntherm, Nmeas, Nsteps);
    // GaugeConf::initialization per replica, from the key sm_hmc_run uses
    if (hot_start)
        for (int r = 0; r < e->R; ++r) TRY(sm_ens_fill_gauge(e, r, sm_traj_seed(p[r].seed, ~0ull), -1.0));
    TRY(all_have(e));
    const Geometry &g = e->c->g;
    std::vector<double> U0, U1;
    std::function<int(int)> save;
    if (save_prefix)
        save = [&](int i) -> int {
            U0.resize((size_t)2 * g.V);
            U1.resize((size_t)2 * g.V);
            for (int r = 0; r < e->R; ++r) {
                TRY(sm_ens_download_gauge(e, r, U0.data(), U1.data()));
                TRY(sm_conf_write(sm_ens_host::conf_name(save_prefix, r, i).c_str(), g.Nx, g.Ntg, U0.data(), U1.data()));
            }
            return SM_OK;
        };
    return sm_ens_host::run_loop(
        e->R, (double)g.Nx * g.Ntg, first_traj, Ntherm, Nmeas, Nsteps,
        [&](uint64_t traj, sm_hmc_result *res) { return sm_ens_hmc_trajectory(e, p, traj, res); }, save,
        sm_jackknife_error, out, sp_series, gs_series);
}

}  // extern "C"
