// sm_ens.h -- the replica ensemble's state (the opaque sm_ens of
// include/sm_hip.h), shared by its HMC (sm_ens.cpp) and its measurements
// (sm_pion.cpp). Private; the layout of every field is in sm_ens.cpp's header.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "sm_ctx.h"
#include "sm_internal.h"

// Every buffer belongs to a BufGroup (sm_buf.h) next to its pointers, built whole
// or not at all and freed at sm_ens_destroy's `delete`, after the stream was
// synchronised; the two solver workspaces own theirs.
struct sm_ens {
    sm_ctx *c = nullptr;
    int R = 0;
    sm_host::BufGroup bufs{"ensemble"};                     // everything sm_ens_create allocates but ws
    double2 *U = nullptr, *Ubak = nullptr;                  // R x 2V complex
    double2 *chi = nullptr, *phi = nullptr, *x = nullptr;   // chi doubles as T = D^dag psi of the force
    double *P = nullptr, *F = nullptr;                      // R x 2V doubles
    BatchWs ws{sm_host::kBatchWho};
    sm::EnsPar *par = nullptr, *h_par = nullptr;            // device, pinned host
    double *massv = nullptr, *h_mass = nullptr;             // m0 + 2 per replica
    double2 *part = nullptr;                                // 3 x R x gauge_reduce_blocks partials
    double2 *sums = nullptr, *h_sums = nullptr;             // 3 x R
    std::vector<char> have;                                 // replica r holds a gauge field
    // even-odd action, from the first even-odd trajectory (or even-odd measurement) on
    BatchWs eows{sm_host::kEoBatchWho};
    sm_host::BufGroup eo_bufs{"ensemble"};                  // Ucb, eh
    double2 *Ucb = nullptr;                                 // even links R x V complex, then odd links R x V
    double2 *eh = nullptr;                                  // EH_N half-lattice fields, R x V complex each
    // pion correlator (sm_pion.cpp), from the first measurement on
    int *pn_src = nullptr;                                  // 2 x kBatchMax / 2 source coordinates
    double *pn_C = nullptr;                                 // R x kBatchMax / 2 x Wt
    sm_host::BufGroup pn_bufs{"ensemble"};
    // topological charge and Wilson flow (sm_flow.cpp): the series on the device, regrown for a longer one
    double *fl_series = nullptr;                            // R x fl_points x 3
    long fl_points = 0;
    sm_host::BufGroup fl_series_bufs{"Wilson flow"};
    // stochastic quark loops (sm_loops.cpp), from the first measurement on
    uint64_t *lp_sk = nullptr;                              // 2 x kBatchMax: the replicas' seeds, then the vector number
    double *lp_out = nullptr;                               // lp_cols x Wt x 4, lp_cols >= R x nnoise
    size_t lp_cols = 0;
    sm_host::BufGroup lp_sk_bufs{"ensemble"}, lp_out_bufs{"ensemble"};
};

namespace sm_host {

inline size_t slab_complex(const sm_ens *e) { return 2 * (size_t)e->c->g.V; }

// half-lattice fields of the even-odd action: phi_e, X, Y = Dhat^dag X, the odd
// work field of Dhat, l_o (chi_e during the heat bath), r_o
enum { EH_PHI, EH_X, EH_Y, EH_T, EH_LO, EH_RO, EH_N };
inline double2 *eh(const sm_ens *e, int i) { return e->eh + (size_t)i * (size_t)e->R * (size_t)e->c->g.V; }

inline BatchLinks links(const sm_ens *e) { return BatchLinks{e->U, (long)slab_complex(e), 0.0, e->massv}; }

inline EoBatchLinks eo_links(const sm_ens *e) {
    const long V = e->c->g.V;
    return EoBatchLinks{e->Ucb, e->Ucb + (size_t)e->R * V, V, 0.0, e->massv};
}

int all_have(const sm_ens *e);      // SM_ERR_STATE naming the first replica without a gauge field
int eo_fields_ready(sm_ens *e);     // the even-odd fields, allocated at first use

}  // namespace sm_host
