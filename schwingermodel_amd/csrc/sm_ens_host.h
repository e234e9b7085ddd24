// sm_ens_host.h -- the replica ensemble's host-side bookkeeping (sm_ens.cpp),
// free of any device call so that tools/ens_host_check.cpp can run it under
// the host sanitizers: the check of R parameter sets that must run in
// lockstep, the Metropolis decision, the configuration file names, and
// HMC::HMC_algorithm's loop (src/hmc.cpp:181-213) with the reference's
// statistics per replica, as sm_hmc_run keeps them for one chain.
#pragma once
#include "../../include/sm_hip.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <vector>

namespace sm_ens_host {

// The first field that keeps p[0..R) from running as one ensemble, or null.
// Per replica: m0, beta, tau, seed. Common: md_steps, cg_tol, cg_max_iter
// (the replicas share every launch), and even_odd, which is 0 (the plain
// action) or 1 (the even-odd action) for all of them: the two actions run
// different launches.
inline const char *params_refusal(const sm_hmc_params *p, int R) {
    for (int r = 0; r < R; ++r) {
        if ((p[r].even_odd != 0 && p[r].even_odd != 1) || p[r].even_odd != p[0].even_odd) return "even_odd";
        if (p[r].md_steps < 1 || p[r].md_steps != p[0].md_steps) return "md_steps";
        if (p[r].cg_max_iter < 1 || p[r].cg_max_iter != p[0].cg_max_iter) return "cg_max_iter";
        if (!(p[r].cg_tol == p[0].cg_tol)) return "cg_tol";
        if (!(p[r].tau > 0.0)) return "tau";
    }
    return nullptr;
}

// HMC::HMC_Update's test, src/hmc.cpp:170-176
inline int metropolis(double r, double dH) { return r <= std::exp(-dH) ? 1 : 0; }

inline std::string conf_name(const char *prefix, int r, int i) {
    return std::string(prefix) + "_r" + std::to_string(r) + "_" + std::to_string(i) + ".ctxt";
}

// mean() of include/statistics.h:9-16: sequential sum, then divide.
inline double seq_mean(const double *x, int n) {
    double prom = 0;
    for (int i = 0; i < n; ++i) prom += x[i] * 1.0;
    return prom / n;
}

// update(traj, res): one trajectory of all R replicas into res[0..R);
// save(i): called after measurement i (null: nothing is saved);
// jackknife: sm_jackknife_error. out[r] and the series rows sp / gs (R x Nmeas,
// nullable) are filled as sm_hmc_run fills them for a lone chain.
inline int run_loop(int R, double Ntot, uint64_t first_traj, int Ntherm, int Nmeas, int Nsteps,
                    const std::function<int(uint64_t, sm_hmc_result *)> &update, const std::function<int(int)> &save,
                    double (*jackknife)(const double *, int, int), sm_hmc_summary *out, double *sp_series,
                    double *gs_series) {
    std::vector<sm_hmc_result> res((size_t)R);
    std::vector<double> sp((size_t)R * Nmeas), gs((size_t)R * Nmeas);
    std::vector<long> accepted((size_t)R, 0), cg_it((size_t)R, 0);
    std::vector<int> cg_fail((size_t)R, 0);
    uint64_t traj = first_traj;
    long ntraj = 0;
    auto step = [&](bool measured) -> int {
        const int rc = update(traj++, res.data());
        if (rc != SM_OK) return rc;
        ++ntraj;
        for (int r = 0; r < R; ++r) {
            cg_it[(size_t)r] += res[(size_t)r].cg_iterations;
            cg_fail[(size_t)r] += res[(size_t)r].cg_failures;
            if (measured) accepted[(size_t)r] += res[(size_t)r].accepted;
        }
        return SM_OK;
    };
    for (int i = 0; i < Ntherm; ++i)
        if (const int rc = step(false)) return rc;
    for (int i = 0; i < Nmeas; ++i) {
        if (const int rc = step(true)) return rc;
        for (int r = 0; r < R; ++r) {
            sp[(size_t)r * Nmeas + i] = res[(size_t)r].sp;
            gs[(size_t)r * Nmeas + i] = res[(size_t)r].gauge_action;
        }
        if (save)
            if (const int rc = save(i)) return rc;
        if (i != Nmeas - 1)
            for (int j = 0; j < Nsteps; ++j)
                if (const int rc = step(true)) return rc;
    }
    for (int r = 0; r < R; ++r) {
        const double *s = sp.data() + (size_t)r * Nmeas, *g = gs.data() + (size_t)r * Nmeas;
        sm_hmc_summary &o = out[r];
        o.Ep = seq_mean(s, Nmeas) / (Ntot * 1.0);
        o.dEp = jackknife(s, Nmeas, 20) / (Ntot * 1.0);
        o.gS = seq_mean(g, Nmeas) / (Ntot * 1.0);
        o.dgS = jackknife(g, Nmeas, 20) / (Ntot * 1.0);
        o.accepted = accepted[(size_t)r];
        o.acceptance = accepted[(size_t)r] / ((Nmeas + Nsteps * (Nmeas - 1)) * 1.0);
        o.trajectories = ntraj;
        o.cg_iterations = cg_it[(size_t)r];
        o.cg_failures = cg_fail[(size_t)r];
        o.cg_link_bytes = 32;  // the batched pass reads the complex links
    }
    if (sp_series) std::copy(sp.begin(), sp.end(), sp_series);
    if (gs_series) std::copy(gs.begin(), gs.end(), gs_series);
    return SM_OK;
}

}  // namespace sm_ens_host
