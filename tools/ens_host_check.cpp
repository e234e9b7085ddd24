// ens_host_check.cpp -- the replica ensemble's host bookkeeping (csrc/sm_ens_host.h)
// under the host sanitizers: no device, the trajectory is a stub.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/ens_host_check.cpp -o build/ens_host_check && build/ens_host_check
//
// Covers the lockstep check of R parameter sets, the Metropolis decision, the
// configuration file names, and the run loop: trajectory numbering, which
// updates count towards the acceptance, the series rows, and the summary
// statistics against a restatement over the rows.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../schwingermodel_amd/csrc/sm_ens_host.h"

using namespace sm_ens_host;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// Jackknife_error of src/statistics.cpp:25-34 as sm_jackknife_error restates it
static double jackknife(const double *dat, int n, int bin) {
    const int dat_bin = n / bin;
    std::vector<double> means((size_t)bin);
    for (int i = 0; i < bin; i++) {
        double prom = 0;
        for (int k = 0; k < bin; k++)
            for (int j = k * dat_bin; j < k * dat_bin + dat_bin; j++)
                if (k != i) prom += dat[j];
        means[(size_t)i] = prom / (n - dat_bin);
    }
    const double mean = seq_mean(dat, n);
    double error = 0;
    for (int m = 0; m < bin; m++) error += (means[(size_t)m] - mean) * (means[(size_t)m] - mean);
    return std::sqrt(error * (bin - 1) / bin);
}

static sm_hmc_params prm(double m0, double beta, double tau, int md, double tol, int it, uint64_t seed, int eo) {
    sm_hmc_params p;
    std::memset(&p, 0, sizeof p);
    p.m0 = m0; p.beta = beta; p.tau = tau; p.md_steps = md; p.cg_tol = tol; p.cg_max_iter = it; p.seed = seed;
    p.even_odd = eo;
    return p;
}

static void check_params() {
    std::vector<sm_hmc_params> p = {prm(0.0, 2, 0.3, 6, 1e-10, 100, 1, 0), prm(0.1, 3, 0.5, 6, 1e-10, 100, 2, 0),
                                    prm(0.2, 2, 0.4, 6, 1e-10, 100, 3, 0)};
    CHECK(params_refusal(p.data(), 3) == nullptr);  // m0, beta, tau, seed are free
    auto refused = [&](int r, void (*edit)(sm_hmc_params &), const char *field) {
        std::vector<sm_hmc_params> q = p;
        edit(q[(size_t)r]);
        const char *f = params_refusal(q.data(), 3);
        CHECK(f && std::string(f) == field);
        CHECK(params_refusal(q.data(), r) == nullptr || r == 0);  // the replicas before r alone pass
    };
    refused(1, [](sm_hmc_params &x) { x.md_steps = 7; }, "md_steps");
    refused(2, [](sm_hmc_params &x) { x.md_steps = 0; }, "md_steps");
    refused(0, [](sm_hmc_params &x) { x.md_steps = 0; }, "md_steps");
    refused(2, [](sm_hmc_params &x) { x.cg_tol = 1e-9; }, "cg_tol");
    refused(1, [](sm_hmc_params &x) { x.cg_tol = std::nan(""); }, "cg_tol");
    refused(1, [](sm_hmc_params &x) { x.cg_max_iter = 99; }, "cg_max_iter");
    refused(2, [](sm_hmc_params &x) { x.even_odd = 1; }, "even_odd");
    refused(0, [](sm_hmc_params &x) { x.even_odd = 1; }, "even_odd");   // replica 0 alone differs
    refused(1, [](sm_hmc_params &x) { x.even_odd = 2; }, "even_odd");
    refused(1, [](sm_hmc_params &x) { x.even_odd = -1; }, "even_odd");
    {  // even_odd is a lockstep parameter: 1 for every replica passes, 2 for every replica does not
        std::vector<sm_hmc_params> q = p;
        for (sm_hmc_params &x : q) x.even_odd = 1;
        CHECK(params_refusal(q.data(), 3) == nullptr);
        q[1].md_steps = 7;  // and the other checks still apply to it
        const char *f = params_refusal(q.data(), 3);
        CHECK(f && std::string(f) == "md_steps");
        q = p;
        for (sm_hmc_params &x : q) x.even_odd = 2;
        f = params_refusal(q.data(), 3);
        CHECK(f && std::string(f) == "even_odd");
    }
    refused(1, [](sm_hmc_params &x) { x.tau = 0.0; }, "tau");
    refused(1, [](sm_hmc_params &x) { x.tau = std::nan(""); }, "tau");
}

static void check_metropolis() {
    CHECK(metropolis(0.5, 0.0) == 1);                    // exp(0) = 1
    CHECK(metropolis(0.999999, -1e-3) == 1);             // dH < 0 always accepts
    CHECK(metropolis(std::exp(-0.25), 0.25) == 1);       // r == exp(-dH): accepted (<=)
    CHECK(metropolis(std::nextafter(std::exp(-0.25), 1.0), 0.25) == 0);
    CHECK(metropolis(0.1, std::nan("")) == 0);           // a broken trajectory is never kept
    CHECK(metropolis(0.1, INFINITY) == 0);
}

static void check_names() {
    CHECK(conf_name("conf", 0, 0) == "conf_r0_0.ctxt");
    CHECK(conf_name("/tmp/a b/run", 63, 124) == "/tmp/a b/run_r63_124.ctxt");
}

static void check_run_loop() {
    const int R = 3, Ntherm = 2, Nmeas = 41, Nsteps = 2;
    const double Ntot = 64.0;
    std::vector<uint64_t> seen;
    std::vector<int> saved;
    // replica r, trajectory t: sp = 100 r + t, action = 2 sp, accepted when (t + r) is even,
    // r + 1 iterations, a failure on trajectory 15 of replica 1
    auto update = [&](uint64_t traj, sm_hmc_result *res) -> int {
        seen.push_back(traj);
        for (int r = 0; r < R; ++r) {
            std::memset(&res[r], 0, sizeof res[r]);
            res[r].sp = 100.0 * r + (double)traj;
            res[r].gauge_action = 2.0 * res[r].sp;
            res[r].accepted = (int)((traj + r) % 2 == 0);
            res[r].cg_iterations = r + 1;
            res[r].cg_failures = (r == 1 && traj == 15) ? 1 : 0;
        }
        return SM_OK;
    };
    auto save = [&](int i) -> int {
        saved.push_back(i);
        return SM_OK;
    };
    std::vector<sm_hmc_summary> out((size_t)R);
    std::vector<double> sp((size_t)R * Nmeas), gs((size_t)R * Nmeas);
    const uint64_t first = 10;
    CHECK(run_loop(R, Ntot, first, Ntherm, Nmeas, Nsteps, update, save, jackknife, out.data(), sp.data(), gs.data()) ==
          SM_OK);
    const long ntraj = Ntherm + Nmeas + (long)Nsteps * (Nmeas - 1);
    CHECK((long)seen.size() == ntraj);
    for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == first + i);  // numbered from first_traj, no gaps
    CHECK((int)saved.size() == Nmeas);
    for (int i = 0; i < Nmeas; ++i) CHECK(saved[(size_t)i] == i);
    for (int r = 0; r < R; ++r) {
        long acc = 0;
        for (int i = 0; i < Nmeas; ++i) {
            const uint64_t t = first + Ntherm + (uint64_t)i * (1 + Nsteps);  // the measured trajectory
            CHECK(sp[(size_t)r * Nmeas + i] == 100.0 * r + (double)t);
            CHECK(gs[(size_t)r * Nmeas + i] == 2.0 * sp[(size_t)r * Nmeas + i]);
        }
        for (uint64_t t = first + Ntherm; t < first + (uint64_t)ntraj; ++t) acc += (t + r) % 2 == 0;  // not the thermalisation
        const sm_hmc_summary &o = out[(size_t)r];
        const double *s = sp.data() + (size_t)r * Nmeas, *g = gs.data() + (size_t)r * Nmeas;
        CHECK(o.accepted == acc);
        CHECK(o.acceptance == acc / ((Nmeas + Nsteps * (Nmeas - 1)) * 1.0));
        CHECK(o.trajectories == ntraj);
        CHECK(o.cg_iterations == ntraj * (r + 1));
        CHECK(o.cg_failures == (r == 1 ? 1 : 0));
        CHECK(o.Ep == seq_mean(s, Nmeas) / Ntot);
        CHECK(o.dEp == jackknife(s, Nmeas, 20) / Ntot);
        CHECK(o.gS == seq_mean(g, Nmeas) / Ntot);
        CHECK(o.dgS == jackknife(g, Nmeas, 20) / Ntot);
        CHECK(o.cg_link_bytes == 32);
    }
    // null series and no save; a failing trajectory ends the run with its code
    CHECK(run_loop(R, Ntot, 0, 0, 1, 0, update, nullptr, jackknife, out.data(), nullptr, nullptr) == SM_OK);
    CHECK(out[0].trajectories == 1);
    int calls = 0;
    auto failing = [&](uint64_t, sm_hmc_result *) -> int { return ++calls == 3 ? SM_ERR_HIP : SM_OK; };
    CHECK(run_loop(R, Ntot, 0, 1, 4, 1, failing, save, jackknife, out.data(), nullptr, nullptr) == SM_ERR_HIP);
    CHECK(calls == 3);
}

int main() {
    check_params();
    check_metropolis();
    check_names();
    check_run_loop();
    if (failures) {
        std::fprintf(stderr, "ens_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("ens_host_check ok\n");
    return 0;
}
