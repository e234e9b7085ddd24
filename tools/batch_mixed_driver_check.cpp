// batch_mixed_driver_check.cpp -- the decisions of the mixed-precision solvers'
// reliable-update driver (csrc/sm_cg_host.h cg_mixed_drive) on K columns under the host
// sanitizers: no device, the operations are a script per column.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/batch_mixed_driver_check.cpp -o build/batch_mixed_driver_check && build/batch_mixed_driver_check
//
// Every column has its own script: the fp64 true residuals, and each segment's k, done and
// bad (tools/mixed_driver_check.cpp's). The batch is driven with all K scripts at once, and
// each script alone as a one-column solver's operations through MixedColumn: a column's
// result, report and the sequence of its own operations (true residuals, injections, folds,
// the fp64 finish and what it is given) must be the same. Both sides run the one driver, so
// this pins that a column is not touched by its neighbours; what the decisions are on a
// column alone is tools/mixed_driver_check.cpp's to assert. The scripted device ends a column's segment on that column's
// script alone and never changes a column that is not named in an operation's mask, which
// the checks assert. Covered: segments that end at different passes with the early ones
// idling, a column that converges at the first update while others go on, a bad column
// that falls back alone, two failed updates on one column only, the iteration limit per
// column, the forced fallback, K = 1 and K = 64. tol 1e-10, |phi| = 1 throughout. And the
// K-column chunk loop under the rounds (cg_chunked_columns, which the fp64 batched hosts
// run as well) on a fixed script, its chunk sizes as literals.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../schwingermodel_amd/csrc/sm_cg_host.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::string last_error;
int sm_host::fail(int code, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error = buf;
    return code;
}

using sm_host::ColMask;

struct Seg { int k, bad; };  // a segment ends after k iterations (bad: on a bad scalar)
struct Script {
    std::vector<double> true_r;
    std::vector<Seg> segs;
    int fp64_iterations = 17;
};

// One column's scripted device state and the log of what was done to it.
struct Column {
    Script s;
    sm::MPScalars h{};
    sm_cg_mixed_info info{};
    size_t n_true = 0, n_seg = 0;
    long first_pass = 0;  // the round's pass count when the running segment began
    int k_before = 0;
    std::vector<std::string> log;

    void true_residual(double tol, int max_iter, bool init, bool restart) {
        log.push_back(restart ? "true restart" : "true");
        CHECK(n_true < s.true_r.size());
        const double t = n_true < s.true_r.size() ? s.true_r[n_true] : 0.0;
        ++n_true;
        if (init) h.phi_norm = 1.0, h.k_total = 0;
        h.true_rr = t * t;
        h.err = h.M = t;
        h.k = h.bad = 0;
        h.done = t < tol * h.phi_norm || h.k_total >= max_iter || !(t == t);
    }
    void inject() {
        log.push_back("inject");
        CHECK(n_seg < s.segs.size());
        ++n_seg;
        k_before = h.k_total;
    }
    // p passes complete p - 1 iterations; the device ends the segment at k or at max_iter
    void advance(long issued, int max_iter) {
        if (h.done || n_seg == 0 || n_seg > s.segs.size()) return;  // an ended segment is not touched again
        const Seg &g = s.segs[n_seg - 1];
        long k = issued - 1;
        const long cap = std::min<long>(g.k, max_iter - k_before);
        h.done = k >= cap;
        if (k > cap) k = cap;
        h.k = (int)k;
        h.k_total = k_before + (int)k;
        h.bad = h.done && g.bad;
        h.err = h.M * std::pow(0.5, (double)k);
    }
    void fold(int discard) { log.push_back(discard ? "fold discard" : "fold " + std::to_string(h.k)); }
    void finish(double tol64, int iters, sm_cg_result *r64) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "solve64 %.17g %d", tol64, iters);
        log.push_back(buf);
        r64->iterations = s.fp64_iterations;
    }
};

// A one-column solver's operations (MixedColumn's Ops) on one Column: the script alone.
struct Vec { int dummy; };
struct Dir { int id; };
struct LoneOps {
    Column c;
    sm::MPScalars &h = c.h;
    sm_cg_mixed_info &info = c.info;
    Dir buf[3] = {{0}, {1}, {2}};
    Dir *d[3] = {&buf[0], &buf[1], &buf[2]};
    double tol = 1e-10, delta = 0.1;
    int max_iter = 1000, force_fallback = 0, debug = 0;
    const char *tag = "lone", *stuck = "the segment did not end";
    Vec rhs{0}, e{0};
    long issued = 0;
    double tol64 = 0.0;
    int iters64 = 0;

    void copy(const Vec *, Vec *) {}
    void add(Vec *, const Vec *) {}
    int true_residual(const Vec *, Vec *, bool init, bool restart) {
        c.true_residual(tol, max_iter, init, restart);
        return SM_OK;
    }
    void inject(const Vec *, Dir *, Dir *) {
        c.inject();
        issued = 0;
    }
    void pass(long, const Dir *, const Dir *, Dir *) { ++issued; }
    int check() { return SM_OK; }
    int read() {
        c.advance(issued, max_iter);
        return SM_OK;
    }
    void fold(Vec *, const Dir *, int discard) { c.fold(discard); }
    int finish_vectors(Vec **r, Vec **v) {
        *r = &rhs;
        *v = &e;
        return SM_OK;
    }
    int solve64(const Vec *, Vec *, double t, int it, sm_cg_result *r64) {
        c.finish(t, it, r64);
        return SM_OK;
    }
};

struct BatchOps {
    std::vector<Column> cols;
    double tol = 1e-10, delta = 0.1;
    int max_iter = 1000, force_fallback = 0, debug = 0;
    const char *tag = "batch", *stuck = "the segment did not end";
    long issued = 0;
    int reads = 0, rounds = 0;
    std::vector<ColMask> pass_masks;  // the mask of each round

    const sm::MPScalars &h(int b) const { return cols[(size_t)b].h; }
    sm_cg_mixed_info &info(int b) { return cols[(size_t)b].info; }
    template <class F>
    void each(ColMask m, F f) {
        for (size_t b = 0; b < cols.size(); ++b)
            if (m >> b & 1) f(cols[b]);
        CHECK(cols.size() == 64 || (m >> cols.size()) == 0);
    }
    void start() {}
    int true_residual(ColMask m, bool init, bool restart) {
        each(m, [&](Column &c) { c.true_residual(tol, max_iter, init, restart); });
        return SM_OK;
    }
    void inject(ColMask m) {
        each(m, [&](Column &c) { c.inject(); });
        issued = 0;
        ++rounds;
        pass_masks.push_back(m);
    }
    void pass(long j, ColMask m) {
        CHECK(j == issued && m == pass_masks.back());
        ++issued;
    }
    int check() { return SM_OK; }
    int read() {
        ++reads;
        each(pass_masks.back(), [&](Column &c) { c.advance(issued, max_iter); });
        return SM_OK;
    }
    void fold(ColMask m, ColMask discard) {
        CHECK(m == pass_masks.back() && (discard & ~m) == 0);
        for (size_t b = 0; b < cols.size(); ++b)
            if (m >> b & 1) cols[b].fold((int)(discard >> b & 1));
    }
    int finish(int b, double tol64, int iters, sm_cg_result *r64) {
        cols[(size_t)b].finish(tol64, iters, r64);
        return SM_OK;
    }
};

static bool same_bits(double a, double b) { return (a == b) || (a != a && b != b); }

// Drive the scripts as one batch and each alone; every column must come out the same.
static BatchOps compare(const std::vector<Script> &scripts, int max_iter = 1000, int force_fallback = 0) {
    const int K = (int)scripts.size();
    BatchOps o;
    o.max_iter = max_iter;
    o.force_fallback = force_fallback;
    for (const Script &s : scripts) {
        Column c;
        c.s = s;
        o.cols.push_back(c);
    }
    std::vector<sm_cg_result> res((size_t)K);
    CHECK(sm_host::cg_mixed_drive(o, K, res.data()) == SM_OK);
    for (int b = 0; b < K; ++b) {
        LoneOps l;
        l.c.s = scripts[(size_t)b];
        l.max_iter = max_iter;
        l.force_fallback = force_fallback;
        Vec phi{0}, x{0}, r{0};
        sm_cg_result lr{};
        CHECK(sm_host::cg_mixed_drive(l, &phi, &x, &r, &lr) == SM_OK);
        const Column &c = o.cols[(size_t)b];
        const bool log_same = c.log == l.c.log;
        CHECK(log_same);
        if (!log_same) {
            std::fprintf(stderr, "column %d of %d, batch | alone:\n", b, K);
            for (size_t i = 0; i < std::max(c.log.size(), l.c.log.size()); ++i)
                std::fprintf(stderr, "  %-40s | %s\n", i < c.log.size() ? c.log[i].c_str() : "",
                             i < l.c.log.size() ? l.c.log[i].c_str() : "");
        }
        const sm_cg_mixed_info &p = c.info, &q = l.c.info;
        CHECK(p.used == 1 && q.used == 1);
        CHECK(p.inner_iterations == q.inner_iterations && p.reliable_updates == q.reliable_updates);
        CHECK(p.fp64_iterations == q.fp64_iterations && p.fell_back == q.fell_back);
        CHECK(same_bits(p.true_residual, q.true_residual));
        CHECK(res[(size_t)b].converged == lr.converged && res[(size_t)b].iterations == lr.iterations);
        CHECK(same_bits(res[(size_t)b].residual, lr.residual) && res[(size_t)b].phi_norm == lr.phi_norm);
        CHECK(c.n_true == l.c.n_true && c.n_seg == l.c.n_seg);
    }
    return o;
}

static int count(const Column &c, const char *what) {
    int n = 0;
    for (const std::string &s : c.log) n += s.rfind(what, 0) == 0;
    return n;
}

static void check_idling() {  // segments of 3, 40 and 11 iterations in one round, then 9, 2 and 30
    Script a{{1, 1e-3, 1e-11}, {{3, 0}, {9, 0}}}, b{{1, 1e-4, 1e-11}, {{40, 0}, {2, 0}}},
        c{{1, 1e-2, 1e-11}, {{11, 0}, {30, 0}}};
    BatchOps o = compare({a, b, c});
    CHECK(o.rounds == 2 && o.pass_masks[0] == 7 && o.pass_masks[1] == 7);
    CHECK(o.cols[0].log == (std::vector<std::string>{"true restart", "inject", "fold 3", "true", "inject", "fold 9", "true"}));
    CHECK(o.cols[1].info.inner_iterations == 42 && o.cols[2].info.inner_iterations == 41);
}

static void check_early_convergence() {  // column 1 passes the stop test at its first update
    Script a{{1, 1e-3, 1e-6, 1e-11}, {{5, 0}, {6, 0}, {7, 0}}}, b{{1, 1e-12}, {{8, 0}}}, c{{1e-12}, {}};
    BatchOps o = compare({a, b, c});
    CHECK(o.rounds == 3 && o.pass_masks[0] == 3 && o.pass_masks[1] == 1 && o.pass_masks[2] == 1);
    CHECK(o.cols[1].info.reliable_updates == 1 && o.cols[1].info.inner_iterations == 8);
    CHECK(o.cols[2].info.reliable_updates == 0 && o.cols[2].log.size() == 1);  // never opened
    CHECK(o.cols[1].h.k_total == 8);  // frozen while column 0 ran two more rounds
}

static void check_bad_column_alone() {
    Script a{{1, 1e-3, 1e-11}, {{6, 0}, {9, 0}}}, bad{{1, 0.1, 1e-11}, {{6, 0}, {3, 1}}}, c{{1, 1e-5, 1e-11}, {{20, 0}, {4, 0}}};
    BatchOps o = compare({a, bad, c});
    CHECK(o.cols[1].info.fell_back == 1 && o.cols[1].info.fp64_iterations == 17 && o.cols[1].info.reliable_updates == 1);
    CHECK(count(o.cols[1], "fold discard") == 1 && count(o.cols[1], "solve64") == 1);
    CHECK(o.cols[1].log.back() == "true restart");
    CHECK(o.cols[0].info.fell_back == 0 && o.cols[2].info.fell_back == 0);
    CHECK(count(o.cols[0], "solve64") == 0 && count(o.cols[2], "solve64") == 0);
    // bad at the very first pass of the very first segment, next to a NaN true residual
    Script first{{1, 1e-11}, {{0, 1}}}, nan{{1, std::nan("")}, {{5, 0}}};
    BatchOps p = compare({first, nan, a});
    CHECK(p.cols[0].info.fell_back == 1 && p.cols[0].info.reliable_updates == 0 && p.cols[0].info.inner_iterations == 0);
    CHECK(p.cols[1].info.fell_back == 0 && count(p.cols[1], "solve64") == 0);
}

static void check_two_failed_updates_on_one_column() {
    Script ok{{1, 0.5, 0.25, 0.1, 1e-11}, {{5, 0}, {5, 0}, {5, 0}, {5, 0}}};
    Script stuck{{1, 0.5, 0.6, 0.7, 1e-11}, {{5, 0}, {6, 0}, {7, 0}}};
    Script recovers{{1, 0.5, 0.6, 0.3, 0.4, 1e-11}, {{5, 0}, {5, 0}, {5, 0}, {5, 0}, {5, 0}}};
    BatchOps o = compare({ok, stuck, recovers});
    CHECK(o.cols[1].info.reliable_updates == 3 && o.cols[1].info.fell_back == 1);
    CHECK(o.cols[1].info.inner_iterations == 18 && count(o.cols[1], "solve64") == 1);
    char want[96];
    std::snprintf(want, sizeof want, "solve64 %.17g %d", 1e-10 * 1.0 / 0.7, 1000 - 18);
    CHECK(o.cols[1].log[o.cols[1].log.size() - 2] == want);
    CHECK(o.cols[0].info.fell_back == 0 && o.cols[2].info.fell_back == 0 && o.cols[2].info.reliable_updates == 5);
}

static void check_max_iter_per_column() {
    Script a{{1, 0.2}, {{50, 0}}}, b{{1, 1e-3, 1e-11}, {{3, 0}, {2, 0}}}, c{{1, 0.5, 0.3}, {{4, 0}, {50, 0}}};
    BatchOps o = compare({a, b, c}, 7);
    CHECK(o.cols[0].info.inner_iterations == 7 && o.cols[1].info.inner_iterations == 5 && o.cols[2].info.inner_iterations == 7);
    // the forced fallback, with iterations left and with none
    Script f{{1, 0.2, 0.05}, {{4, 0}}};
    BatchOps p = compare({a, f}, 7, 1);
    CHECK(p.cols[1].info.fell_back == 1 && count(p.cols[1], "solve64 ") == 1 && p.cols[0].info.fell_back == 0);
    Script g{{1, 0.2}, {{7, 1}}};  // bad at the limit: fell_back is reported, no fp64 solve
    BatchOps q = compare({g, b}, 7);
    CHECK(q.cols[0].info.fell_back == 1 && count(q.cols[0], "solve64") == 0 && count(q.cols[0], "fold discard") == 1);
}

static void check_k1_and_k64() {
    Script a{{1, 1e-4, 1e-11}, {{9, 0}, {14, 0}}};
    BatchOps o = compare({a});
    CHECK(o.cols[0].info.inner_iterations == 23 && o.cols[0].info.reliable_updates == 2);
    std::vector<Script> many;
    for (int b = 0; b < 64; ++b) many.push_back(Script{{1, 1e-4, 1e-11}, {{1 + b, 0}, {70 - b, b == 63}}});
    BatchOps p = compare(many);
    CHECK(p.pass_masks[0] == ~(ColMask)0 && p.cols[63].info.fell_back == 1 && p.cols[62].info.fell_back == 0);
    std::vector<sm_cg_result> res(65);
    BatchOps z;
    CHECK(sm_host::cg_mixed_drive(z, 0, res.data()) == SM_ERR_ARG);
    CHECK(sm_host::cg_mixed_drive(z, 65, res.data()) == SM_ERR_ARG);
}

static void check_endless_segment() {  // a device that never ends a segment is an error, not a hang
    struct Endless : BatchOps {
        int read() {
            ++reads;
            return SM_OK;
        }
    } o;
    o.max_iter = 40;
    Column c;
    c.s = Script{{1}, {{5, 0}}};
    o.cols.push_back(c);
    sm_cg_result res{};
    CHECK(sm_host::cg_mixed_drive(o, 1, &res) == SM_ERR_STATE);
    CHECK(last_error == o.stuck && o.issued == 41);
}

// The K-column chunk loop itself (cg_chunked_columns), driven directly: three columns whose
// residuals fall at 0.5, at 0.6 then 0.9 from k = 10, and at 0.8 then 0.97 from k = 12, to the
// target 1e-3, which they pass at k = 10, 28 and 151: a column is done from pass k + 1 on. The
// chunk sizes are literals from a separate copy of the hosts' loop run on this script, not
// from cg_chunked_columns: 4, then 8 (no rate yet), then the slowest running column's wish.
static void check_chunk_loop() {
    auto err = [](int b, int k) {
        const double r1[3] = {0.5, 0.6, 0.8}, r2[3] = {0.5, 0.9, 0.97};
        const int kink[3] = {10, 10, 12};
        return k <= kink[b] ? std::pow(r1[b], (double)k) : std::pow(r1[b], (double)kink[b]) * std::pow(r2[b], (double)(k - kink[b]));
    };
    const int kend[3] = {10, 28, 151};
    for (int b = 0; b < 3; ++b) CHECK(err(b, kend[b]) < 1e-3 && err(b, kend[b] - 1) >= 1e-3);
    std::vector<long> chunks, reads;
    long passes = 0;
    bool ended = false;
    int last_running = -1;
    CHECK(sm_host::cg_chunked_columns(
              3, 1001,
              [&](long j, long nb) {
                  CHECK(j == passes);
                  passes += nb;
                  chunks.push_back(nb);
                  return SM_OK;
              },
              [&](long issued) {
                  CHECK(issued == passes);
                  reads.push_back(issued);
                  return SM_OK;
              },
              [&](int b) {
                  const int k = (int)std::min<long>(passes - 1, kend[b]);
                  return sm_host::CgStatus{k, err(b, k), 1e-3, passes - 1 >= kend[b]};
              },
              [&](long issued, int running, int) {
                  CHECK(issued == passes);
                  last_running = running;
              },
              &ended) == SM_OK);
    CHECK(chunks == (std::vector<long>{4, 8, 22, 98, 22}));
    CHECK(reads == (std::vector<long>{4, 12, 34, 132, 154}));
    CHECK(ended && last_running == 0);
    // the limit ends the loop with columns running: the last chunk is cut, *ended is false
    chunks.clear();
    passes = 0;
    CHECK(sm_host::cg_chunked_columns(
              3, 40, [&](long, long nb) { passes += nb; chunks.push_back(nb); return SM_OK; }, [&](long) { return SM_OK; },
              [&](int b) {
                  const int k = (int)std::min<long>(passes - 1, kend[b]);
                  return sm_host::CgStatus{k, err(b, k), 1e-3, passes - 1 >= kend[b]};
              },
              [&](long, int running, int) { last_running = running; }, &ended) == SM_OK);
    CHECK(chunks == (std::vector<long>{4, 8, 22, 6}));
    CHECK(!ended && last_running == 1);
}

int main() {
    check_chunk_loop();
    check_idling();
    check_early_convergence();
    check_bad_column_alone();
    check_two_failed_updates_on_one_column();
    check_max_iter_per_column();
    check_k1_and_k64();
    check_endless_segment();
    if (failures) {
        std::fprintf(stderr, "batch_mixed_driver_check: %d failures\n", failures);
        return 1;
    }
    std::printf("batch_mixed_driver_check ok\n");
    return 0;
}
