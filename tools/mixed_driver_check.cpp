// mixed_driver_check.cpp -- the decisions of the mixed-precision solvers' reliable-update
// driver (csrc/sm_cg_host.h cg_mixed_drive) on one column, as the one-column solvers reach
// it (through MixedColumn), under the host sanitizers: no device, the operations are a script.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/mixed_driver_check.cpp -o build/mixed_driver_check && build/mixed_driver_check
//
// The scripted operations take the fp64 true residuals and each segment's k, done and bad
// from lists, hand out three tagged direction buffers and log every call. Covered: the
// plain solve, the two-failed-updates fallback and what the fp64 finish is given, the bad
// segment, the iteration limit in a segment and after a forced fallback, the NaN true
// residual, the segment that never ends, the buffer rotation across segments of lengths
// 1, 2, 4, 5, and the start in place (x == phi: no copy). tol 1e-10, |phi| = 1 throughout.
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

struct Vec { const char *name; };  // an fp64 vector
struct Dir { int id; };            // a direction buffer
struct Seg { int k, bad, never; }; // a segment ends after k iterations (bad: on a bad scalar; never: not at all)
struct Pass { long j; int d1, d2, dn; };
struct Segment { int dprev, d0, dlast, discard; std::vector<Pass> passes; };  // dlast < 0: not folded

struct Ops {
    // what the driver reads
    sm::MPScalars h{};
    sm_cg_mixed_info info{};
    Dir buf[3] = {{0}, {1}, {2}};
    Dir *d[3] = {&buf[0], &buf[1], &buf[2]};
    double tol = 1e-10, delta = 0.1;
    int max_iter = 1000, force_fallback = 0, debug = 0;
    const char *tag = "check", *stuck = "the segment did not end";
    // the script
    std::vector<double> true_r;
    std::vector<Seg> segs;
    int fp64_iterations = 17;
    // the log
    Vec rhs{"rhs"}, e{"e"};
    std::vector<std::string> calls;
    std::vector<Segment> seg_log;
    size_t n_true = 0;
    long issued = 0;
    int k_before = 0;
    const Vec *rhs_from = nullptr, *solved = nullptr, *added = nullptr;
    double tol64 = 0.0;
    int iters64 = -1, restarts = 0;

    void copy(const Vec *a, Vec *b) {
        calls.push_back(std::string("copy ") + a->name + " " + b->name);
        if (b == &rhs) rhs_from = a;
    }
    void add(Vec *x, const Vec *v) {
        calls.push_back(std::string("add ") + x->name + " " + v->name);
        added = v;
    }
    int true_residual(const Vec *, Vec *, bool init, bool restart) {
        calls.push_back(restart ? "true restart" : "true");
        CHECK(n_true < true_r.size());
        const double t = true_r[n_true++];
        if (init) h.phi_norm = 1.0, h.k_total = 0;
        if (restart && !init) ++restarts, h.k_total += 1000;  // the driver keeps its own count over the finish
        h.true_rr = t * t;
        h.err = h.M = t;
        h.k = h.bad = 0;
        h.done = t < tol * h.phi_norm || h.k_total >= max_iter || !(t == t);
        return SM_OK;
    }
    void inject(const Vec *, Dir *dprev, Dir *d0) {
        calls.push_back("inject");
        CHECK(seg_log.size() < segs.size());
        seg_log.push_back(Segment{dprev->id, d0->id, -1, 0, {}});
        issued = 0;
        k_before = h.k_total;
    }
    void pass(long j, const Dir *d1, const Dir *d2, Dir *dn) {
        CHECK(j == issued);
        seg_log.back().passes.push_back(Pass{j, d1->id, d2->id, dn->id});
        ++issued;
    }
    int check() { return SM_OK; }
    int read() {  // p passes complete p - 1 iterations; the device ends the segment at k or at max_iter
        calls.push_back("read");
        const Seg &s = segs[seg_log.size() - 1];
        long k = issued - 1;
        const long cap = s.never ? k : std::min<long>(s.k, max_iter - k_before);
        h.done = !s.never && k >= cap;
        if (k > cap) k = cap;
        h.k = (int)k;
        h.k_total = k_before + (int)k;
        h.bad = h.done && s.bad;
        h.err = h.M * std::pow(0.5, (double)k);
        return SM_OK;
    }
    void fold(Vec *, const Dir *dlast, int discard) {
        calls.push_back(discard ? "fold discard" : "fold");
        seg_log.back().dlast = dlast->id;
        seg_log.back().discard = discard;
    }
    int finish_vectors(Vec **r, Vec **v) {
        *r = &rhs;
        *v = &e;
        return SM_OK;
    }
    int solve64(const Vec *b, Vec *, double t, int it, sm_cg_result *r64) {
        calls.push_back("solve64");
        solved = b;
        tol64 = t;
        iters64 = it;
        r64->iterations = fp64_iterations;
        return SM_OK;
    }
    int count(const char *what) const {
        int n = 0;
        for (const std::string &c : calls) n += c == what;
        return n;
    }
};

static Vec phi{"phi"}, x{"x"}, r{"r"};

static int run(Ops &o, sm_cg_result *res) {
    *res = sm_cg_result{};
    return sm_host::cg_mixed_drive(o, &phi, &x, &r, res);
}

static void check_plain() {  // 1
    Ops o;
    o.true_r = {1, 1e-4, 1e-11};
    o.segs = {{9, 0, 0}, {14, 0, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    CHECK(o.calls.front() == "copy phi x");
    CHECK(o.info.used == 1 && o.info.reliable_updates == 2 && o.info.fell_back == 0 && o.info.fp64_iterations == 0);
    CHECK(res.converged == 1 && res.iterations == 23 && o.info.inner_iterations == 23);
    CHECK(res.residual == 1e-11 && res.phi_norm == 1.0 && o.info.true_residual == 1e-11);
    CHECK(o.count("solve64") == 0 && o.count("fold") == 2 && o.count("true") == 2 && o.count("true restart") == 1);
}

static void check_two_failed_updates() {  // 2
    Ops o;
    o.true_r = {1, 0.5, 0.6, 0.7, 1e-11};
    o.segs = {{5, 0, 0}, {6, 0, 0}, {7, 0, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    CHECK(o.info.reliable_updates == 3);  // the counter reaches 2 at the third update, not before
    CHECK(o.seg_log.size() == 3);
    CHECK(o.rhs_from == &r && o.solved == &o.rhs && o.added == &o.e);
    CHECK(o.tol64 == 1e-10 * 1.0 / 0.7 && o.iters64 == 1000 - 18);
    CHECK(o.info.fell_back == 1 && o.info.fp64_iterations == 17);
    CHECK(o.restarts == 1 && o.calls.back() == "true restart");
    CHECK(o.info.inner_iterations == 18 && res.iterations == 18 + 17);
    CHECK(res.converged == 1 && res.residual == 1e-11);
    // an update that lowers the residual again resets the counter
    Ops p;
    p.true_r = {1, 0.5, 0.6, 0.3, 0.4, 1e-11};
    p.segs = {{5, 0, 0}, {5, 0, 0}, {5, 0, 0}, {5, 0, 0}, {5, 0, 0}};
    CHECK(run(p, &res) == SM_OK);
    CHECK(p.info.reliable_updates == 5 && p.info.fell_back == 0 && p.count("solve64") == 0);
}

static void check_bad_segment() {  // 3
    Ops o;
    o.true_r = {1, 0.1, 1e-11};
    o.segs = {{6, 0, 0}, {3, 1, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    CHECK(o.seg_log.size() == 2);
    CHECK(o.seg_log[1].discard == 1 && o.seg_log[1].dlast == o.seg_log[1].d0);  // y dropped, on dbuf(0)
    CHECK(o.info.reliable_updates == 1);
    CHECK(o.info.fell_back == 1 && o.count("solve64") == 1 && o.iters64 == 1000 - 9);
    CHECK(o.tol64 == 1e-10 * 1.0 / 0.1);
    CHECK(o.info.inner_iterations == 9 && res.iterations == 9 + 17 && res.converged == 1);
}

static void check_limit_in_segment() {  // 4
    Ops o;
    o.max_iter = 7;
    o.true_r = {1, 0.2};
    o.segs = {{50, 0, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    CHECK(o.info.reliable_updates == 1 && o.seg_log.size() == 1);
    CHECK(res.converged == 0 && res.iterations == 7 && res.residual == 0.2);
    CHECK(o.info.fell_back == 0 && o.count("solve64") == 0);
}

static void check_limit_after_forced_fallback() {  // 5
    Ops o;
    o.max_iter = 7;
    o.force_fallback = 1;
    o.true_r = {1, 0.2};
    o.segs = {{50, 0, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    // the limit is seen before the forced fallback: the loop ends on it
    CHECK(res.converged == 0 && res.iterations == 7 && o.count("solve64") == 0 && o.info.fell_back == 0);
    Ops p;  // the fallback is taken with iterations left ...
    p.max_iter = 7;
    p.force_fallback = 1;
    p.true_r = {1, 0.2, 0.05};
    p.segs = {{4, 0, 0}};
    CHECK(run(p, &res) == SM_OK);
    CHECK(p.info.fell_back == 1 && p.count("solve64") == 1 && p.iters64 == 3 && res.converged == 0);
    Ops q;  // ... and with none: fell_back is reported, no fp64 solve is started
    q.max_iter = 7;
    q.true_r = {1, 0.2};
    q.segs = {{7, 1, 0}};
    CHECK(run(q, &res) == SM_OK);
    CHECK(q.info.fell_back == 1 && q.count("solve64") == 0 && q.count("fold discard") == 1);
    CHECK(res.converged == 0 && res.iterations == 7 && q.info.reliable_updates == 0);
}

static void check_nan() {  // 6
    Ops o;
    o.true_r = {1, std::nan("")};
    o.segs = {{5, 0, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    CHECK(o.seg_log.size() == 1 && o.info.reliable_updates == 1);
    CHECK(res.converged == 0 && !(res.residual == res.residual));
    CHECK(o.info.fell_back == 0 && o.count("solve64") == 0);
}

static void check_endless_segment() {  // 7
    Ops o;
    o.max_iter = 40;
    o.true_r = {1, 0.3};
    o.segs = {{12, 0, 0}, {0, 0, 1}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_ERR_STATE);
    CHECK(last_error == o.stuck);
    CHECK(o.seg_log.size() == 2 && (long)o.seg_log[1].passes.size() == 40 - 12 + 1);
    CHECK(o.seg_log[1].dlast == -1);  // nothing folded
}

static void check_rotation() {  // 8
    Ops o;
    o.true_r = {1, 0.5, 0.25, 0.1, 0.05, 1e-11};
    o.segs = {{1, 0, 0}, {2, 0, 0}, {4, 0, 0}, {5, 0, 0}, {3, 0, 0}};
    sm_cg_result res;
    CHECK(run(o, &res) == SM_OK);
    CHECK(o.seg_log.size() == 5 && res.iterations == 15 && res.converged == 1);
    for (size_t s = 0; s < o.seg_log.size(); ++s) {
        const Segment &g = o.seg_log[s];
        const int J = o.segs[s].k;
        CHECK((int)g.passes.size() > J);  // pass J completes iteration J
        CHECK(g.dprev != g.d0);
        for (const Pass &p : g.passes) {
            for (int id : {p.d1, p.d2, p.dn}) CHECK(id >= 0 && id <= 2);
            if (p.j >= 2) CHECK(p.d1 != p.d2 && p.d1 != p.dn && p.d2 != p.dn);
            if (p.j >= 1) CHECK(p.d1 == g.passes[(size_t)p.j - 1].dn);  // d_{j-1}
            if (p.j >= 2) CHECK(p.d2 == g.passes[(size_t)p.j - 2].dn);  // d_{j-2}
        }
        // passes 0 and 1 read the injected pair; pass 0's own buffer is d_0's
        CHECK(g.passes[0].d1 == g.d0 && g.passes[0].d2 == g.dprev && g.passes[0].dn == g.d0);
        CHECK(g.passes[1].d1 == g.d0 && g.passes[1].d2 == g.dprev);
        CHECK(g.discard == 0 && g.dlast == g.passes[(size_t)J - 1].dn);  // the fold's d_{J-1}
        if (s + 1 < o.seg_log.size()) {
            CHECK(o.seg_log[s + 1].dprev == g.dlast);
            CHECK(o.seg_log[s + 1].d0 == g.passes[(size_t)J].dn);
        }
    }
}

static void check_in_place() {  // 9: x == phi starts without a copy, x != phi with exactly one
    Ops o;
    o.true_r = {1, 1e-4, 1e-11};
    o.segs = {{9, 0, 0}, {14, 0, 0}};
    sm_cg_result res{};
    CHECK(sm_host::cg_mixed_drive(o, &phi, &phi, &r, &res) == SM_OK);
    CHECK(o.count("copy phi phi") == 0 && o.calls.front() == "true restart");
    Ops p;
    p.true_r = o.true_r;
    p.segs = o.segs;
    sm_cg_result res2;
    CHECK(run(p, &res2) == SM_OK);
    CHECK(p.count("copy phi x") == 1 && p.calls.front() == "copy phi x");
    CHECK(std::vector<std::string>(p.calls.begin() + 1, p.calls.end()) == o.calls);  // nothing else differs
    CHECK(res.converged == 1 && res.iterations == res2.iterations && res.residual == res2.residual);
    CHECK(o.info.reliable_updates == 2 && o.info.inner_iterations == 23);
}

int main() {
    check_plain();
    check_two_failed_updates();
    check_bad_segment();
    check_limit_in_segment();
    check_limit_after_forced_fallback();
    check_nan();
    check_endless_segment();
    check_rotation();
    check_in_place();
    if (failures) {
        std::fprintf(stderr, "mixed_driver_check: %d failures\n", failures);
        return 1;
    }
    std::printf("mixed_driver_check ok\n");
    return 0;
}
