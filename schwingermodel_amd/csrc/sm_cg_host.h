// sm_cg_host.h -- the control flow the CG hosts share, free of any device call
// and of every HIP header so that tools/mixed_driver_check.cpp and
// tools/batch_mixed_driver_check.cpp can run it under the host sanitizers: the
// chunk planner of every CG host, the chunked status loop of the fp64
// one-column ones (cg_chunked) and of every K-column host
// (cg_chunked_columns), and the reliable-update driver of the three mixed-precision
// solvers (sm_cgmp.cpp, sm_eomp.cpp, sm_cgbatchmp.cpp), which is described
// here and nowhere else: one loop on K columns, and MixedColumn, which hands it
// a one-column solver's operations as K = 1.
#pragma once
#include "../../include/sm_hip.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace sm {

// Device-resident scalars of a mixed solve: a segment of fp32 inner iterations
// between two fp64 true residuals (reliable updates). alpha and beta are real.
struct MPScalars {
    double alpha, beta;      // alpha_j, beta_j after pass j's scalar step (beta: the injection's before pass 0)
    double alpha2, beta2;    // those of the pass before
    double rn;               // iterated |r|^2 of the previous iteration
    double err;              // iterated |r| of the last iteration
    double M;                // largest iterated |r| since the segment began (starts at the true |r|)
    double phi_norm, tol, delta;
    double true_rr, phi_rr;  // |phi - D D^dag x|^2 (fp64) of the last update, |phi|^2
    int k;                   // inner iterations of this segment
    int k_total;             // inner iterations of the solve
    int max_iter;            // bound on k_total
    int done;                // the segment is over: every later pass and scalar step is a no-op
    int bad;                 // it ended on a non-finite scalar (or <d,Ad> <= 0)
    int k_last;              // k of the segment before this one (the batched injection finds d_prev in ring slot (k_last - 1) mod 3)
};

}  // namespace sm

namespace sm_host {

int fail(int code, const char *fmt, ...);

#define TRY(expr)                     \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != SM_OK) return rc_; \
    } while (0)

// How many CG iterations to enqueue before the next status read. Kernels are
// no-ops once the device's `done` flag is set, so queueing past convergence
// costs empty launches and every status read costs a host round trip: predict
// the iterations left to the stop test from the residual's observed geometric
// rate, and stay a few percent past it.
struct CgChunker {
    int chunk = 4;
    int k_prev = -1;
    double err_prev = 0.0;
    int next(int k, double err, double target) {
        int c = chunk < 64 ? 2 * chunk : 64;
        if (k_prev >= 0 && k > k_prev && err_prev > 0.0 && err > 0.0 && err < err_prev && target > 0.0) {
            const double rate = std::pow(err / err_prev, 1.0 / (k - k_prev));
            if (rate < 1.0) {
                const double left = std::log(target / err) / std::log(rate);
                c = left <= 0.0 ? 2 : (int)std::ceil(left * 1.05) + 1;
                c = c < 2 ? 2 : (c > 256 ? 256 : c);
            }
        }
        k_prev = k;
        err_prev = err;
        chunk = c;
        return c;
    }
};

// What a status read tells the planner: iterations done, the residual, what it
// must reach, and whether the solve (or segment) is over.
struct CgStatus {
    int k;
    double err, target;
    int done;
};

// The chunked status loop of a CG host: up to `limit` passes, enqueued by
// issue(nb) in chunks the planner sizes, each followed by the caller's own
// read-back status(&st) -- whatever it launches, copies, waits for and prints
// between a chunk's last pass and the read. Stops at st.done; *done (nullable)
// says whether that was seen before the limit.
template <class Issue, class Status>
int cg_chunked(long limit, Issue issue, Status status, bool *done = nullptr) {
    CgChunker plan;
    int chunk = plan.chunk;
    CgStatus st{};
    for (long issued = 0; issued < limit && !st.done;) {
        const long nb = (limit - issued) < chunk ? (limit - issued) : chunk;
        TRY(issue(nb));
        issued += nb;
        TRY(status(&st));
        if (!st.done) chunk = plan.next(st.k, st.err, st.target);
    }
    if (done) *done = st.done != 0;
    return SM_OK;
}

// The same loop on K columns that stop one by one, the only copy: the fp64
// batched hosts (sm_ctx.h batch_cg_solve) and cg_mixed_drive's rounds run it.
// Up to `limit` passes in chunks that start at 4: issue(j, nb) enqueues passes
// j .. j + nb - 1, read(issued) is the caller's read-back of all K states with
// whatever it launches before it, status(b) column b's CgStatus (done: it is
// over, or not part of this loop). One CgChunker per column; of the columns
// still running the longest wish wins, 2 at the least. debug(issued, running,
// wish) is the caller's line after each read. Stops when no column runs or at
// the limit; *ended (nullable) says whether every column was seen done. With
// K = 1 the chunks are cg_chunked's.
template <class Issue, class Read, class Status, class Debug>
int cg_chunked_columns(int K, long limit, Issue issue, Read read, Status status, Debug debug, bool *ended = nullptr) {
    std::vector<CgChunker> plan((size_t)K);
    int chunk = CgChunker().chunk, running = 1;
    for (long issued = 0; issued < limit && running;) {
        const long nb = limit - issued < chunk ? limit - issued : chunk;
        TRY(issue(issued, nb));
        issued += nb;
        TRY(read(issued));
        running = 0;
        int wish = 2;
        for (int b = 0; b < K; ++b) {
            const CgStatus st = status(b);
            if (st.done) continue;
            ++running;
            const int w = plan[(size_t)b].next(st.k, st.err, st.target);
            if (w > wish) wish = w;
        }
        debug(issued, running, wish);
        chunk = wish;
    }
    if (ended) *ended = !running;
    return SM_OK;
}

// The reliable-update driver of the mixed-precision solvers, on operator A
// (D D^dag or Dhat Dhat^dag) and K <= 64 columns, each a solve of its own:
//
//   x = phi; r = phi - A x in fp64; M = |r|
//   segment: d_0 = fp32(r) + beta d_prev (first: beta = 0), y = 0, fp32 passes
//       on y until the iterated |r| < delta M (M: the largest iterated |r| of
//       the segment) or < tol |phi| -- decided on the device, read by the host
//       in chunks
//   reliable update: x += y (+ the pending alpha_{J-1} d_{J-1}), y = 0,
//       r = phi - A x in fp64; stop if |r| < tol |phi|; else beta = |r|^2 /
//       (the last iteration's iterated |r_{J-1}|^2) and the next segment
//       starts from d_{J-1}: the search direction survives the replacement of
//       the residual, so the updates cost almost no extra iterations (a
//       restarted defect correction costs 20-50 % more on these operators).
// A column stops only on an fp64 true residual. Two consecutive updates that
// fail to lower it, or a non-finite fp32 scalar, hand the rest of that column
// to the fp64 solver: A e = r with its own x0 = r convention, x += e.
//
// The columns go in rounds: inject for the open columns, passes in chunks until
// every open column's segment has ended (cg_chunked_columns, all K scalar
// blocks read once per chunk: with K = 1 the sequence of cg_chunked), fold,
// one true residual for the open columns, then the
// decisions column by column. A column whose segment ended early idles until
// the round is over; a column that has stopped, or is marked for the fp64
// finish, is closed: nothing of it is touched again before the finishes, which
// run one column at a time after the rounds. Every column therefore takes the
// decisions it would take alone.
//
// Columns are named by bit masks (bit b = column b). Ops supplies every device
// call, and alone knows which solver it serves:
//   h(b), info(b)            column b's scalars (host mirror) and report
//   tol, max_iter, delta, force_fallback, debug, tag, stuck
//   start()                  x = phi, every column
//   true_residual(m, init, restart)   r_b = phi_b - A x_b and its scalars for b in m, all K mirrors read back
//                            (init: the solve's first true residual)
//   inject(m)                d_0 = fp32(r) + beta d_prev
//   pass(j, m)               pass j of the round and its scalar step
//   check(), read()          the launches' error state; that and all K scalar blocks into the mirrors
//   fold(m, discard)         x += y, y = 0 for b in m (b in discard: y = 0 only)
//   finish(b, tol, iters, &res)   the fp64 finish of column b: A e = r_b, x_b += e
typedef unsigned long long ColMask;

template <class Ops>
int cg_mixed_drive(Ops &o, int K, sm_cg_result *res) {
    struct Col {
        int fails = 0;
        double prev_true = 0.0;
        bool fallback = false;
    };
    if (K < 1 || K > 64) return fail(SM_ERR_ARG, "%s: K = %d outside 1..64", o.tag, K);
    const double tol = o.tol;
    const int max_iter = o.max_iter;
    std::vector<Col> col((size_t)K);
    for (int b = 0; b < K; ++b) {
        o.info(b) = sm_cg_mixed_info{};
        o.info(b).used = 1;
    }
    auto bit = [](int b) { return (ColMask)1 << b; };
    ColMask open = K == 64 ? ~(ColMask)0 : bit(K) - 1;
    o.start();
    TRY(o.true_residual(open, true, true));
    for (;;) {
        for (int b = 0; b < K; ++b) {  // what each open column's last true residual decides
            if (!(open & bit(b))) continue;
            const sm::MPScalars &h = o.h(b);
            sm_cg_mixed_info &info = o.info(b);
            Col &c = col[(size_t)b];
            const double true_err = std::sqrt(h.true_rr);
            if (o.debug)
                fprintf(stderr, "[%s] column %d update %d inner %d true %.3e (target %.3e)\n", o.tag, b,
                        info.reliable_updates, h.k_total, true_err, tol * h.phi_norm);
            if (info.reliable_updates > 0) c.fails = true_err < c.prev_true ? 0 : c.fails + 1;
            c.prev_true = true_err;
            if (!(true_err == true_err) || true_err < tol * h.phi_norm || h.k_total >= max_iter) {
                open &= ~bit(b);
            } else if (c.fails >= 2 || (o.force_fallback && info.reliable_updates >= 1)) {
                c.fallback = true;
                open &= ~bit(b);
            }
        }
        if (!open) break;
        o.inject(open);
        long limit = 0;  // every column stops itself at its own max_iter
        for (int b = 0; b < K; ++b)
            if ((open & bit(b)) && (long)(max_iter - o.h(b).k_total) + 1 > limit) limit = (long)(max_iter - o.h(b).k_total) + 1;
        bool ended = false;
        TRY(cg_chunked_columns(
            K, limit,
            [&](long j, long nb) {
                for (long i = 0; i < nb; ++i) o.pass(j + i, open);
                return SM_OK;
            },
            [&](long) { return o.read(); },
            [&](int b) {
                const sm::MPScalars &h = o.h(b);
                return CgStatus{h.k, h.err, std::fmax(o.delta * h.M, tol * h.phi_norm), !(open & bit(b)) || h.done};
            },
            [&](long j, int running, int wish) {
                if (o.debug) fprintf(stderr, "[%s]   passes %ld running %d next chunk %d\n", o.tag, j, running, wish);
            },
            &ended));
        if (!ended) return fail(SM_ERR_STATE, "%s", o.stuck);
        ColMask bad = 0;
        for (int b = 0; b < K; ++b) {
            if (!(open & bit(b))) continue;
            const sm::MPScalars &h = o.h(b);
            o.info(b).inner_iterations = h.k_total;
            if (h.bad) {  // y is not trusted, x and r are those of the last update
                bad |= bit(b);
                col[(size_t)b].fallback = true;
            } else {
                o.info(b).reliable_updates++;
            }
        }
        o.fold(open, bad);
        if (bad) TRY(o.check());
        open &= ~bad;
        if (open) TRY(o.true_residual(open, false, false));
    }
    for (int b = 0; b < K; ++b) {
        const sm::MPScalars &h = o.h(b);
        sm_cg_mixed_info &info = o.info(b);
        info.inner_iterations = h.k_total;
        double true_err = std::sqrt(h.true_rr);
        const double phi_norm = h.phi_norm;
        if (col[(size_t)b].fallback && h.k_total < max_iter && true_err > 0.0) {
            sm_cg_result r64{};
            const int inner = h.k_total;
            TRY(o.finish(b, tol * phi_norm / true_err, max_iter - h.k_total, &r64));
            info.fell_back = 1;
            info.fp64_iterations = r64.iterations;
            TRY(o.true_residual(bit(b), false, true));
            info.inner_iterations = inner;
            true_err = std::sqrt(h.true_rr);
        } else if (col[(size_t)b].fallback) {
            info.fell_back = 1;
        }
        info.true_residual = phi_norm > 0.0 ? true_err / phi_norm : true_err;
        res[b].converged = true_err < tol * phi_norm ? 1 : 0;
        res[b].iterations = info.inner_iterations + info.fp64_iterations;
        res[b].residual = true_err;
        res[b].phi_norm = phi_norm;
    }
    return SM_OK;
}

// A one-column solver's operations as the driver's K = 1 column set. The
// wrapped Ops (sm_ctx.h MixedDev and what sm_cgmp.cpp / sm_eomp.cpp add):
//   h, info, d[3]            the scalars' host mirror, the solve's report, the direction buffers
//   tol, max_iter, delta, force_fallback, debug, tag, stuck
//   copy(a, b), add(x, e)    b = a, x += e in fp64
//   true_residual(x, r, init, restart)   r = phi - A x, its scalars into h
//   inject(r, dprev, d0)     d0 = fp32(r) + beta dprev
//   pass(j, d1, d2, dn)      pass j of the segment and its scalar step
//   check(), read()          the launches' error state; that and the scalars into h
//   fold(x, dlast, discard)  the reliable update's x += y, y = 0 (discard: y = 0 only)
//   finish_vectors(&rhs, &e), solve64(rhs, e, tol, max_iter, &res)   the fp64 finish
// The three direction buffers rotate by pointer: d_i of the running segment
// lives in d[(base + i) mod 3], i >= -1.
template <class Ops, class Vec>
struct MixedColumn {
    Ops &o;
    const Vec *phi;
    Vec *x, *r;
    int base = 0;
    double tol = o.tol, delta = o.delta;
    int max_iter = o.max_iter, force_fallback = o.force_fallback, debug = o.debug;
    const char *tag = o.tag, *stuck = o.stuck;

    auto dbuf(long i) const { return o.d[(((base + i) % 3) + 3) % 3]; }
    const sm::MPScalars &h(int) const { return o.h; }
    sm_cg_mixed_info &info(int) { return o.info; }
    void start() {
        if (x != phi) o.copy(phi, x);
    }
    int true_residual(ColMask, bool init, bool restart) { return o.true_residual(x, r, init, restart); }
    void inject(ColMask) { o.inject(r, dbuf(-1), dbuf(0)); }
    void pass(long j, ColMask) {  // passes 0 and 1 both read d_0 and d_{-1}; pass 0 stores no d
        o.pass(j, j == 0 ? dbuf(0) : dbuf(j - 1), j == 0 ? dbuf(-1) : dbuf(j - 2), dbuf(j));
    }
    int check() { return o.check(); }
    int read() { return o.read(); }
    void fold(ColMask, ColMask discard) {
        if (discard) return o.fold(x, dbuf(0), 1);
        const int J = o.h.k;
        o.fold(x, dbuf(J - 1), 0);
        base = (base + J) % 3;  // d_{J-1} becomes the next segment's d_{-1}, d_J's buffer takes its d_0
    }
    int finish(int, double tol64, int iters, sm_cg_result *r64) {  // r kept apart: the fp64 solver's own buffers may include it
        Vec *rhs, *e;
        TRY(o.finish_vectors(&rhs, &e));
        o.copy(r, rhs);
        TRY(o.solve64(rhs, e, tol64, iters, r64));
        o.add(x, e);
        return SM_OK;
    }
};

template <class Ops, class Vec>
int cg_mixed_drive(Ops &o, const Vec *phi, Vec *x, Vec *r, sm_cg_result *res) {
    MixedColumn<Ops, Vec> col{o, phi, x, r};
    return cg_mixed_drive(col, 1, res);
}

}  // namespace sm_host
