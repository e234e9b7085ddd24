// sm_cgmp.cpp -- mixed-precision CG on D D^dagger: fp32 inner iterations
// (sm_cgsp.hip) held to the fp64 stop test by reliable updates.
//
//   x = phi; r = phi - D D^dag x in fp64 (the existing apply); M = |r|
//   segment: d_0 = fp32(r) + beta d_prev (first: beta = 0), y = 0, fp32
//       two-direction passes on y until the iterated |r| < delta M (M: the
//       largest iterated |r| of the segment) or < tol |phi| -- decided on the
//       device, read by the host in chunks (CgChunker)
//   reliable update: x += y, y = 0, r = phi - D D^dag x in fp64; stop if
//       |r| < tol |phi|; else beta = |r|^2 / (the last iteration's iterated
//       |r_{J-1}|^2) and the next segment starts from d_{J-1}: the search
//       direction survives the replacement of the residual, so the updates
//       cost almost no extra iterations (a restarted defect correction costs
//       20-50 % more on this operator).
// The solve stops only on an fp64 true residual. Two consecutive updates that
// fail to lower it, or a non-finite fp32 scalar, hand the rest to the fp64
// solver: D D^dag e = r with its own x0 = r convention, x += e.
//
// One-shard contexts only (sm_cg_precision refuses the others). Everything the
// fp32 side touches is its own -- directions, y, links, partials, scalars --
// so the fp64 paths find their state as they left it.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

void cg_mixed_free(sm_ctx *c) {
    for (float2 *&d : c->mp_d) {
        stream_free(c, d);
        d = nullptr;
    }
    stream_free(c, c->mp_y);
    stream_free(c, c->mp_U);
    c->mp_y = c->mp_U = nullptr;
    if (c->mp_partials) (void)hipFree(c->mp_partials);
    if (c->mp_fb) (void)hipFree(c->mp_fb);
    if (c->mp_sc) (void)hipFree(c->mp_sc);
    if (c->mp_h_sc) (void)hipHostFree(c->mp_h_sc);
    c->mp_partials = c->mp_fb = nullptr;
    c->mp_sc = c->mp_h_sc = nullptr;
    c->mp_U_valid = false;
}

// The fp32 buffers, at the first mixed solve (placed like the fp64 pass's
// streamed buffers); the fp32 links again after every change of U.
static int mixed_ready(sm_ctx *c) {
    const size_t fb = sizeof(float2) * 2 * (size_t)c->g.V;
    if (!c->mp_sc) {
        for (float2 *&d : c->mp_d) HIP_TRY(stream_malloc(c, (void **)&d, fb));
        HIP_TRY(stream_malloc(c, (void **)&c->mp_y, fb));
        HIP_TRY(stream_malloc(c, (void **)&c->mp_U, fb));
        HIP_TRY(hipMalloc(&c->mp_partials, sizeof(double2) * 2 * (size_t)kMaxPartials));
        HIP_TRY(hipHostMalloc(&c->mp_h_sc, sizeof(MPScalars)));
        HIP_TRY(hipMalloc(&c->mp_sc, sizeof(MPScalars)));
        HIP_TRY(hipMemsetAsync(c->mp_sc, 0, sizeof(MPScalars), c->stream));
        launch_mp_zero(c->stream, 2 * c->g.V, c->mp_y);
        c->mp_U_valid = false;
    }
    if (!c->mp_U_valid) {
        launch_sp_convert_links(c->stream, c->g, c->U, c->mp_U);
        c->mp_U_valid = true;
    }
    HIP_TRY(hipGetLastError());
    return SM_OK;
}

static int read_scalars(sm_ctx *c) {
    HIP_TRY(hipMemcpyAsync(c->mp_h_sc, c->mp_sc, sizeof(MPScalars), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

int cg_dev_mixed(sm_ctx *c, const double *phi_, double *x_, double m0, double tol, int max_iter, sm_cg_result *res) {
    TRY(check_ready(c));
    if (!phi_ || !x_) return fail(SM_ERR_ARG, "null argument");
    if (c->sharded()) return fail(SM_ERR_STATE, "the mixed-precision CG runs on one-shard contexts");
    const CGFusedCfg cfg = cg_sp_config(c->g, c->racfg);
    const int ntiles = cfg.TBk * cfg.XB;
    if (ntiles > kMaxPartials) return fail(SM_ERR_ARG, "too many tiles for the mixed-precision pass");
    TRY(mixed_ready(c));
    const long n = 2 * c->g.V;
    const double mass = m0 + 2;
    const double2 *phi = (const double2 *)phi_;
    double2 *x = (double2 *)x_;
    double2 *r = c->field(F_R), *t = c->field(F_T), *Ax = c->field(F_AD);
    MPScalars *sc = c->mp_sc;
    const MPScalars &h = *c->mp_h_sc;
    sm_cg_mixed_info &info = c->mp_info;
    info = sm_cg_mixed_info{};
    info.used = 1;
    if (x != phi) launch_copy(c->stream, n, phi, x);  // x = phi

    // x's true residual in fp64 into r and sc; init: the solve's first
    auto true_residual = [&](bool init, bool restart) -> int {
        TRY(apply(c, x, t, mass, 1, nullptr, nullptr, nullptr));
        TRY(apply(c, t, Ax, mass, 0, nullptr, nullptr, nullptr));
        const int nb = launch_mp_residual(c->stream, n, phi, Ax, r, c->mp_partials);
        launch_mp_update(c->stream, nb, c->mp_partials, sc, init ? 1 : 0, restart ? 1 : 0, tol, c->mp_delta, max_iter);
        HIP_TRY(hipGetLastError());
        return read_scalars(c);
    };

    int base = 0;  // d_i of the running segment lives in mp_d[(base + i) mod 3], i >= -1
    auto dbuf = [&](long i) { return c->mp_d[(((base + i) % 3) + 3) % 3]; };
    bool fallback = false;
    int fails = 0;
    double prev_true = 0.0;
    TRY(true_residual(true, true));
    for (;;) {
        const double true_err = std::sqrt(h.true_rr);
        if (c->debug_cg)
            fprintf(stderr, "[sm cg mixed] update %d inner %d true %.3e (target %.3e)\n", info.reliable_updates,
                    h.k_total, true_err, tol * h.phi_norm);
        if (info.reliable_updates > 0) fails = true_err < prev_true ? 0 : fails + 1;
        prev_true = true_err;
        if (!(true_err == true_err) || true_err < tol * h.phi_norm || h.k_total >= max_iter) break;
        if (fails >= 2 || (c->mp_force_fallback && info.reliable_updates >= 1)) {
            fallback = true;
            break;
        }
        // the segment: pass 0 on the injected direction, then passes 1, 2, ...
        // until the device ends it; the state is read once per chunk
        launch_mp_inject(c->stream, n, r, dbuf(-1), dbuf(0), sc);
        const int k_before = h.k_total;
        const long most = (long)(max_iter - k_before) + 1;  // the device stops itself at max_iter
        CgChunker plan;
        long j = 0;
        int chunk = plan.chunk;
        for (;;) {
            for (int i = 0; i < chunk && j < most; ++i, ++j) {
                // passes 0 and 1 both read d_0 and d_{-1}; pass 0 stores nothing
                const float2 *d1 = j == 0 ? dbuf(0) : dbuf(j - 1), *d2 = j == 0 ? dbuf(-1) : dbuf(j - 2);
                launch_cg_sp(c->stream, c->g, cfg, d1, d2, dbuf(j), c->mp_y, c->mp_U, mass, j, sc, c->mp_partials);
                launch_cg_sp_scalars(c->stream, ntiles, c->mp_partials, sc, j == 0);
            }
            HIP_TRY(hipGetLastError());
            TRY(read_scalars(c));
            if (c->debug_cg)
                fprintf(stderr, "[sm cg mixed]   passes %ld k %d err %.3e M %.3e done %d\n", j, h.k, h.err, h.M, h.done);
            if (h.done) break;
            if (j >= most) return fail(SM_ERR_STATE, "mixed-precision CG: the segment did not end at max_iter");
            const double target = std::fmax(c->mp_delta * h.M, tol * h.phi_norm);
            chunk = plan.next(h.k, h.err, target);
        }
        info.inner_iterations = h.k_total;
        const int J = h.k;
        if (h.bad) {  // a non-finite scalar: y is not trusted, x and r are those of the last update
            launch_mp_fold(c->stream, c->g, x, c->mp_y, dbuf(0), sc, 1);
            HIP_TRY(hipGetLastError());
            fallback = true;
            break;
        }
        launch_mp_fold(c->stream, c->g, x, c->mp_y, dbuf(J - 1), sc, 0);
        base = (int)((base + J) % 3);  // d_{J-1} becomes the next segment's d_{-1}, d_J's buffer takes its d_0
        info.reliable_updates++;
        TRY(true_residual(false, false));
    }
    info.inner_iterations = h.k_total;
    double true_err = std::sqrt(h.true_rr);
    const double phi_norm = h.phi_norm;
    if (fallback && h.k_total < max_iter && true_err > 0.0) {
        // the fp64 finish: D D^dag e = r (r kept apart: the fp64 solver's own buffers include F_R)
        if (!c->mp_fb) HIP_TRY(hipMalloc(&c->mp_fb, sizeof(double2) * 2 * (size_t)n));
        double2 *rhs = c->mp_fb, *e = c->mp_fb + n;
        launch_copy(c->stream, n, r, rhs);
        sm_cg_result r64{};
        TRY(cg_dev_fp64(c, (const double *)rhs, (double *)e, m0, tol * phi_norm / true_err, max_iter - h.k_total, &r64));
        launch_mp_add(c->stream, n, x, e);
        info.fell_back = 1;
        info.fp64_iterations = r64.iterations;
        const int inner = h.k_total;
        TRY(true_residual(false, true));
        info.inner_iterations = inner;
        true_err = std::sqrt(h.true_rr);
    } else if (fallback) {
        info.fell_back = 1;
    }
    info.true_residual = phi_norm > 0.0 ? true_err / phi_norm : true_err;
    res->converged = true_err < tol * phi_norm ? 1 : 0;
    res->iterations = info.inner_iterations + info.fp64_iterations;
    res->residual = true_err;
    res->phi_norm = phi_norm;
    return SM_OK;
}

}  // namespace sm_host
