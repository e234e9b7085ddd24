// sm_eomp.cpp -- mixed-precision CG on Dhat Dhat^dagger (the even-odd
// action's solver): fp32 inner iterations (sm_eosp.hip) held to the fp64 stop
// test by reliable updates. The scheme is sm_cgmp.cpp's, on half-lattice
// vectors and with the stored-Ad pass:
//
//   x = phi_e; r = phi_e - Dhat Dhat^dag x in fp64 (eo_dhat); M = |r|
//   segment: d_0 = fp32(r) + beta d_prev (first: beta = 0), y = 0, fp32
//       one-pass iterations on y until the iterated |r| < delta M or
//       < tol |phi| -- decided on the device, read in CgChunker chunks
//   reliable update: x += y (+ alpha_{J-1} d_{J-1} after an odd last pass J),
//       y = 0, r = phi_e - Dhat Dhat^dag x in fp64; stop if |r| < tol |phi|;
//       else beta = |r|^2 / |r_{J-1}|^2 and the next segment starts from
//       d_{J-1}: the search direction survives the update.
// The solve stops only on an fp64 true residual. Two consecutive updates that
// fail to lower it, or a bad fp32 scalar, hand the rest to the fp64 even-odd
// solver: Dhat Dhat^dag e = r (its own x0 = r convention), x += e.
//
// One-shard contexts only (sm_eo_cg_precision refuses the others). The fp32
// side owns everything it writes: directions, Ad, y, links, partials, scalars
// and the fp64 work vectors of the true residual. The fp64 even-odd vectors
// are used only by the fp64 code itself (eo_dhat's scratch, the fallback's
// eo_cg), which overwrites them at every start.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "sm_ctx.h"
#include "sm_internal.h"

using namespace sm;

namespace sm_host {

void eo_cg_mixed_free(sm_ctx *c) {
    for (float2 *&d : c->eomp_d) {
        stream_free(c, d);
        d = nullptr;
    }
    for (float2 *&a : c->eomp_a) {
        stream_free(c, a);
        a = nullptr;
    }
    for (float2 *&u : c->eomp_U) {
        stream_free(c, u);
        u = nullptr;
    }
    stream_free(c, c->eomp_y);
    c->eomp_y = nullptr;
    if (c->eomp_w) (void)hipFree(c->eomp_w);
    if (c->eomp_fb) (void)hipFree(c->eomp_fb);
    if (c->eomp_partials) (void)hipFree(c->eomp_partials);
    if (c->eomp_sc) (void)hipFree(c->eomp_sc);
    if (c->eomp_h_sc) (void)hipHostFree(c->eomp_h_sc);
    c->eomp_w = c->eomp_fb = c->eomp_partials = nullptr;
    c->eomp_sc = c->eomp_h_sc = nullptr;
    c->eomp_U_valid = false;
}

// The mode's buffers, at the first mixed even-odd solve; the fp32 links again
// after every change of U (from the checkerboard links eo_ready just made).
static int eo_mixed_ready(sm_ctx *c) {
    const size_t n = (size_t)c->g.V;  // complex entries of a one-parity field
    const size_t fb = sizeof(float2) * n;
    if (!c->eomp_sc) {
        for (float2 *&d : c->eomp_d) HIP_TRY(stream_malloc(c, (void **)&d, fb));
        for (float2 *&a : c->eomp_a) HIP_TRY(stream_malloc(c, (void **)&a, fb));
        for (float2 *&u : c->eomp_U) HIP_TRY(stream_malloc(c, (void **)&u, fb));
        HIP_TRY(stream_malloc(c, (void **)&c->eomp_y, fb));
        HIP_TRY(hipMalloc(&c->eomp_w, sizeof(double2) * 3 * n));
        HIP_TRY(hipMalloc(&c->eomp_partials, sizeof(double2) * 2 * (size_t)kMaxPartials));
        HIP_TRY(hipHostMalloc(&c->eomp_h_sc, sizeof(MPScalars)));
        HIP_TRY(hipMalloc(&c->eomp_sc, sizeof(MPScalars)));
        HIP_TRY(hipMemsetAsync(c->eomp_sc, 0, sizeof(MPScalars), c->stream));
        launch_mp_zero(c->stream, (long)n, c->eomp_y);
        c->eomp_U_valid = false;
    }
    if (!c->eomp_U_valid) {
        launch_eo_sp_convert_links(c->stream, c->g, eo_links(c, 0), eo_links(c, 1), c->eomp_U[0], c->eomp_U[1]);
        c->eomp_U_valid = true;
    }
    HIP_TRY(hipGetLastError());
    return SM_OK;
}

static int read_scalars(sm_ctx *c) {
    HIP_TRY(hipMemcpyAsync(c->eomp_h_sc, c->eomp_sc, sizeof(MPScalars), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SM_OK;
}

// b, x: even vectors on the device (x may be b); eo_ready has run for the current U.
int eo_cg_mixed(sm_ctx *c, const double2 *phi, double2 *x, double mass, double tol, int max_iter, sm_cg_result *res) {
    if (c->sharded() || c->peer) return fail(SM_ERR_STATE, "the mixed-precision even-odd CG runs on one-shard contexts");
    const EoTdCfg cfg = eo_td_config(c->g);
    const int ntiles = eo_td_blocks(cfg);
    if (ntiles > kMaxPartials) return fail(SM_ERR_ARG, "too many tiles for the mixed-precision even-odd pass");
    TRY(eo_mixed_ready(c));
    const long n = c->g.V;
    double2 *r = c->eomp_w, *w = c->eomp_w + n, *Ax = c->eomp_w + 2 * n;
    MPScalars *sc = c->eomp_sc;
    const MPScalars &h = *c->eomp_h_sc;
    sm_cg_mixed_info &info = c->eomp_info;
    info = sm_cg_mixed_info{};
    info.used = 1;
    if (x != phi) launch_copy(c->stream, n, phi, x);  // x = phi_e

    // x's true residual in fp64 into r and sc; init: the solve's first
    auto true_residual = [&](bool init, bool restart) -> int {
        TRY(eo_dhat(c, 1, x, w, mass));
        TRY(eo_dhat(c, 0, w, Ax, mass));
        const int nb = launch_mp_residual(c->stream, n, phi, Ax, r, c->eomp_partials);
        launch_mp_update(c->stream, nb, c->eomp_partials, sc, init ? 1 : 0, restart ? 1 : 0, tol, c->mp_delta,
                         max_iter);
        HIP_TRY(hipGetLastError());
        return read_scalars(c);
    };

    int base = 0;  // d_i of the running segment lives in eomp_d[(base + i) mod 3], i >= -1
    auto dbuf = [&](long i) { return c->eomp_d[(((base + i) % 3) + 3) % 3]; };
    bool fallback = false;
    int fails = 0;
    double prev_true = 0.0;
    TRY(true_residual(true, true));
    for (;;) {
        const double true_err = std::sqrt(h.true_rr);
        if (c->debug_cg)
            fprintf(stderr, "[sm eo_cg mixed] update %d inner %d true %.3e (target %.3e)\n", info.reliable_updates,
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
                // passes 0 and 1 both read d_0 and d_{-1}; pass 0 stores no d and reads no Ad
                const float2 *d1 = j == 0 ? dbuf(0) : dbuf(j - 1), *d2 = j == 0 ? dbuf(-1) : dbuf(j - 2);
                launch_eo_sp(c->stream, c->g, cfg, d1, d2, c->eomp_a[(j + 1) & 1], dbuf(j), c->eomp_a[j & 1], c->eomp_y,
                             c->eomp_U[0], c->eomp_U[1], mass, j, sc, c->eomp_partials);
                launch_cg_sp_scalars(c->stream, ntiles, c->eomp_partials, sc, j == 0);
            }
            HIP_TRY(hipGetLastError());
            TRY(read_scalars(c));
            if (c->debug_cg)
                fprintf(stderr, "[sm eo_cg mixed]   passes %ld k %d err %.3e M %.3e done %d\n", j, h.k, h.err, h.M,
                        h.done);
            if (h.done) break;
            if (j >= most) return fail(SM_ERR_STATE, "mixed-precision even-odd CG: the segment did not end at max_iter");
            const double target = std::fmax(c->mp_delta * h.M, tol * h.phi_norm);
            chunk = plan.next(h.k, h.err, target);
        }
        info.inner_iterations = h.k_total;
        const int J = h.k;
        if (h.bad) {  // a bad scalar: y is not trusted, x and r are those of the last update
            launch_eo_mp_fold(c->stream, n, x, c->eomp_y, dbuf(0), sc, 1);
            HIP_TRY(hipGetLastError());
            fallback = true;
            break;
        }
        launch_eo_mp_fold(c->stream, n, x, c->eomp_y, dbuf(J - 1), sc, 0);
        base = (int)((base + J) % 3);  // d_{J-1} becomes the next segment's d_{-1}, d_J's buffer takes its d_0
        info.reliable_updates++;
        TRY(true_residual(false, false));
    }
    info.inner_iterations = h.k_total;
    double true_err = std::sqrt(h.true_rr);
    const double phi_norm = h.phi_norm;
    if (fallback && h.k_total < max_iter && true_err > 0.0) {
        // the fp64 finish: Dhat Dhat^dag e = r through the fp64 even-odd solver
        if (!c->eomp_fb) HIP_TRY(hipMalloc(&c->eomp_fb, sizeof(double2) * 2 * (size_t)n));
        double2 *rhs = c->eomp_fb, *e = c->eomp_fb + n;
        launch_copy(c->stream, n, r, rhs);
        sm_cg_result r64{};
        TRY(eo_cg(c, rhs, e, mass, tol * phi_norm / true_err, max_iter - h.k_total, &r64));
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
