// sm_flow.cpp -- topological charge and Wilson flow of a context's gauge field
// and of every replica of an ensemble (include/sm_hip.h, "topological charge
// and Wilson flow"). Kernels: sm_flow.hip.
//
//   sums     one reduction launch writes a field's (or R fields') partials,
//            one launch sums them into three doubles per field on the device.
//            sm_topology all-reduces them over the shards like any global sum;
//            the charges are the raw sums over 2 pi, divided on the host.
//   flow     every stage (one launch, for all replicas) and every measurement
//            (two launches) of the whole flow is enqueued on the context's
//            stream; the sums of point k land in a device series, replica-major
//            as the caller's, which ONE copy brings back after the last stage.
//            The only synchronisation is the one behind that copy (and the
//            flowed field's download when the caller asks for it).
//   buffers  a stage reads one field buffer and writes the other; the first
//            stage reads the gauge field itself, so nothing is copied and U is
//            never written. The context allocates two buffers and the
//            accumulator at its first flow; the ensemble flows in Ubak, chi and
//            P, free between trajectories (a trajectory writes each before it
//            reads it), with its partials in part.
// One-shard contexts for the flow; always fp64; synchronous.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "sm_ctx.h"
#include "sm_ens.h"
#include "sm_internal.h"

using namespace sm;
using namespace sm_host;

namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559;

// measured points of a flow, or -1 for parameters no flow runs with
long flow_points(const sm_flow_params *p) {
    if (!p || !(p->eps > 0.0) || !std::isfinite(p->eps) || p->nsteps < 0 || p->meas_every < 1) return -1;
    const long n = 1 + (long)(p->nsteps / p->meas_every);
    return n > INT_MAX ? -1 : n;
}

int check_flow_params(const sm_flow_params *p, long *points) {
    if (!p) return fail(SM_ERR_ARG, "null argument");
    *points = flow_points(p);
    if (*points < 0)
        return fail(SM_ERR_ARG, "bad flow params eps=%g nsteps=%d meas_every=%d (eps > 0 and finite, nsteps >= 0, "
                    "meas_every >= 1)", p->eps, p->nsteps, p->meas_every);
    return SM_OK;
}

// raw sums (action, sum of plaquette angles, sum Im U_01) -> sm_topo, in place
void to_topo(sm_topo *t, long n) {
    for (long i = 0; i < n; ++i) {
        t[i].q_geo = t[i].q_geo / kTwoPi;
        t[i].q_sin = t[i].q_sin / kTwoPi;
    }
}

// a device series of R x points x 3 doubles, kept and regrown for a longer one
int series_ready(sm_ctx *c, BufGroup &b, double **buf, long *have, int R, long points) {
    if (!b.empty() && *have >= points) return SM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    b.release();
    *have = 0;
    TRY(b.add(buf, 3 * (size_t)R * (size_t)points, BufKind::device, "series"));
    *have = points;
    return SM_OK;
}

struct FlowFields {
    bool ens;            // the replica kernels (R fields per launch) or the one-field ones
    int R;
    const double2 *U;    // the field(s) flowed from; never written
    double2 *W[2];
    double *A;
    double2 *part;       // 2 x R rows of gauge_reduce_blocks partials
    double *series;      // R x points x 3
};

// Enqueue the whole flow; *last = where the flowed field(s) end up (U itself for nsteps = 0).
int enqueue_flow(sm_ctx *c, const FlowFields &f, const sm_flow_params *p, long points, const double2 **last) {
    const Geometry &g = c->g;
    hipStream_t s = c->stream;
    auto measure = [&](const double2 *F, long k) {
        if (f.ens) launch_ens_topo(s, g, f.R, F, f.part);
        else launch_topo(s, g, 1, F, nullptr, f.part);
        launch_topo_sums(s, g, f.R, f.part, f.series + 3 * k, 3 * points);
    };
    const double2 *cur = f.U;
    int w = 0;
    measure(cur, 0);
    for (int step = 1; step <= p->nsteps; ++step) {
        for (int stage = 0; stage < 3; ++stage) {
            if (f.ens) launch_ens_flow_stage(s, g, f.R, stage, p->eps, cur, f.A, f.W[w]);
            else launch_flow_stage(s, g, stage, p->eps, cur, f.A, f.W[w]);
            cur = f.W[w];
            w ^= 1;
        }
        if (step % p->meas_every == 0) measure(cur, step / p->meas_every);
    }
    HIP_TRY(hipGetLastError());
    *last = cur;
    return SM_OK;
}

int one_shard(const sm_ctx *c) {
    if (c->sharded() || c->hosted || c->peer || c->nshard != 1)
        return fail(SM_ERR_ARG, "the Wilson flow runs on one-shard contexts (no t-shards, loopback, peer or "
                    "host-staged transport): the stages would need ghost exchanges of a field that is not U");
    return SM_OK;
}

int flow_buffers_ready(sm_ctx *c) {
    BufGroup &b = c->fl_bufs;
    if (!b.empty()) return SM_OK;
    const size_t n = 2 * (size_t)c->g.V;
    for (double2 *&W : c->fl_W) TRY(b.add(&W, n, BufKind::device, "field buffer"));
    return b.add(&c->fl_A, n, BufKind::device, "accumulator");
}

}  // namespace

extern "C" {

int sm_flow_points(const sm_flow_params *p) { return (int)flow_points(p); }

int sm_topology(sm_ctx *c, sm_topo *out) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    if (!out) return fail(SM_ERR_ARG, "null argument");
    TRY(check_ready(c));
    HIP_TRY(hipSetDevice(c->device));
    // the plaquette's neighbour links: the 2-deep U faces on t-shards (sm_plaquette's), the wrap on one shard
    const double2 *fU = c->sharded() ? face2_recv(c, 2) : nullptr;
    double *sums = (double *)c->sums;
    launch_topo(c->stream, c->g, c->kshards(), c->U, fU, c->partials);
    launch_topo_sums(c->stream, c->g, 1, c->partials, sums, 0);
    HIP_TRY(hipGetLastError());
    TRY(allreduce_dev(c, sums, 3));
    HIP_TRY(hipMemcpyAsync(c->h_sums, sums, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double *h = (const double *)c->h_sums;
    *out = sm_topo{h[0], h[1], h[2]};
    to_topo(out, 1);
    return SM_OK;
}

int sm_wilson_flow(sm_ctx *c, const sm_flow_params *p, sm_topo *series, double *U0_out, double *U1_out) {
    if (!c) return fail(SM_ERR_ARG, "null context");
    if (!series || (U0_out == nullptr) != (U1_out == nullptr))
        return fail(SM_ERR_ARG, "null argument (U0_out and U1_out: both or neither)");
    long points = 0;
    TRY(check_flow_params(p, &points));
    TRY(one_shard(c));
    TRY(check_ready(c));
    HIP_TRY(hipSetDevice(c->device));
    if (p->nsteps > 0) TRY(flow_buffers_ready(c));
    TRY(series_ready(c, c->fl_series_bufs, &c->fl_series, &c->fl_points, 1, points));
    const FlowFields f{false, 1, c->U, {c->fl_W[0], c->fl_W[1]}, c->fl_A, c->partials, c->fl_series};
    const double2 *last = nullptr;
    TRY(enqueue_flow(c, f, p, points, &last));
    HIP_TRY(hipMemcpyAsync(series, c->fl_series, sizeof(sm_topo) * (size_t)points, hipMemcpyDeviceToHost,
                           c->stream));
    if (U0_out) TRY(download_plane_pair(c, last, U0_out, U1_out));
    else HIP_TRY(hipStreamSynchronize(c->stream));
    to_topo(series, points);
    return SM_OK;
}

int sm_ens_topology(sm_ens *e, sm_topo *out) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    if (!out) return fail(SM_ERR_ARG, "null argument");
    TRY(all_have(e));
    sm_ctx *c = e->c;
    HIP_TRY(hipSetDevice(c->device));
    TRY(series_ready(c, e->fl_series_bufs, &e->fl_series, &e->fl_points, e->R, 1));
    launch_ens_topo(c->stream, c->g, e->R, e->U, e->part);
    launch_topo_sums(c->stream, c->g, e->R, e->part, e->fl_series, 3);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, e->fl_series, sizeof(sm_topo) * (size_t)e->R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    to_topo(out, e->R);
    return SM_OK;
}

int sm_ens_wilson_flow(sm_ens *e, const sm_flow_params *p, sm_topo *series, double *U_out) {
    if (!e) return fail(SM_ERR_ARG, "null ensemble");
    if (!series) return fail(SM_ERR_ARG, "null argument");
    long points = 0;
    TRY(check_flow_params(p, &points));
    TRY(all_have(e));
    sm_ctx *c = e->c;
    HIP_TRY(hipSetDevice(c->device));
    TRY(series_ready(c, e->fl_series_bufs, &e->fl_series, &e->fl_points, e->R, points));
    const FlowFields f{true, e->R, e->U, {e->Ubak, e->chi}, e->P, e->part, e->fl_series};
    const double2 *last = nullptr;
    TRY(enqueue_flow(c, f, p, points, &last));
    const size_t n = (size_t)e->R * (size_t)points;
    HIP_TRY(hipMemcpyAsync(series, e->fl_series, sizeof(sm_topo) * n, hipMemcpyDeviceToHost, c->stream));
    if (U_out)
        HIP_TRY(hipMemcpyAsync(U_out, last, sizeof(double2) * slab_complex(e) * (size_t)e->R, hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    to_topo(series, (long)n);
    return SM_OK;
}

}  // extern "C"
