// sm_ctx.h -- private host-side state of one lattice shard (the opaque
// sm_ctx of include/sm_hip.h) and the transport / launch helpers shared by
// sm_capi.cpp (operators, CG) and sm_md.cpp (gauge field, MD, HMC).
#pragma once
#include "../../include/sm_hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "sm_buf.h"
#include "sm_internal.h"
#include "sm_peer.h"

namespace sm_host {  // fail, TRY: sm_cg_host.h (through sm_internal.h)

constexpr const char *kBatchWho = "batched CG", *kEoBatchWho = "batched even-odd CG";  // their error prefixes

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return ::sm_host::fail(SM_ERR_HIP, "%s failed: %s (%s:%d)", #expr,           \
                                   hipGetErrorString(e_), __FILE__, __LINE__);          \
    } while (0)

#define NCCL_TRY(expr)                                                                     \
    do {                                                                                   \
        ncclResult_t r_ = (expr);                                                          \
        if (r_ != ncclSuccess)                                                             \
            return ::sm_host::fail(SM_ERR_RCCL, "%s failed: %s (%s:%d)", #expr,             \
                                   ncclGetErrorString(r_), __FILE__, __LINE__);            \
    } while (0)

}  // namespace sm_host


// Work fields, each 2*V complex (plane mu0 then mu1).
// F_D, F_D2, F_R: the three d buffers of the one-pass CG paths (F_R is r in the
// six-launch path); F_AD2: the second Ad buffer of the stored-Ad pass (ping-pong with F_AD).
enum { F_IN, F_OUT, F_TMP, F_X, F_R, F_D, F_D2, F_T, F_AD, F_PHI, F_L, F_RR, F_AD2, NFIELDS };

// Workspace of an fp64 batched CG solve of up to K columns of n complex, the
// full-lattice solver's (sm_cgbatch.cpp, n = 2V) or the even-odd one's
// (sm_eobatch.cpp, n = V): the context owns one of each for sm_cg_batch and
// sm_eo_cg_batch, a replica ensemble (sm_ens.cpp) its own. bufs owns every
// pointer (batch_ws_alloc); who: the solver's error prefix.
struct BatchWs {
    explicit BatchWs(const char *who) : bufs(who) {}
    sm_host::BufGroup bufs;
    int K = 0;                      // columns it holds
    long n = 0;                     // complex per column
    double2 *d[3] = {};             // d_i in d[i mod 3], K x n complex each
    double2 *a[2] = {};             // Ad by pass parity
    double2 *partials = nullptr;    // K x BatchCfg::pstride
    sm::CGScalars *sc = nullptr, *h_sc = nullptr;  // K each: device, pinned host mirror
};

// State of a mixed-precision solver (sm_cgmp.cpp on the full lattice,
// sm_eomp.cpp on one parity): its own directions, y, links, partials and
// scalars, from the first mixed solve on; nothing shared with the fp64 paths.
// n = the solver's vector length in complex entries (2V / V). bufs owns every
// pointer but fb, which is fin's: a failed fallback request leaves the rest.
struct MixedWs {
    MixedWs(const char *who, sm_ctx *c) : bufs(who, c), fin(who) {}
    sm_host::BufGroup bufs, fin;
    float2 *d[3] = {};              // the three direction buffers, n float2 each
    float2 *a[2] = {};              // even-odd: Ad_j by pass parity
    float2 *y = nullptr;            // the fp32 correction to x
    float2 *U[2] = {};              // the links as the fp32 pass reads them (even-odd: even, odd)
    bool U_valid = false;           // false after every change of U (exchange_ghost_U)
    double2 *w = nullptr;           // even-odd: fp64 work r, Dhat^dag x, Dhat Dhat^dag x (3n)
    double2 *fb = nullptr;          // fp64 finish: rhs and correction (2n; allocated on a fallback)
    double2 *partials = nullptr;    // 2 per tile
    sm::MPScalars *sc = nullptr, *h_sc = nullptr;  // device, pinned host mirror
    sm_cg_mixed_info info{};        // the last solve
};

// State of the mixed-precision batched solver (sm_cgbatchmp.cpp) for K columns:
// its own fp32 directions, Ad, y and links, the fp64 work of the true residual,
// partials and scalars; nothing shared with the fp64 batch but the K = 1
// workspace of the rare fp64 finish (sm_ctx::bt, whatever it holds). bufs owns
// every pointer.
struct CGBatchMixedWs {
    sm_host::BufGroup bufs{"mixed batched CG"};
    int K = 0;                      // columns it holds
    float2 *d[3] = {};              // the direction ring, K x 2V float2 each
    float2 *a[2] = {};              // Ad by pass parity
    float2 *y = nullptr;            // the fp32 corrections
    float2 *U = nullptr;            // the links as the fp32 pass reads them, converted at every solve
    double2 *r = nullptr, *t = nullptr, *ax = nullptr;  // fp64: r, D^dag x (the finish's e), D D^dag x; K x 2V each
    double2 *partials = nullptr;
    sm::MPScalars *sc = nullptr, *h_sc = nullptr;  // K each: device, pinned host mirror
};

// Every buffer allocated after creation belongs to a BufGroup (sm_buf.h) next to
// its pointers: one group per capacity, built whole or not at all, tested with
// empty() and freed by its destructor at sm_destroy's `delete`, after the
// streams were synchronised. The creation-time buffers (U, fields[], faces,
// scalars, pinned mirrors, Uang, the peer region) are sm_destroy's own.
struct sm_ctx {
    int device = 0;
    int nshard = 1, shard = 0;
    // RCCL loopback (sm_create_loopback): one shard driven through the t-shard
    // code path, faces and scalar sums over a one-rank communicator (self
    // send/recv). Tests the RCCL data path on a single GPU.
    bool loop = false;
    int debug_cg = 0;  // test option debug_cg=1: the CG host loops print their status at each check (stderr)
    bool sharded() const { return nshard > 1 || loop; }  // faces + collectives (else periodic wrap)
    int kshards() const { return sharded() ? 2 : 1; }    // the kernels' view: > 1 reads faces
    sm::Geometry g{};
    sm::LaunchCfg cfg{};
    sm::CGFusedCfg fcfg{};
    sm::CGFusedCfg racfg{};        // recompute-Ad CG pass (sm_cgra.hip)
    // CG iteration: 0 the reference's six-launch sequence (576 B/site), 4 the
    // two-direction one-pass form with a stored Ad (sm_cgfused.hip: no r
    // vector, x every other pass, 224 B/site), 5 the two-direction pass that
    // recomputes Ad instead of storing it (sm_cgra.hip, 160 B/site). Chosen at
    // creation: 5 from 256^2 sites per shard, 4 below (latency-bound grids).
    int cg_fused = 4;
    int cg_red_max_blocks = sm::kRedundantMaxBlocks;  // stored-Ad pass: redundant scalars up to this grid
    long cg_flush_pass = -1;        // last one-pass pass whose scalars still await evaluation
    int cg_flush_nparts = 0;        // its partial count (the one-pass or the recompute-Ad grid)
    int cg_ra_red_max_blocks = 512; // recompute-Ad pass: redundant scalars up to this many blocks (one shard)
    // recompute-Ad pass with compact links (sm_cgra.hip UC): U enters the CG as
    // one double + one 16-bit flag word per link (sm_linkcode.h, 20 B/site),
    // rebuilt bitwise in registers.
    // Built at the first solve after U changes (uang_state 0); state 1 = in
    // use, 2 = some link is not encodable (far off the unit circle, NaN), so
    // the complex links are used.
    int link_angles = 1;
    int uang_state = 0;
    int link_fmt = 1;               // codes in use: 2 = flag nibbles, one byte per site; 1 = 16-bit flag words
    int cg_link_bytes_last = 0;     // link bytes per site the last CG pass launched read (sm_cg_link_bytes; 0: none yet)
    // Placement of the buffers the CG pass streams (stream_malloc): 5 = an
    // allocation of >= 2 GiB each with hipDeviceMallocContiguous (the
    // default; plain allocation of that size when the driver has no
    // contiguous memory), 0 = own size (A/B). Test option pad_alloc=N; DESIGN
    // §2 and profiles/r04_e_alloc_trials.jsonl give the measurements.
    int pad_alloc = 5;
    // Placement probe at creation (sm_place.cpp placement_probe): candidates
    // per streamed buffer (0 = no probe; sm_set_placement_probe, test option
    // place_probe=N), the pass time of the initial set and after each
    // buffer's search (us per pass), and which buffers moved (bit mask).
    int place_probe = 3;
    long place_min_mib = 256;       // smallest field (MiB) that is probed; test option probe_min_mib=N
    int place_n = 0, place_chosen = 0;
    double place_us[16] = {};       // the initial set, then one per buffer searched (up to 3 sweeps of 4)
    double *Uang = nullptr;         // 2V link codes (plane mu0 then mu1)
    double *Uang_face = nullptr;    // t-shards: codes of the 4-deep ghost links (16 Nx)
    sm_host::BufGroup uang_face_bufs{"link codes"};
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t comm_stream = nullptr;  // halo exchange overlapped with interior compute (hosted: == stream)
    bool own_comm_stream = false;       // comm_stream created by (and destroyed with) this context
    hipEvent_t ev_ready = nullptr, ev_halo = nullptr;
    // t-shard CG pass (split launches): the interior launch records ev_int at
    // its own end (hipExtLaunchKernelGGL), and the next pass's comm stream
    // waits on it instead of a marker behind it on the main stream; valid for
    // pass ev_int_pass only (-1: record the marker). kernel_events = 0 keeps
    // the markers (test option).
    hipEvent_t ev_int = nullptr;
    long ev_int_pass = -1;
    int kernel_events = 1;
    hipEvent_t ev_rccl = nullptr;   // orders an RCCL operation after the previous one on the other stream
    hipStream_t rccl_last = nullptr;  // stream of the last RCCL operation (sm_comm.cpp rccl_order)
    int rccl_ordered = 1;           // test option rccl_order=0: no ordering events (A/B)
    // t-shards: the edge block-columns run on the comm stream right after the
    // halo, concurrently with the interior launch on the main stream.
    // recompute-Ad CG on t-shards: the edge launch packs d_j's faces and the
    // exchange for pass j+1 is issued right behind it (cg_faces_for: the pass
    // whose d_{j-1} faces are already in flight); edge launch rows per block
    int cg_face_pipe = 1;
    int apply_split = 1;            // t-shard Dirac apply: interior / edge launches around the faces (0: faces first)
    int cg_edge_xchunk = -1;        // -1: by the residency rule (launch_cg_ra_pass)
    int cg_shard_blocks_per_cu[3] = {-1, -1, -1};  // occupancy of the t-shard pass by link form (-1: not asked yet)
    int n_cu = 256;                 // compute units of the device (residency of a launch)
    long cg_faces_for = -1;
    int cg_faces_packed = 0;        // face_pipe 2: cg_faces_for's faces are packed, not yet sent
    // recompute-Ad pass: ticketed tail (the pass's last block sums the partials
    // by groups of 64 and forms the scalars / the shard's sums), no scalar kernel
    int cg_tail = 1;
    int cg_red_shards = 1;          // t-shards: next pass's blocks evaluate the scalars from the all-reduced sums
    int cg_flush_sums = 0;          // the pending flush evaluates sc->sumr (t-shards), not partials
    unsigned *tick = nullptr;       // 1 + kMaxTickGroups counters, zeroed at creation
    double2 *gsum = nullptr;        // 3 per group
    ncclComm_t comm = nullptr;      // the context's one communicator; its operations in one total order
    // Device-initiated transport (sm_peer.h; sm_create_peer / sm_peer_connect,
    // sm_create_peer_loopback): every shard's region mapped here, kernels store
    // into the neighbours' regions and wait on flags in their own. One stream.
    bool peer = false;
    bool peer_connected = false;
    char *peer_region = nullptr;    // mine (uncached, IPC-exported)
    char *peer_open[sm::kPeerMaxRanks] = {};  // the others' regions as opened here (null: mine / not open)
    sm::PeerView peer_view{};       // host copy (kernel arguments)
    sm::PeerView *peer_view_dev = nullptr;  // device copy (the CG pass's tail)
    unsigned long long peer_coll_seq = 0, peer_face_seq = 0;  // the next collective / face exchange is seq + 1
    unsigned *peer_tick = nullptr;  // zeroed ticket counter of the transport kernels
    int peer_store = 0;             // CG pass face stores: 0 16-B write-through, 1 8-B atomic, 2 plain (test option)
    unsigned long long peer_wait_ticks = sm::kPeerWaitTicks;  // one wait's time limit (test option peer_wait_ms)
    // RCCL contexts: the recompute-Ad pass's scalar sums all-reduced in its own last
    // block through 4-KiB peer headers (sm_peer.h) instead of an ncclAllReduce per
    // pass; the halos stay RCCL (sm_comm.cpp rccl_peer_sums_setup). Test option
    // rccl_sums=1 keeps the ncclAllReduce.
    bool peer_sums = false;
    int peer_sums_wish = 1;
    int hosted_psums = 0;           // host-staged contexts: the same in-pass sums (test option hosted_psums=1)
    bool hosted = false;            // host-callback transport instead of RCCL
    sm_host_transport tr{};
    double *h_face = nullptr;       // pinned: send_lo, send_hi, recv_lo, recv_hi (4 x up to 8Nx doubles)
    double *h_red = nullptr;        // pinned: all-reduce staging (8 doubles)
    bool have_gauge = false;
    double2 *U = nullptr;          // 2V
    double2 *ghostU = nullptr;     // Nx: U_t at local t = -1 (lower neighbour's last column)
    double2 *fields[NFIELDS] = {};  // 2V each, one allocation per field (stream_alloc_bytes)
    double2 *faces = nullptr;      // 4 * 2Nx per spinor being exchanged (x2 for force)
    double2 *faces2 = nullptr;     // 2-deep faces: send lo/hi of 2 fields (4Nx each), recv d, r, U (8Nx each)
    double2 *faces4 = nullptr;     // 4-deep faces (sm_capi.cpp face4_*): send lo/hi, recv d x2 (by pass parity), U
    double2 *partials = nullptr;   // 2 * max(nparts)
    double2 *sums = nullptr;       // 4 complex scratch (allreduce)
    double *Fbuf = nullptr;        // 2V doubles (force)
    sm::CGScalars *sc = nullptr;       // device
    sm::CGScalars *h_sc = nullptr;     // pinned host mirror
    double2 *h_sums = nullptr;     // pinned host
    int nparts_dslash = 0, nparts_red = 0;
    // molecular dynamics (sm_md.cpp; allocated on first use)
    double2 *U_alt = nullptr;       // 2V: the other gauge buffer (leapfrog copy / kept conf)
    double *Pmd = nullptr;          // 2V: momenta
    double *Fmd = nullptr;          // 2V: MD force
    sm_host::BufGroup md_bufs{"molecular dynamics"};
    // even-odd action (sm_eo.cpp; allocated on first use)
    double2 *eo = nullptr;          // checkerboard work vectors, V complex each
    double2 *Ucb = nullptr;         // gauge field in checkerboard layout (even, odd)
    double2 *eo_faces = nullptr;    // t-sharded: checkerboard face slots (sm_eo.cpp)
    double2 *eo_faces4 = nullptr;   // t-sharded: 4-deep checkerboard face slots of the one-pass eo CG
    sm_host::BufGroup eo_bufs{"even-odd action"};
    int eo_fused = 1;               // Dhat as one fused marching pass (0: two hop launches)
    int eo_cg_td = 1;               // even-odd CG: the one-pass two-direction kernel (sm_eotd.hip, one shard;
                                    // 0.54 vs 0.94 ms per iteration at 4096^2 for the six launches)
    int eo_cg_folded = 0;           // even-odd CG: 1 = 2 passes + scalars per iteration (opt-in:
                                    // measured slower than the 6 launches from 512^2 to 2048^2)
    // active CG
    double cg_mass = 0.0;
    const double2 *cg_phi = nullptr;
    double2 *cg_x = nullptr;        // the x the passes update: the caller's, or F_X (cg_x_user != null)
    double2 *cg_x_user = nullptr;   // the caller's x when the passes run on F_X (copied back by sm_cg_finish)
    bool x_internal = false;        // fields of >= 256 MiB: a solve runs on F_X (stream_alloc_bytes) and
                                    // copies x to the caller's buffer at sm_cg_finish
    int cg_active = 0;
    long cg_issued = 0;             // iterations enqueued since sm_cg_begin
    int cg_pending_x = 0;           // fused path: last x update deferred to sm_cg_finish
    // mixed-precision CG (sm_cgmp.cpp; one shard): sm_cg_dev runs fp32 inner
    // iterations with fp64 reliable updates when cg_precision == 1.
    int cg_precision = 0;
    double mp_delta = 0.1;          // update when the iterated |r| < mp_delta * its maximum (test option mp_delta_pct)
    int mp_force_fallback = 0;      // test option: take the fp64 finish after the first update
    MixedWs mp{"mixed-precision CG", this};  // info: the last sm_cg_dev
    // mixed-precision even-odd CG (sm_eomp.cpp; one shard): every even-odd
    // solve runs fp32 inner iterations (sm_eosp.hip) with fp64 reliable updates
    // when eo_cg_precision == 1. Independent of cg_precision; shares only the
    // test options mp_delta / mp_force_fallback. Neither eo / sc / partials /
    // tick nor the mp state above is touched by the fp32 side.
    int eo_cg_precision = 0;
    MixedWs eomp{"mixed-precision even-odd CG", this};  // info: the last even-odd solve
    // batched multi-source CG (sm_cgbatch.cpp; one shard): its own directions,
    // Ad buffers, scalars and partials for bt.K columns, from the first batched
    // solve on and regrown for a larger K. Reads c->U at every call; keeps
    // nothing that depends on the gauge field.
    BatchWs bt{sm_host::kBatchWho};  // the solver's workspace
    int bt_tiles = 0;               // test option batch_tiles=N: tiles per launch aimed at (0: kBatchTargetTiles)
    // sm_cg_batch(_dev) and the correlator's solve run fp32 inner iterations with
    // fp64 reliable updates when bt_precision == 1 (sm_cgbatchmp.cpp). Independent
    // of cg_precision and eo_cg_precision; shares only the test options mp_delta
    // / mp_force_fallback. The replica ensemble does not look at it.
    int bt_precision = 0;
    CGBatchMixedWs btmp;
    std::vector<sm_cg_mixed_info> bt_info;  // the columns of the last batched solve (all zero: it ran fp64)
    // pion correlator: sources / solutions (bt_pion_K columns), source coordinates, C
    int bt_pion_K = 0;
    double2 *bt_phi = nullptr, *bt_x = nullptr;
    sm_host::BufGroup bt_stage_bufs{sm_host::kBatchWho};  // bt_phi, bt_x
    int *bt_src = nullptr;          // 2 x kBatchMax / 2 ints
    double *bt_C = nullptr;         // kBatchMax / 2 x Wt
    sm_host::BufGroup bt_corr_bufs{sm_host::kBatchWho};   // bt_src, bt_C

    // batched even-odd CG (sm_eobatch.cpp; one shard, fp64): its own workspace
    // for eob.K columns, the checkerboard copy of U it makes at every call, the
    // columns' even parts (eob_K columns) and the host-pointer entry's
    // full-layout staging (eob_fK columns), all from the first call on. Shares
    // nothing with eo / Ucb, the mixed solvers, bt or the stepwise solver.
    BatchWs eob{sm_host::kEoBatchWho};
    int eob_tiles = 0;              // test option eo_batch_tiles=N: tiles per launch aimed at (0: kEoBatchTargetTiles)
    double2 *eob_U = nullptr;       // even links, then odd links: 2V complex
    int eob_K = 0, eob_fK = 0;
    double2 *eob_phi = nullptr, *eob_x = nullptr;    // eob_K x V complex
    double2 *eob_fphi = nullptr, *eob_fx = nullptr;  // eob_fK x 2V complex
    sm_host::BufGroup eob_U_bufs{sm_host::kEoBatchWho}, eob_half_bufs{sm_host::kEoBatchWho},  // eob_U; eob_phi, eob_x
        eob_full_bufs{sm_host::kEoBatchWho};                                                   // eob_fphi, eob_fx

    // sm_pion_correlator through the even-odd system (sm_pion_solver = 1; sm_pion.cpp):
    // five half-lattice fields and the full-layout propagators for pn_K columns, from
    // the first such call on. The solve runs on eob and eob_U (above).
    int pion_solver = 0;
    int pn_K = 0;
    double2 *pn_buf = nullptr;      // pn_K x 7V complex
    sm_host::BufGroup pn_bufs{sm_host::kEoBatchWho};

    // topological charge and Wilson flow (sm_flow.cpp). sm_topology works in
    // partials / sums; a flow (one shard) in two field buffers and one
    // accumulator of its own, allocated at the first flow, and a device series.
    double2 *fl_W[2] = {};          // 2V complex each: a stage reads one (or U) and writes the other
    double *fl_A = nullptr;         // 2V doubles
    double *fl_series = nullptr;    // 3 doubles per measured point, regrown for a longer series
    long fl_points = 0;
    sm_host::BufGroup fl_bufs{"Wilson flow"}, fl_series_bufs{"Wilson flow"};  // fl_W, fl_A; fl_series

    // stochastic quark loops (sm_loops.cpp), from the first call on: the columns' (seed, k) and the
    // loops of lp_cols columns on the device. Solves and fields are the batched CG's / the pion's above.
    uint64_t *lp_sk = nullptr;      // 2 x kBatchMax: seeds, then vector numbers
    double *lp_out = nullptr;       // lp_cols x Wt x 4
    size_t lp_cols = 0;
    sm_host::BufGroup lp_sk_bufs{"quark loops"}, lp_out_bufs{"quark loops"};

    double2 *field(int i) { return fields[i]; }
};

namespace sm_host {

using namespace sm;

// CgChunker and the chunked status loop of the CG hosts (cg_chunked): sm_cg_host.h

// Largest face exchanged, in doubles per x: 4 columns x 2 planes x complex.
constexpr size_t kMaxFaceDoubles = 16;

TFaces faces_for(sm_ctx *c, const double2 *in, const double2 *recv_lo, const double2 *recv_hi);
double2 *face_buf(sm_ctx *c, int set, int which);
int exchange_faces_on(sm_ctx *c, hipStream_t s, double2 *slo, double2 *shi, double2 *rlo, double2 *rhi,
                      size_t cnt);
// n independent face exchanges in ONE transport round (RCCL: one group of 4n
// point-to-point operations; the host-staged transport runs them in turn)
int exchange_faces_multi(sm_ctx *c, hipStream_t s, int n, double2 *const *slo, double2 *const *shi,
                         double2 *const *rlo, double2 *const *rhi, size_t cnt);
// RCCL contexts hold ONE communicator; every RCCL operation runs on the
// stream it is issued on, ordered on the GPU after the previous RCCL
// operation (sm_comm.cpp rccl_order), in host issue order -- the same
// sequence on every rank. n face exchanges in one group:
// send_up[i] -> up rank's recv_down[i], send_down[i] -> down rank's recv_up[i].
int rccl_p2p_group(sm_ctx *c, hipStream_t s, int n, const double2 *const *send_up, double2 *const *recv_down,
                   const double2 *const *send_down, double2 *const *recv_up, size_t cnt);
// shards 1..P-1 send cnt doubles to shard 0, which receives shard r's at recv + r*cnt
int rccl_gather_to0(sm_ctx *c, hipStream_t s, const double *send, double *recv, size_t cnt);
// waiter has waited for an event recorded on signaler after its last RCCL
// operation (a launch schedule's own join): no ordering event needed
void rccl_joined(sm_ctx *c, hipStream_t waiter, hipStream_t signaler);
int exchange_faces(sm_ctx *c, double2 *slo, double2 *shi, double2 *rlo, double2 *rhi, size_t cnt);
int allreduce_dev(sm_ctx *c, double *dev, int n);
int halo(sm_ctx *c, const double2 *field, int set, int kind, TFaces *f);  // kind: FaceKind
const double2 *loU(sm_ctx *c);
int apply(sm_ctx *c, const double2 *in, double2 *out, double mass, int dagger, const double2 *aux,
          double2 *partials, const CGScalars *skip);
int global_sum(sm_ctx *c, int nparts, const double2 *part, int slot);
// alpha (which = 0) / beta (1) from per-block partials: local sum, all-reduce, scalar
int cg_scalar(sm_ctx *c, int nparts, int which);
int check_ready(sm_ctx *c);
int upload_plane_pair(sm_ctx *c, double2 *dst, const double *p0, const double *p1);
int download_plane_pair(sm_ctx *c, const double2 *src, double *p0, double *p1);
double2 *face2_recv(sm_ctx *c, int which);  // 0: d, 1: r, 2: U, 3: Ad
double2 *face4_recv_U(sm_ctx *c);           // 4-deep ghost links (recompute-Ad CG)
bool cg_ra_ok(const sm_ctx *c);             // the recompute-Ad pass fits this shard (Wt >= 4 when sharded)
int exchange_ghost_U(sm_ctx *c);
// (sm_comm.cpp) the peer transport connected; the in-pass CG sums' headers of an
// RCCL / host-staged context (agreed over the shards; never fail on a local
// failure); the peer view and its handshake; the recompute-Ad pass's 4-deep
// faces: send buffers, receive slot of pass `pass`, pack + exchange into recv
int up_rank(const sm_ctx *c);    // t + 1 neighbour shard (periodic)
int down_rank(const sm_ctx *c);  // t - 1 neighbour shard
int peer_ready(const sm_ctx *c);
int rccl_peer_sums_setup(sm_ctx *c);
int hosted_peer_sums_setup(sm_ctx *c);
int peer_set_view(sm_ctx *c);
double2 *face4_send(sm_ctx *c, int hi);
double2 *face4_recv_d(sm_ctx *c, long pass);
int halo4(sm_ctx *c, hipStream_t s, const double2 *field, double2 *recv);
// the fused CG kernel's 2-deep faces of nf <= 3 fields in one transport round
// (receive buffers faces[f]); halo2: one field on the main stream
int halo2_multi(sm_ctx *c, hipStream_t s, const double2 *const *fields, double2 *const *faces, int nf);
int halo2(sm_ctx *c, const double2 *field, double2 *face);

// Streamed CG buffers and the placement probe (sm_place.cpp)
size_t stream_alloc_bytes(size_t bytes, size_t floor_bytes = size_t(2) << 30);
hipError_t stream_malloc(sm_ctx *c, void **p, size_t bytes);
void stream_free(sm_ctx *c, void *p);
size_t link_code_bytes(long n);           // codes of n links (sm_linkcode.h), flag words and flag bytes
int placement_probe(sm_ctx *c, size_t fb);
int placement_probe_default();            // candidates per buffer for new contexts

// sm_cg_dev's fp64 solve (sm_capi.cpp), and the mixed-precision one it hands
// to when the context's cg_precision is 1 (sm_cgmp.cpp)
int cg_dev_fp64(sm_ctx *c, const double *phi, double *x, double m0, double tol, int max_iter, sm_cg_result *res);
int cg_dev_mixed(sm_ctx *c, const double *phi, double *x, double m0, double tol, int max_iter, sm_cg_result *res);
// The device calls of a one-column mixed solve (sm_cg_host.h MixedColumn) that
// do not depend on the operator. A solver adds true_residual, pass, fold and
// solve64 on its own.
struct MixedDev {
    sm_ctx *c;
    MixedWs &w;
    long n;                         // complex entries of a vector
    const double2 *phi;
    double tol;
    int max_iter;
    const char *tag, *stuck;        // of the debug lines; the error of a segment that does not end
    const MPScalars &h = *w.h_sc;
    sm_cg_mixed_info &info = w.info;
    float2 *const *d = w.d;
    double delta = c->mp_delta;
    int force_fallback = c->mp_force_fallback, debug = c->debug_cg;
    void copy(const double2 *a, double2 *b) { launch_copy(c->stream, n, a, b); }
    void add(double2 *x, const double2 *e) { launch_mp_add(c->stream, n, x, e); }
    void inject(const double2 *r, float2 *dprev, float2 *d0) { launch_mp_inject(c->stream, n, r, dprev, d0, w.sc); }
    int check() {
        HIP_TRY(hipGetLastError());
        return SM_OK;
    }
    int read() {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w.h_sc, w.sc, sizeof(MPScalars), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SM_OK;
    }
    // r = phi - Ax and what the driver decides on, read back
    int residual(const double2 *Ax, double2 *r, bool init, bool restart) {
        const int nb = launch_mp_residual(c->stream, n, phi, Ax, r, w.partials);
        launch_mp_update(c->stream, nb, w.partials, w.sc, init ? 1 : 0, restart ? 1 : 0, tol, delta, max_iter);
        return read();
    }
    int finish_vectors(double2 **rhs, double2 **e) {
        if (w.fin.empty()) TRY(w.fin.add(&w.fb, 2 * (size_t)n, BufKind::device, "finish vectors"));
        *rhs = w.fb;
        *e = w.fb + n;
        return SM_OK;
    }
};
// ---- the fp64 batched CG hosts (sm_cgbatch.cpp, sm_eobatch.cpp) ----
// A workspace for K columns of n complex with pstride complex of partials per
// column (the solver's BatchCfg::pstride, which does not depend on K), zeroed;
// SM_ERR_HIP names the bytes under w's `who` on failure and leaves w empty.
int batch_ws_alloc(sm_ctx *c, BatchWs &w, int K, long n, long pstride);
void batch_ws_free(BatchWs &w);
// The host of both solvers, the only copy: init(dbuf) starts the columns (x =
// phi, d_0 where pass 0 expects d_{-1}, the scalars), then up to max_iter + 1
// passes (pass 0 forms Ad_0; a column stops itself at k == max_iter) through
// cg_chunked_columns (sm_cg_host.h), pass(j, d_{j-1}, d_{j-2}, Ad_{j-1}, d_j,
// Ad_j) being the operator's launcher; after each chunk the flush and one read
// of all K scalar blocks; then finish-x and the results. tag: of the debug line.
template <class Init, class Pass>
int batch_cg_solve(sm_ctx *c, const BatchWs &w, const BatchCfg &cfg, int K, double2 *x, double tol, int max_iter,
                   sm_cg_result *res, const char *tag, Init init, Pass pass) {
    HIP_TRY(hipSetDevice(c->device));
    auto dbuf = [&](long i) { return w.d[((i % 3) + 3) % 3]; };
    init(dbuf);
    HIP_TRY(hipGetLastError());
    const CGScalars *h = w.h_sc;
    TRY(cg_chunked_columns(
        K, (long)max_iter + 1,
        [&](long j0, long nb) {
            for (long j = j0; j < j0 + nb; ++j) pass(j, dbuf(j - 1), dbuf(j - 2), w.a[(j + 1) & 1], dbuf(j), w.a[j & 1]);
            return SM_OK;
        },
        [&](long issued) {
            launch_batch_flush(c->stream, cfg, K, w.partials, w.sc, issued - 1);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(w.h_sc, w.sc, sizeof(CGScalars) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return SM_OK;
        },
        [&](int b) { return CgStatus{h[b].k, h[b].err, tol * h[b].phi_norm, h[b].done}; },
        [&](long issued, int open, int wish) {
            if (c->debug_cg) fprintf(stderr, "[%s] passes %ld open %d of %d next chunk %d\n", tag, issued, open, K, wish);
        }));
    launch_batch_finish_x(c->stream, K, w.n, x, w.d[0], w.d[1], w.d[2], w.sc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int b = 0; b < K; ++b) {
        res[b].converged = h[b].converged;
        res[b].iterations = h[b].k;
        res[b].residual = h[b].err;
        res[b].phi_norm = h[b].phi_norm;
    }
    return SM_OK;
}
// The two entry points on any such workspace: K columns of phi -> x, column b
// on l's links and mass (even-odd: even vectors, V complex apart, on l's
// checkerboard links).
int cg_batch_solve(sm_ctx *c, const BatchWs &w, int K, const double2 *phi, double2 *x, const BatchLinks &l,
                   double tol, int max_iter, sm_cg_result *res);
int eo_batch_solve(sm_ctx *c, const BatchWs &w, int K, const double2 *phi, double2 *x, const EoBatchLinks &l,
                   double tol, int max_iter, sm_cg_result *res);
// (sm_cgbatch.cpp) the context's device staging bt_phi / bt_x for K columns; and every batched solve
// of its entry points: K columns of phi -> x on the context's field with m0, fp64 on c->bt or the
// mixed solver (sm_cg_batch_precision), c->bt_info = the columns' reports
int batch_staging_ready(sm_ctx *c, int K);
int batch_solve(sm_ctx *c, int K, const double2 *phi, double2 *x, double m0, double tol, int max_iter,
                sm_cg_result *res);
// The context's even-odd batch workspace for K columns and its checkerboard link buffer (sm_eobatch.cpp)
int eob_ready(sm_ctx *c, int K);
// ---- the pion correlator's even-odd path (sm_pion.cpp) ----
// S_b = D^-1 phi_b for K point sources through the even-odd system, every stage
// one launch for all K columns: phihat_e = phi_e + (1/2m) H_eo phi_o, X =
// (Dhat Dhat^dag)^-1 phihat_e (eo_batch_solve on w and l, reported in res),
// S_e = Dhat^dag X, S_o = (1/m) phi_o + (1/2m) H_oe S_e. eh: five half-lattice
// fields of K x V complex; S: K full-layout columns.
int pion_eo_propagators(sm_ctx *c, const BatchWs &w, int K, const PionCols &src, double2 *eh, const EoBatchLinks &l,
                        double tol, int max_iter, sm_cg_result *res, double2 *S);
// The same from sources already in eh's first two fields (phi_e, phi_o): what
// pion_eo_propagators runs after writing its point sources, and the quark
// loops (sm_loops.cpp) after their noise.
int eo_propagators(sm_ctx *c, const BatchWs &w, int K, double2 *eh, const EoBatchLinks &l, double tol, int max_iter,
                   sm_cg_result *res, double2 *S);
// The context's even-odd batch workspace and pn_buf for K columns
int pion_eo_ready(sm_ctx *c, int K);
// sm_pion_correlator's body in mode 1 (arguments checked by the caller; sx / st: device)
int pion_correlator_eo(sm_ctx *c, double m0, double tol, int max_iter, int nsrc, const int *sx, const int *st,
                       double *C, sm_cg_result *res);
// The mixed-precision batched solve on the context's gauge field (sm_cgbatchmp.cpp):
// K columns of phi -> x on the device, c->bt_info[b] = column b's report.
int cg_batch_mixed(sm_ctx *c, int K, const double2 *phi, double2 *x, double m0, double tol, int max_iter,
                   sm_cg_result *res);

// even-odd preconditioned pseudofermion action (sm_eo.cpp); phi / chi in the
// full layout, only their even sites used
int eo_ready(sm_ctx *c);
// the fp64 building blocks the mixed even-odd solve (sm_eomp.cpp) stands on:
// out_e = Dhat v_e / Dhat^dag v_e, and the fp64 CG on Dhat Dhat^dag (x0 = b)
int eo_dhat(sm_ctx *c, int dagger, const double2 *v, double2 *out, double mass, const double2 *aux = nullptr,
            double2 *partials = nullptr, int *nparts = nullptr);
int eo_cg(sm_ctx *c, const double2 *b, double2 *x, double mass, double tol, int max_iter, sm_cg_result *res);
const double2 *eo_links(sm_ctx *c, int parity);  // the checkerboard links eo_ready made of the current U
// every even-odd solve of the library: eo_cg, or eo_cg_mixed when eo_cg_precision == 1
int eo_solve(sm_ctx *c, const double2 *b, double2 *x, double mass, double tol, int max_iter, sm_cg_result *res);
int eo_cg_mixed(sm_ctx *c, const double2 *b, double2 *x, double mass, double tol, int max_iter, sm_cg_result *res);
int eo_md_force(sm_ctx *c, const sm_hmc_params *p, const double2 *phi_full, double *F, sm_cg_result *res);
int eo_fermion_action(sm_ctx *c, const sm_hmc_params *p, const double2 *phi_full, double *S, sm_cg_result *res);
int eo_pseudofermion(sm_ctx *c, const sm_hmc_params *p, const double2 *chi_full, double2 *phi_full);

}  // namespace sm_host
