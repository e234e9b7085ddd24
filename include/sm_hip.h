/*
 * sm_hip.h -- C-ABI of the MI355X-native Wilson-Dirac / CG hot path
 * (libsm_hip.so). Plain pointers and sizes only; no HIP, RCCL or torch types.
 *
 * This is the drop-in boundary for Fabian2598/SchwingerModel's
 *   src/dirac_operator.cpp   (D_phi, D_dagger_phi, D_D_dagger_phi,
 *                             phi_dag_partialD_phi)
 *   src/conjugate_gradient.cpp (conjugate_gradient)
 *   include/variables.h:181-192 (dot)
 * Each entry point below names the reference function it replaces. A C++
 * shim with the reference's exact signatures (schwingermodel_amd/csrc/
 * dirac_operator_hip.cpp) is built on top of it; see INTEGRATION.md.
 *
 * Host field layout = the reference's spinor (include/variables.h:54-100):
 * for every field two separate arrays (mu0, mu1) of complex<double>, each
 * complex stored as (re, im) doubles, site n = x*Wt + t over this shard's
 * block (all Nx rows, Wt = Nt/nshard t-values starting at t0 = shard*Wt).
 * U: mu0 = U_t (mu = 0, t-direction), mu1 = U_x. re_field (force) = two
 * arrays of doubles.
 *
 * Device ("_dev") variants take ONE device buffer per field: plane mu0
 * followed by plane mu1 (2*Nx*Wt complex<double>), already resident in HBM.
 *
 * Multi-GPU: the lattice is sharded along t over nshard processes (one GPU
 * each), neighbours t+-1 exchanged over RCCL (xGMI). Every rank must call
 * every operator/CG entry point in lockstep, as in the reference (SPMD).
 *
 * Return codes: 0 = OK, nonzero = error (sm_last_error() describes it).
 * No C++ exceptions cross this boundary.
 */
#ifndef SM_HIP_H
#define SM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SM_OK 0
#define SM_ERR_ARG 1    /* bad argument / geometry                      */
#define SM_ERR_HIP 2    /* HIP runtime error (incl. no GPU)             */
#define SM_ERR_RCCL 3   /* RCCL error                                   */
#define SM_ERR_STATE 4  /* call out of order (e.g. no gauge uploaded)   */

typedef struct sm_ctx sm_ctx;

/* CG outcome (the reference returns only 1/0; it also prints err on failure,
 * src/conjugate_gradient.cpp:64-65). */
typedef struct {
    int converged;     /* 1 = ||r|| < tol*||phi||, 0 = max_iter reached   */
    int iterations;    /* loop passes (D D^dag applications in the loop)  */
    double residual;   /* ||r|| of the last iteration (reference "err")    */
    double phi_norm;   /* ||phi||                                          */
} sm_cg_result;

/* ---- library / host-only helpers (no GPU needed) ------------------------ */
int sm_abi_version(void);
const char *sm_last_error(void);

/* t-shard geometry: replaces include/mpi_setup.h:6-23 (assignWidth) for the
 * ranks_x = 1, ranks_t = nshard decomposition. */
int sm_shard_plan(int Nt, int nshard, int shard, int *t0, int *Wt);

/* Counter-based synthetic fields: gauge U = exp(i theta),
 * theta ~ N(0, sigma^2) (sigma > 0), uniform (sigma < 0, "hot"), 0 ("cold");
 * spinor as HMC::RandomCHI (src/hmc.cpp:19-28). Writes rows [x0, x0+nx),
 * t in [t0, t0+Wt) of the global Nx x Nt_global field. */
void sm_fill_gauge(uint64_t seed, double sigma, int Nt_global, int x0, int nx, int t0, int Wt,
                   double *U0, double *U1);
void sm_fill_spinor(uint64_t seed, int Nt_global, int x0, int nx, int t0, int Wt, double *p0,
                    double *p1);
/* Noise vector k of `seed` for the stochastic quark loops (sm_quark_loops):
 * eta_a(n) = (+-1 +- i) / sqrt(2), the two signs two bits of the counter hash
 * keyed by (seed, k), plane a and the global site. No libm call: bitwise the
 * values the device regenerates. The layout and the window arguments of
 * sm_fill_spinor. */
void sm_fill_noise(uint64_t seed, uint64_t k, int Nt_global, int x0, int nx, int t0, int Wt, double *p0,
                   double *p1);

/* 28-byte-record binary gauge configuration (src/gauge_conf.cpp:378-423
 * SaveConf / :495-546 readBinary): per site x-major, t-minor, mu = 0,1:
 * int32 x, int32 t, int32 mu, float64 re, float64 im. Global field. */
int sm_conf_write(const char *path, int Nx, int Nt, const double *U0, const double *U1);
int sm_conf_read(const char *path, int Nx, int Nt, double *U0, double *U1);

/* Number of visible GPUs (0 and an error code when there is none). */
int sm_device_count(int *n);

/* RCCL unique id for nshard > 1 (rank 0 creates, all ranks receive it). */
int sm_comm_unique_id(void *id_out, int id_bytes);  /* id_bytes >= 128 */

/* ---- context -------------------------------------------------------------- */
/* One context = one t-shard on one GPU. unique_id is ignored for nshard == 1. */
int sm_create(sm_ctx **out, int Nx, int Nt_global, int nshard, int shard, int device,
              const void *unique_id);

/* Host-staged transport (instead of RCCL) for nshard > 1: halos and scalar
 * all-reduces go through caller callbacks on host buffers. Used to run several
 * shards on ONE GPU (tests: torch.distributed gloo) or over a caller's own
 * MPI; slower than RCCL, same kernels and the same results.
 *   exchange: send_up -> shard+1 (arrives there as recv_lo),
 *             send_down -> shard-1 (arrives there as recv_hi); n doubles each.
 *   allreduce_sum: in-place global sum of n doubles, identical on all shards. */
typedef struct {
    void *user;
    int (*exchange)(void *user, const double *send_down, const double *send_up, double *recv_lo,
                    double *recv_hi, long n);
    int (*allreduce_sum)(void *user, double *buf, long n);
} sm_host_transport;
int sm_create_hosted(sm_ctx **out, int Nx, int Nt_global, int nshard, int shard, int device,
                     const sm_host_transport *transport);
/* RCCL loopback: ONE shard (the whole lattice) driven through the t-shard code
 * path -- faces packed and exchanged with ncclSend/ncclRecv to itself, scalar
 * sums through ncclAllReduce -- over a one-rank communicator built from
 * unique_id (sm_comm_unique_id). The results equal sm_create's one-shard
 * context; it exists so the RCCL data path can be verified on a single GPU. */
int sm_create_loopback(sm_ctx **out, int Nx, int Nt_global, int device, const void *unique_id);
/* Device-initiated shard transport ("peer", round 6; replaces the halo
 * MPI_Send/MPI_Recv of src/dirac_operator.cpp:66-88 and the dot's
 * MPI_Allreduce of include/variables.h:190 like the RCCL path does, without
 * RCCL). Each shard owns one region of uncached device memory; kernels store
 * faces and scalar sums straight into the neighbours' / every shard's region
 * over xGMI and publish sequence flags there; the receiving kernel waits on
 * the flags in its own region (one waiting thread, a time limit on every
 * wait). The recompute-Ad CG pass writes d_j's faces into the neighbours'
 * rings and all-reduces its sums in its own last block, so a pass is ONE
 * launch on ONE stream. Works between processes on one GPU as well (the
 * one-GPU tests) and needs no RCCL communicator.
 * Two steps, with any host-side all-gather in between:
 *   sm_create_peer writes this shard's region handle (sm_peer_handle_bytes()
 *   bytes) to handle_out; sm_peer_connect takes the nshard handles in rank
 *   order (handle_bytes_each apart), maps the others' regions, and checks the
 *   world with one all-reduce. The context is unusable for sharded work until
 *   then. */
int sm_peer_handle_bytes(void);
int sm_create_peer(sm_ctx **out, int Nx, int Nt_global, int nshard, int shard, int device, void *handle_out,
                   int handle_bytes);
int sm_peer_connect(sm_ctx *ctx, const void *handles, int handle_bytes_each);
/* One shard through the peer transport's t-shard path, its own neighbour on
 * both sides (the peer counterpart of sm_create_loopback). */
int sm_create_peer_loopback(sm_ctx **out, int Nx, int Nt_global, int device);
/* Synchronises the context's stream; SM_ERR_RCCL if a peer-transport wait
 * timed out (*timed_out_seq = its sequence number, 0 if none; may be NULL).
 * sm_cg_finish checks it too. SM_OK on other transports. */
int sm_peer_status(sm_ctx *ctx, unsigned long long *timed_out_seq);
int sm_destroy(sm_ctx *ctx);
/* Launch on a caller stream (a hipStream_t, e.g. torch's current stream);
 * NULL restores the context's own stream. Synchronises the previous stream
 * first. A sharded context has ONE RCCL communicator and orders every RCCL
 * operation on the GPU after the previous one (events between this stream and
 * the context's private comm stream, which carries the faces that travel under
 * an interior launch), in issue order: no two of its RCCL kernels are ever in
 * flight at once. */
int sm_set_stream(sm_ctx *ctx, void *hip_stream);
/* The context's communication world, read from the transport itself:
 * transport 0 = none (one shard), 1 = host-staged (sm_create_hosted),
 * 2 = RCCL (sm_create with nshard > 1, or sm_create_loopback), 3 = peer
 * (sm_create_peer: *nranks / *rank = the shards its connected view holds and
 * this one's place in it; the peer loopback: 1 / 0); for RCCL *nranks /
 * *rank = ncclCommCount / ncclCommUserRank of the RCCL communicator, and
 * 1 / 0 without one (the RCCL world of a host-staged or one-shard context is
 * this process alone). Any output pointer may be NULL. */
int sm_comm_info(const sm_ctx *ctx, int *transport, int *nranks, int *rank);
/* 1 if the recompute-Ad CG pass of a sharded context all-reduces its scalar
 * sums in its own last block (the peer transport; RCCL contexts whose shards
 * agreed on the peer headers at creation), 0 if it calls the transport's
 * all-reduce after each pass. */
int sm_cg_sums_in_pass(const sm_ctx *ctx, int *in_pass);
int sm_synchronize(sm_ctx *ctx);
/* Launch-geometry knobs of the stencil kernels (tuning / A-B benchmarks):
 * bt = t-columns per block (64, 128, 192 or 256: whole waves up to 256
 * threads; anything else is SM_ERR_ARG and leaves the setting as it was),
 * xchunk = rows marched per block (>= 1; may exceed Nx),
 * xcd_remap = 1 maps the tiles one XCD receives to x-adjacent tiles,
 * variant selects the stencil code variant. Values <= 0 (< 0 for xcd_remap
 * and variant) keep the current setting. */
int sm_tune(sm_ctx *ctx, int bt, int xchunk, int xcd_remap, int variant);
/* CG path: fused = 5 (the default from 256^2 sites per shard up) is the
 * two-direction iteration that recomputes
 * Ad_{j-1} = D D^dag d_{j-1} in-kernel instead of storing it (sm_cgra.hip):
 * 160 B/site. fused = 4 (the default on smaller shards) is the
 * two-direction one-pass iteration that stores Ad:
 * no r vector (r_{j-1} = d_{j-1} - beta_{j-2} d_{j-2} is rebuilt from the two
 * stored directions) and x updated on even passes only, 224 B/site.
 * fused = 0 is the reference's six-launch sequence (576 B/site). Other
 * values return SM_ERR_ARG (the two-pass and r-vector iterations of round 1
 * were dominated at every size and removed). xchunk = rows per block of the
 * active one-pass kernel. < 0 / <= 0 keep. */
int sm_tune_cg(sm_ctx *ctx, int fused, int xchunk);
/* Launch geometry of the recompute-Ad CG pass (fused = 5): waves per block
 * (1, 2 or 4; each wave owns 56 t-columns) and rows marched per block.
 * Values <= 0 keep the current setting. */
int sm_tune_cg_geometry(sm_ctx *ctx, int waves_per_block, int xchunk);
/* t-strip blocks of the recompute-Ad pass (one-shard contexts): strip = 1
 * makes each block's waves (4, or 2 after sm_tune_cg_geometry(ctx, 2, .))
 * march ONE strip of 64 * waves t-columns (8 of them halo; the stencil stages'
 * t-hops between its waves go through LDS) instead of one window of 56 owned
 * columns per wave; balanced = 1 splits x into XB equal chunks of
 * ~Nx/XB rows instead of xchunk-row chunks. < 0 keeps. SM_ERR_ARG on a
 * t-shard context. */
int sm_tune_cg_strip(sm_ctx *ctx, int strip, int balanced);
/* Compact links in the recompute-Ad CG pass (fused = 5, on by default from
 * 4M sites per shard): the pass reads each link as its smaller component v
 * (one double, exact) plus a 16-bit flag word -- which component v is, the
 * sign of the other, and the other's offset in ulps from sqrt(1 - v^2) -- and
 * rebuilds the link BITWISE in registers (schwingermodel_amd/csrc/
 * sm_linkcode.h): 20 instead of 32 B/site of links, 148 instead of 160 B/site
 * per iteration, and the same iterates as the complex-link pass. The codes are
 * rebuilt at the first solve after U changes, by a kernel that also decodes
 * every code with the pass's own decoder; they are used only if EVERY link
 * comes back bitwise (it does unless a link is off the unit circle by more
 * than ~1e-12 in |U|^2, far beyond the drift of the reference's leapfrog,
 * src/hmc.cpp:70-100), else the pass reads the complex links. D, D^dag and
 * the force always read the stored links. sm_cg_link_angles is the round-2
 * name of the same call (the code was then the link's angle). */
int sm_cg_link_codes(sm_ctx *ctx, int on, int *in_use);
/* Round-2 name of sm_cg_link_codes; same behaviour, kept for old callers.
 * on: 1 / 0 enable / disable, < 0 keep; *in_use (may be NULL): 1 if the last
 * sm_cg_begin / sm_cg set the codes up for the active path. The choice is
 * each context's own, also on t-shards: the codes are exact, so shards that
 * choose differently still compute bitwise the same iterates with the same
 * collectives (each shard checks its own links and the ghost links it
 * receives). */
int sm_cg_link_angles(sm_ctx *ctx, int on, int *in_use);
/* Bytes of link data per site the last CG pass launched on this context read,
 * recorded at its launch: 32 (complex links; every path but the recompute-Ad
 * pass), 20 (codes with 16-bit flag words) or 17 (codes with the flag
 * nibbles of both links packed into one byte, the form every field takes
 * whose ulp offsets all lie in [-2, 1], e.g. fresh exp(i theta) fields); 0
 * before the first pass. A later gauge upload or Metropolis reject does not
 * change it. The recompute-Ad pass streams 128 B/site besides. */
int sm_cg_link_bytes(const sm_ctx *ctx, int *bytes_per_site);
/* Precision of the solves that go through sm_cg_dev (sm_cg, sm_md_force(_dev),
 * sm_leapfrog(_dev), sm_hamiltonian(_dev), sm_hmc_trajectory, sm_hmc_run):
 * 0 = fp64 (default), 1 = mixed; < 0 keeps. SM_ERR_ARG on a sharded or loopback
 * context (v1 is one shard) and for other values; *mode_out (nullable) = current.
 * Mixed: the iterations run in fp32 (a recompute-Ad pass on float fields, 80
 * instead of 145-160 B/site) on a correction y to x, and reliable updates hold
 * the answer to the fp64 stop test: whenever the iterated residual has fallen
 * by 10x, x += y and r = phi - D D^dag x is recomputed in fp64, and the search
 * direction is kept across the replacement. The solve stops only on such a
 * true residual (sm_cg_result.residual), so x passes the same stop test as the
 * fp64 solve but is NOT the reference's iterate sequence: the two solutions
 * differ by up to the stop test's slack (~tol relative), not by 1e-12.
 * iterations counts the fp32 iterations plus any fp64 ones, and max_iter
 * bounds that sum. If two consecutive updates fail to lower the true residual,
 * or an fp32 scalar is not finite, the solve finishes in fp64 (D D^dag e = r,
 * x += e). sm_cg_begin / iterate / finish stay fp64; the even-odd solver has
 * its own switch (sm_eo_cg_precision below), independent of this one. The fp32
 * buffers are allocated at the first mixed solve. */
int sm_cg_precision(sm_ctx *ctx, int mode, int *mode_out);
typedef struct { int used; int inner_iterations; int reliable_updates;
                 int fp64_iterations; int fell_back; double true_residual; } sm_cg_mixed_info;
/* The last sm_cg_dev of the context: used = 1 if it ran mixed (else all zero),
 * the fp32 iterations, the fp64 true residuals taken after the initial one,
 * the iterations and the flag of the fp64 finish, and the last true residual
 * ||phi - D D^dag x|| / ||phi||. */
int sm_cg_mixed_last(const sm_ctx *ctx, sm_cg_mixed_info *out);  /* the last sm_cg_dev */
/* Diagnostic (tests): encode every link of the context's current U and decode
 * it again ON THE DEVICE with the CG pass's own functions. Writes the rebuilt
 * links to U_out_dev (device, the layout of sm_upload_gauge_dev; may be NULL),
 * the largest per-component |rebuilt - stored| to *max_err (0 when every link
 * comes back bitwise) and the count of links NOT rebuilt bitwise to *n_bad
 * (this shard only). Synchronous. */
int sm_link_code_check(sm_ctx *ctx, double *U_out_dev, double *max_err, long *n_bad);
/* Streaming-bandwidth ceiling on the ctx stream (measured roofline reference):
 * out = a + b (two_reads = 1: the stencil's 2-read/1-write byte mix) or
 * out = a, over n complex<double> device elements. */
int sm_bench_stream(sm_ctx *ctx, int two_reads, long n, const double *a, const double *b, double *out,
                    int blocks);
int sm_local_sites(const sm_ctx *ctx, long *V, int *Nx, int *Wt, int *t0);
/* Build id of this library: 16 hex digits of the SHA-256 of its sources,
 * headers and compile flags (schwingermodel_amd/build.py source_id). Profile
 * summaries under profiles/ record it, and bench.py cites only a summary of
 * the build that runs. */
const char *sm_build_id(void);
/* Placement probe of the context's creation (fields >= 256 MiB): the CG pass
 * runs at one of two speeds depending on where the driver physically places
 * its streamed buffers relative to each other, so creation searches one buffer
 * at a time (x, then the three direction buffers), trying up to
 * `candidates` fresh allocations of that buffer and keeping the fastest
 * (schwingermodel_amd/csrc/sm_place.cpp placement_probe; not on host-staged
 * contexts, where shard processes share one GPU); a sweep over the four
 * buffers that improved the pass by > 1 % is followed by another (at most 3).
 * *n = timings (0: no probe, else 1 + 4 per sweep), us_per_pass[0] (may be
 * NULL; room for 16) = median microseconds per pass of the initial placement,
 * us_per_pass[i] = after the search of the i-th buffer searched; *chosen = bit
 * mask of the buffers that moved, bit i = buffer i of the search order, whose
 * names sm_placement_buffer_name gives. */
int sm_placement_report(const sm_ctx *ctx, double *us_per_pass, int *n, int *chosen);
/* Name of bit i of sm_placement_report's mask ("x", "d1", "d0", "d2"; the
 * order the probe searches the buffers in), NULL past the last. */
const char *sm_placement_buffer_name(int i);
/* Candidates per buffer of the placement probe for contexts created after
 * this call (process-wide; default 3, 0 disables the probe, at most 8).
 * Transient memory while probing: that many allocations of one buffer.
 * SM_ERR_ARG for a value out of range, which leaves the setting as it was. */
int sm_set_placement_probe(int candidates);
/* The current process-wide setting of sm_set_placement_probe (callers that
 * change it temporarily restore this value). */
int sm_get_placement_probe(void);

/* Gauge field (host / device). Must precede every operator call; re-upload
 * whenever the caller changes U (the reference mutates U between calls,
 * src/hmc.cpp:69-99). */
int sm_upload_gauge(sm_ctx *ctx, const double *U0, const double *U1);
int sm_upload_gauge_dev(sm_ctx *ctx, const double *U_dev);

/* ---- operators, host pointers (drop-in; synchronous) ---------------------- */
/* D_phi (dagger = 0), src/dirac_operator.cpp:24; D_dagger_phi (dagger = 1), :247 */
int sm_dirac(sm_ctx *ctx, const double *in0, const double *in1, double *out0, double *out1,
             double m0, int dagger);
/* D_D_dagger_phi, src/dirac_operator.cpp:477 */
int sm_ddag(sm_ctx *ctx, const double *in0, const double *in1, double *out0, double *out1,
            double m0);
/* phi_dag_partialD_phi(U, left, right) -> re_field, src/dirac_operator.cpp:486 */
int sm_force(sm_ctx *ctx, const double *l0, const double *l1, const double *r0, const double *r1,
             double *F0, double *F1);
/* dot(a, b) = sum a conj(b) over all shards, include/variables.h:181. out = (re, im) */
int sm_dot(sm_ctx *ctx, const double *a0, const double *a1, const double *b0, const double *b1,
           double *out);
/* conjugate_gradient(U, phi, x, m0), src/conjugate_gradient.cpp:4: solves
 * D D^dag x = phi with x0 = phi and the stop test ||r|| < tol ||phi||. */
int sm_cg(sm_ctx *ctx, const double *phi0, const double *phi1, double *x0, double *x1, double m0,
          double tol, int max_iter, sm_cg_result *res);

/* ---- operators, device-resident fields (asynchronous on the ctx stream) --- */
int sm_dirac_dev(sm_ctx *ctx, const double *in, double *out, double m0, int dagger);
int sm_ddag_dev(sm_ctx *ctx, const double *in, double *out, double m0);
int sm_force_dev(sm_ctx *ctx, const double *l, const double *r, double *F);
int sm_dot_dev(sm_ctx *ctx, const double *a, const double *b, double *out_host); /* syncs */
int sm_cg_dev(sm_ctx *ctx, const double *phi, double *x, double m0, double tol, int max_iter,
              sm_cg_result *res);
/* Stepwise CG for benchmarking: begin (x = phi, r, d, norms), enqueue n
 * iterations without host synchronisation, then read the status (syncs). */
int sm_cg_begin(sm_ctx *ctx, const double *phi, double *x, double m0, double tol);
int sm_cg_iterate(sm_ctx *ctx, int n);
int sm_cg_status(sm_ctx *ctx, sm_cg_result *res);
/* End a stepwise solve: apply the x update the fused iteration defers to the
 * next pass (x += alpha_{k-1} d_{k-1}), then report like sm_cg_status. Until
 * then x lags one update behind the reference's x; on fields of 256 MiB and
 * more (4096^2 / 2 planes and up) the passes work on an internal x, and the
 * caller's x holds the solution only after this call. */
int sm_cg_finish(sm_ctx *ctx, sm_cg_result *res);

/* ==== gauge field, molecular dynamics and HMC =====
 * The next layer out from the Dirac/CG path: the whole MD force step of
 * src/hmc.cpp with U, momenta and forces resident on the device (the drop-in
 * shim above re-uploads U per call; these never do). Every sum is global over
 * shards (all ranks call in lockstep). Momenta: two planes of V doubles. */

/* Copy this shard's gauge field to the host (reference layout). */
int sm_download_gauge(sm_ctx *ctx, double *U0, double *U1);
/* Draw the gauge field on the device with the sm_fill_gauge generator
 * (sigma > 0 Gaussian angle, < 0 hot start as GaugeConf::initialization
 * src/gauge_conf.cpp:32-37, 0 cold). Same distribution as the host draw;
 * the device's log/sincos may differ from glibc in the last bit. */
int sm_fill_gauge_dev(sm_ctx *ctx, uint64_t seed, double sigma);

/* Compute_Plaquette01 + MeasureSp_HMC + Compute_gaugeAction
 * (src/gauge_conf.cpp:41-85, 430-453): *sp = sum_n Re U_01(n),
 * *gauge_action = sum_n beta Re(1 - U_01(n)). plaq (host, nullable) receives
 * this shard's U_01(n) field (V complex). */
int sm_plaquette(sm_ctx *ctx, double beta, double *sp, double *gauge_action, double *plaq);
/* GaugeConf::Compute_Staple (src/gauge_conf.cpp:89-373): both directions,
 * host output (reference spinor layout). */
int sm_staples(sm_ctx *ctx, double *S0, double *S1);
/* HMC::Force_G (src/hmc.cpp:31-40): F += -beta Im(U conj(staple)), host F. */
int sm_gauge_force(sm_ctx *ctx, double beta, double *F0, double *F1);

/* HMC parameters (src/main.cpp:19-27 inputs + the CG settings). */
typedef struct {
    double m0;          /* bare mass                                       */
    double beta;        /* gauge coupling                                  */
    double tau;         /* trajectory length                               */
    int md_steps;       /* leapfrog steps (the reference evaluates the force
                           md_steps - 1 times, src/hmc.cpp:76)             */
    double cg_tol;      /* CG::tol (1e-10 in src/main.cpp:27)              */
    int cg_max_iter;    /* CG::max_iter (10000)                            */
    uint64_t seed;      /* counter-based draws: momenta, sources, Metropolis */
    int even_odd;       /* 0: the reference's action phi^dag (DD^dag)^-1 phi;
                           1: the even-odd preconditioned action
                           phi_e^dag (Dhat Dhat^dag)^-1 phi_e, same gauge
                           distribution, one half-lattice CG per force
                           (even Nx and shard width, shards >= 4 wide;
                           see sm_eo_* below)                               */
} sm_hmc_params;

/* HMC::Force (src/hmc.cpp:44-60) at the current U: psi = (DD^dag)^-1 phi,
 * F = phi_dag_partialD_phi(U, psi, D^dag psi) + gauge force. res: the CG. */
int sm_md_force(sm_ctx *ctx, const sm_hmc_params *p, const double *phi0, const double *phi1, double *F0,
                double *F1, sm_cg_result *res);
int sm_md_force_dev(sm_ctx *ctx, const sm_hmc_params *p, const double *phi, double *F, sm_cg_result *res);
/* HMC::Leapfrog (src/hmc.cpp:63-101): evolves the context's U and the
 * momenta P (in/out) along one trajectory; *cg_iters = CG loop passes summed
 * over the force evaluations; *cg_failures = non-converged solves. */
int sm_leapfrog(sm_ctx *ctx, const sm_hmc_params *p, const double *phi0, const double *phi1, double *P0,
                double *P1, long *cg_iters, int *cg_failures);
int sm_leapfrog_dev(sm_ctx *ctx, const sm_hmc_params *p, const double *phi, double *P, long *cg_iters,
                    int *cg_failures);
/* HMC::Hamiltonian (src/hmc.cpp:104-148) at the current U:
 * H = sum 0.5 P^2 + (beta sum Re(1 - U_01) + Re dot((DD^dag)^-1 phi, phi)). */
typedef struct {
    double H;             /* the Hamiltonian                                */
    double kinetic;       /* sum 0.5 P^2                                    */
    double gauge_action;  /* beta sum Re(1 - U_01)                          */
    double fermion;       /* Re dot((DD^dag)^-1 phi, phi)                   */
    double sp;            /* sum Re U_01                                    */
    int cg_iterations;
    int cg_converged;
} sm_hamiltonian_terms;
int sm_hamiltonian(sm_ctx *ctx, const sm_hmc_params *p, const double *phi0, const double *phi1, const double *P0,
                   const double *P1, sm_hamiltonian_terms *out);
int sm_hamiltonian_dev(sm_ctx *ctx, const sm_hmc_params *p, const double *phi, const double *P,
                       sm_hamiltonian_terms *out);

/* One HMC update, HMC::HMC_Update (src/hmc.cpp:151-178), entirely on the
 * device: momenta and chi drawn for trajectory `traj` (counter-based, the
 * same on every rank), phi = D chi, leapfrog on a copy of U, Metropolis with
 * r = uniform(seed, traj) (identical on all ranks, no broadcast). On reject
 * the previous U is restored by a buffer swap. */
typedef struct {
    double H_old, H_new, dH;
    double r;              /* the Metropolis uniform                          */
    int accepted;
    double sp;             /* sum Re U_01 of the configuration kept           */
    double gauge_action;   /* beta sum Re(1 - U_01) of the configuration kept */
    long cg_iterations;    /* all solves: H_old, the forces, H_new            */
    int cg_failures;
} sm_hmc_result;
int sm_hmc_trajectory(sm_ctx *ctx, const sm_hmc_params *p, uint64_t traj, sm_hmc_result *out);

/* One pure-gauge (quenched) molecular-dynamics trajectory on the device:
 * HMC::Leapfrog (src/hmc.cpp:63-101, with its loop bound) driven by
 * HMC::Force_G alone (:31-40, p->beta), momenta drawn for `traj` as in
 * sm_hmc_trajectory; the evolved U is kept (no Metropolis step). No CG runs,
 * so it evolves large fields cheaply through the leapfrog's own link update
 * U <- U exp(i eps P), whose rounding moves |U| off 1 the way an HMC does
 * (bench.py times the CG on such a field). p->m0, cg_* and even_odd unused. */
int sm_quenched_trajectory(sm_ctx *ctx, const sm_hmc_params *p, uint64_t traj);

/* HMC::HMC_algorithm (src/hmc.cpp:181-213): optional hot start
 * (GaugeConf::initialization, drawn on the device), Ntherm thermalisation
 * updates, then Nmeas measurements of Sp and the gauge action separated by
 * Nsteps decorrelation updates. Ep = mean(Sp)/V, dEp = Jackknife_error(Sp,
 * 20)/V, gS and dgS likewise (src/statistics.cpp:4-34, restated with its
 * integer binning), V = Nx*Nt. Trajectories are numbered 0, 1, ... from
 * first_traj (the counter-based draws' key). acceptance = accepted /
 * (Nmeas + Nsteps*(Nmeas-1)): the updates of the measurement phase (the
 * reference's SimData value, src/main.cpp:169). sp_series / gs_series
 * (nullable, Nmeas doubles) receive the measured Sp / gauge action.
 * save_prefix (nullable): after measurement i, shard 0 writes
 * <save_prefix>_<i>.ctxt in the 28-byte record format (SaveConf). */
typedef struct {
    double Ep, dEp, gS, dgS;
    double acceptance;
    long accepted;          /* measurement-phase accepts                  */
    long trajectories;      /* all updates run                            */
    long cg_iterations;
    int cg_failures;
    int cg_link_bytes;      /* link bytes per site the CG pass read in the last
                               solve (sm_cg_link_bytes: 32 complex links, 20
                               codes + flag words, 17 codes + packed flags) */
} sm_hmc_summary;
int sm_hmc_run(sm_ctx *ctx, const sm_hmc_params *p, int hot_start, uint64_t first_traj, int Ntherm, int Nmeas,
               int Nsteps, const char *save_prefix, sm_hmc_summary *out, double *sp_series, double *gs_series);

/* Jackknife_error (src/statistics.cpp:25-34) with its binning as written:
 * bin blocks of n/bin samples; leftover samples only enter the mean. */
double sm_jackknife_error(const double *dat, int n, int bin);

/* Even-odd pieces, for tests and callers of the preconditioned action:
 * Dhat = m - (1/m) D_eo D_oe on the even sites (m = m0 + 2): out = Dhat in
 * (dagger = 0) or Dhat^dag in, on the even sites of full-layout fields (odd
 * sites of out are 0); sm_eo_cg solves Dhat Dhat^dag x = phi_e the same way.
 * t-sharded contexts exchange 2-column checkerboard faces per hop (SM_ERR_ARG
 * for odd Nx, odd shard width or shards narrower than 4). */
int sm_eo_dhat(sm_ctx *ctx, int dagger, const double *in0, const double *in1, double *out0, double *out1,
               double m0);
int sm_eo_cg(sm_ctx *ctx, const double *phi0, const double *phi1, double *x0, double *x1, double m0, double tol,
             int max_iter, sm_cg_result *res);
/* sm_eo_cg on device-resident full-layout fields (the layout of sm_cg_dev): no
 * host transfers; x's odd sites are set to 0. Synchronous. */
int sm_eo_cg_dev(sm_ctx *ctx, const double *phi, double *x, double m0, double tol, int max_iter,
                 sm_cg_result *res);
/* Precision of the even-odd solver: sm_eo_cg(_dev) and every even-odd solve inside
 * sm_md_force(_dev), sm_leapfrog(_dev), sm_hamiltonian(_dev), sm_hmc_trajectory
 * and sm_hmc_run when p->even_odd = 1. 0 = fp64 (default), 1 = mixed; < 0
 * keeps. SM_ERR_ARG (mode stays 0) on sharded, loopback and peer contexts and
 * for other values; *mode_out (nullable) = current. Independent of
 * sm_cg_precision: either switch changes only its own solver.
 * Mixed: the scheme of sm_cg_precision on Dhat Dhat^dag. The iterations run
 * the one-pass even-odd kernel on float2 checkerboard fields (128 instead of
 * 256 B per even site) on a correction y to x; whenever the iterated residual
 * has fallen by 10x, x += y and r = phi_e - Dhat Dhat^dag x is recomputed in
 * fp64, and the search direction is kept. The solve stops only on such a true
 * residual, so x passes the fp64 stop test but is not the fp64 iterate
 * sequence. iterations = fp32 + fp64 iterations, bounded by max_iter. Two
 * consecutive updates that fail to lower the true residual, or a bad fp32
 * scalar, finish in fp64 (Dhat Dhat^dag e = r through the fp64 even-odd CG,
 * x += e). The fp32 buffers are allocated at the first mixed even-odd solve. */
int sm_eo_cg_precision(sm_ctx *ctx, int mode, int *mode_out);
/* The context's last even-odd solve, as sm_cg_mixed_last: all zero if it ran
 * fp64; true_residual = ||phi_e - Dhat Dhat^dag x|| / ||phi_e||. */
int sm_eo_cg_mixed_last(const sm_ctx *ctx, sm_cg_mixed_info *out);

/* ==== batched multi-source CG and the pion correlator =======================
 * D D^dag x_b = phi_b for K right-hand sides on the context's current gauge
 * field, ONE launch per iteration for the whole batch (schwingermodel_amd/
 * csrc/sm_cgbatch.hip). Below 256^2 a lone solve's iteration costs the same
 * 11-12 us whatever the lattice (launch + each block's dependent loads); K
 * columns share that cost. Each column runs the stored-Ad two-direction
 * iteration of sm_tune_cg's fused = 4 -- the reference's iterate sequence
 * (src/conjugate_gradient.cpp:31-63, x0 = phi) to ~1e-12 -- with its own alpha,
 * beta, residual and stop test ||r_b|| < tol ||phi_b||; a column that has
 * stopped costs nothing more, and its x, iteration count and residual are
 * those of the moment it stopped. A column's result does not depend on K, on
 * its position in the batch or on the other columns: bitwise the same alone
 * and in any batch.
 * Layout: K columns, contiguous, column b at offset b * 2*Nx*Nt complex, each
 * laid out as sm_cg_dev's field (plane mu0, then plane mu1). x must not alias
 * phi. res[b] reports column b exactly as sm_cg_result reports a lone solve.
 * Returns SM_OK also when some columns reach max_iter (res[b].converged says
 * so); SM_ERR_ARG for K < 1, K > sm_cg_batch_max(), a null pointer, and on
 * sharded, host-staged, loopback and peer contexts (version 1 is one shard);
 * SM_ERR_STATE before a gauge upload; SM_ERR_HIP when the workspace cannot be
 * allocated (sm_last_error() names the bytes asked for; the context stays
 * usable).
 * fp64 unless sm_cg_batch_precision (below) says otherwise: sm_cg_precision
 * and sm_eo_cg_precision do not reach it.
 * Traffic per site and column: 224 B per iteration (read d_{j-1}, d_{j-2},
 * Ad_{j-1}: 96; write d_j, Ad_j: 64; x read + written every other pass: 32
 * mean; links 32, from cache after the first column). Workspace, allocated at
 * the first batched solve, regrown when a later call has a larger K and freed
 * by sm_destroy: three direction and two Ad buffers, 160 B per site and
 * column (the host-pointer entry and the correlator stage phi and x on the
 * device: 64 B more), plus 48 B of partial sums per column and (60 t-columns
 * x G rows) with G = 1 below Nx = 512, 8 from there, and one scalar block per
 * column. It shares no buffer or state with sm_cg_begin / iterate / finish,
 * sm_cg_dev, the mixed or the even-odd solvers, and keeps nothing derived
 * from the gauge field: an upload or an HMC trajectory between two batched
 * solves needs no call. Synchronous. */
int sm_cg_batch_max(void);   /* largest K accepted (64) */
int sm_cg_batch_dev(sm_ctx *ctx, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                    sm_cg_result *res /* K */);
/* The same with host pointers (K columns in the layout above). */
int sm_cg_batch(sm_ctx *ctx, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                sm_cg_result *res /* K */);
/* Precision of sm_cg_batch, sm_cg_batch_dev and the solve inside
 * sm_pion_correlator, and of nothing else: 0 = fp64 (default; the code above,
 * unchanged), 1 = mixed; < 0 keeps. SM_ERR_ARG (mode stays as it was) for mode 1
 * on sharded, host-staged, loopback and peer contexts and for other values;
 * *mode_out (nullable) = current. Independent of sm_cg_precision and
 * sm_eo_cg_precision in both directions; the replica ensemble stays fp64.
 * Mixed: the scheme of sm_cg_precision applied to every column. The iterations
 * run the batch's stored-Ad pass on float2 fields (112 instead of 224 B per
 * site and column), K columns per launch, on a correction y_b to x_b; whenever
 * column b's iterated residual has fallen by 10x its segment ends (the column
 * idles until the slowest column's has), x_b += y_b and r_b = phi_b -
 * D D^dag x_b is recomputed in fp64 for all open columns at once, and the
 * search direction is kept. A column stops only on such a true residual
 * (res[b].residual, converged), so x_b passes the fp64 stop test but is NOT the
 * reference's iterate sequence; iterations = fp32 + fp64 iterations, bounded by
 * max_iter per column. A column whose two consecutive updates fail to lower the
 * true residual, or with a non-finite fp32 scalar (an all-zero or a huge
 * source), finishes in fp64 after the others: D D^dag e = r_b through the fp64
 * batched solver with K = 1, x_b += e. As in fp64, a column's bits depend on
 * that column, the gauge field and the arguments only.
 * Memory: 96 B of fp32 and 96 B of fp64 work per site and column (the fp64
 * workspace of 160 B is not allocated unless a column takes the fp64 finish,
 * and then for one column), allocated at the first mixed batched solve and
 * regrown for a larger K; the fp32 links (16 B per site) are converted from
 * the current gauge field at the start of every solve, so nothing derived from
 * it is kept here either.
 * When to switch it on (whole solves to 1e-10 against the fp64 batch, DESIGN.md
 * section 3.8 has every row): from 128^2 with K >= 8 (1.14-1.27x) and from
 * 256^2 for every K (1.44-1.48x; 1024^2: 1.55-1.75x). Not at 64^2 (0.69-0.86x
 * for K <= 16, 1.03x at K = 64: two launches per iteration where the fp64
 * batch has one) nor at 128^2 with K = 1. At 1024^2 K sequential sm_cg_dev
 * solves in mixed mode (sm_cg_precision) are as fast or faster. */
int sm_cg_batch_precision(sm_ctx *ctx, int mode, int *mode_out);
/* The K columns of the context's last sm_cg_batch(_dev) or sm_pion_correlator
 * (K = 2 nsrc), as sm_cg_mixed_last: out[b].used = 1 if it ran mixed, else all
 * zero. SM_ERR_ARG when K is not that solve's column count. */
int sm_cg_batch_mixed_last(const sm_ctx *ctx, int K, sm_cg_mixed_info *out /* K */);

/* Pion correlator from nsrc point sources on the current gauge field. For
 * source s and spin a in {0, 1}: phi = the unit vector at site (src_x[s],
 * src_t[s]) of plane a (built on the device), y_a = (D D^dag)^-1 phi in ONE
 * batched solve of 2 nsrc columns (2 nsrc <= sm_cg_batch_max()), S_a =
 * D^dag y_a = D^-1 phi, and
 *   C[s*Nt + t] = sum_x sum_a (|S_a,0(x,t)|^2 + |S_a,1(x,t)|^2) = sum_x tr S S^dag,
 * the pion by gamma5-hermiticity. t is the absolute time coordinate (the
 * caller shifts by src_t[s]). The sums run in a fixed order without atomics:
 * repeated calls agree bitwise. C: nsrc*Nt doubles on the host; res
 * (nullable): the 2 nsrc solves, column 2 s + a. SM_ERR_ARG for nsrc < 1,
 * 2 nsrc above the cap or a coordinate out of range; otherwise as
 * sm_cg_batch. Memory: 224 B per site and column while it runs. */
int sm_pion_correlator(sm_ctx *ctx, double m0, double tol, int max_iter, int nsrc, const int *src_x,
                       const int *src_t, double *C /* nsrc*Nt, host */, sm_cg_result *res /* 2*nsrc, nullable */);

/* The solve inside sm_pion_correlator: 0 = D D^dag as described above (default;
 * that code path, unchanged), 1 = through the even-odd system; < 0 keeps.
 * *mode_out (nullable) = current. SM_ERR_ARG (mode stays as it was) for mode 1
 * on sharded, host-staged, loopback and peer contexts and for other values.
 * Mode 1, with m = m0 + 2, D = m - H/2 and Dhat = m - (1/4m) H_eo H_oe, for all
 * 2 nsrc columns at once, every stage one launch:
 *   phihat_e = phi_e + (1/2m) H_eo phi_o,  X = (Dhat Dhat^dag)^-1 phihat_e
 *   (sm_eo_cg_batch's solver, about 0.4-0.5x the iterations of D D^dag),
 *   S_e = Dhat^dag X,  S_o = (1/m) phi_o + (1/2m) H_oe S_e,
 * then the same slice sums. res reports the even-odd solves (the stop test is
 * ||r|| < tol ||phihat_e||). Always fp64, whatever sm_cg_batch_precision says.
 * C and res are bitwise sm_ens_pion_correlator's with solver 1 on the same
 * field and mass. Odd Nx or Nt in mode 1 fails sm_pion_correlator (not this
 * switch) with SM_ERR_ARG; mode 0 keeps working. Memory in mode 1: sm_eo_cg_batch's
 * workspace plus 112 B per site and column of half-lattice fields and
 * propagators, from the first such call on. */
int sm_pion_solver(sm_ctx *ctx, int mode, int *mode_out);

/* ==== batched even-odd CG ====================================================
 * Dhat Dhat^dag x_b = phi_b on the even sites for K right-hand sides on the
 * context's current gauge field, ONE launch per iteration for the whole batch
 * (schwingermodel_amd/csrc/sm_eobatch.hip): the batched counterpart of
 * sm_eo_cg_dev. Each column runs the one-pass even-odd iteration of
 * sm_eo_cg's default path (the two-direction recurrence, both Dhat^dag and
 * Dhat in one march) with its own alpha, beta, residual and stop test
 * ||r_b|| < tol ||phi_b,e||; a column that has stopped costs nothing more. A
 * column's result depends on its own source, the gauge field, m0, tol and
 * max_iter only: bitwise the same alone, at any position of any batch and
 * next to any other columns.
 * Layout: K full-layout columns as in sm_cg_batch. The even part of phi_b
 * ((x + t) even) is the source, its odd part is ignored; x_b's odd sites are
 * set to 0. x must not alias phi. res[b] reports column b as sm_cg_result
 * reports a lone sm_eo_cg_dev. Returns SM_OK also when some columns reach
 * max_iter. SM_ERR_ARG for K < 1, K > sm_cg_batch_max(), a null pointer, x
 * aliasing phi, max_iter < 0, odd Nx or Nt, and on sharded, host-staged,
 * loopback and peer contexts; SM_ERR_STATE before a gauge upload; SM_ERR_HIP
 * when an allocation fails (sm_last_error() names the bytes asked for; the
 * context stays usable).
 * Always fp64: sm_cg_precision, sm_eo_cg_precision and sm_cg_batch_precision
 * do not reach it.
 * Traffic per even site and column: ~256 B per iteration (sm_eotd.hip's).
 * Memory, allocated at the first call, regrown for a larger K and freed by
 * sm_destroy: three direction and two Ad buffers on the half lattice (80 B per
 * site and column), the columns' even parts (32 B per site and column; the
 * host-pointer entry stages phi and x on the device: 64 B more), the
 * checkerboard copy of the gauge field (32 B per site), partial sums (48 B per
 * column and (56 k-columns x G rows), G = 2 below Nx = 512, 8 from there) and
 * one scalar block per column. It shares no buffer or state with sm_eo_cg /
 * sm_eo_cg_dev, the mixed solvers, sm_cg_batch or the stepwise solver; the
 * checkerboard links are rebuilt from the current gauge field at every call,
 * so an upload or an HMC trajectory between two solves needs no call.
 * Synchronous. */
int sm_eo_cg_batch_dev(sm_ctx *ctx, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                       sm_cg_result *res /* K */);
/* The same with host pointers. */
int sm_eo_cg_batch(sm_ctx *ctx, int K, const double *phi, double *x, double m0, double tol, int max_iter,
                   sm_cg_result *res /* K */);

/* ==== replica ensemble: R independent HMC chains, one launch per step ========
 * R <= sm_ens_max() gauge fields in one context, evolved in lockstep: every CG
 * iteration and every molecular-dynamics kernel is ONE launch for all replicas
 * (schwingermodel_amd/csrc/sm_ens.cpp). A lone chain on a 16^2-256^2 lattice
 * is bound by launch latency (11-12 us per CG iteration whatever the lattice);
 * R chains -- more statistics, or one chain per (beta, m0) point of a scan --
 * share that cost. Replica r has its own m0, beta, tau and seed; md_steps,
 * cg_tol, cg_max_iter and even_odd (0 or 1) are common (the replicas share
 * every launch): anything else is SM_ERR_ARG naming the field.
 * sm_ens_hmc_trajectory is HMC::HMC_Update (src/hmc.cpp:151-178) for every
 * replica at once: the draws, phi = D chi, H_old (one batched solve of R
 * columns, column r on replica r's links and mass), the leapfrog with the
 * reference's loop bound (md_steps - 1 batched force solves), H_new, and a
 * Metropolis step per replica with r = uniform(seed_r, traj). out[r] reports
 * replica r as sm_hmc_result reports a lone chain; cg_iterations counts the
 * replica's own column, not the slowest one.
 * What a replica computes depends on its own field, parameters and seed only:
 * bitwise the same alone (R = 1), at any position of any ensemble, whatever
 * the other replicas hold. Its draws are those of a lone chain with p[r].seed
 * (sm_traj_seed(seed, traj); the hot start of sm_ens_hmc_run from
 * sm_traj_seed(seed, ~0), as sm_hmc_run). sp and gauge_action are bitwise what
 * sm_plaquette gives a lone context holding the same field; quantities
 * downstream of a CG solve agree with the lone chain to the solvers' rounding
 * (the batched CG sums in another order than sm_cg_dev's), so a lone chain and
 * a replica started alike drift apart like two decompositions of one chain.
 * A rejected replica gets its previous field back bitwise (a device copy of
 * that replica only). Always fp64: sm_cg_precision and sm_eo_cg_precision do
 * not reach it. The ensemble owns its fields (U and its backup, momenta,
 * force, chi, phi, x: 192 B per site and replica) and its solver workspace
 * (160 B per site and replica); the context's gauge field, sm_cg_dev,
 * sm_cg_batch, the stepwise solver and their buffers are untouched by any
 * ensemble call. It works on the context's stream; destroy it before the
 * context. SM_ERR_ARG on sharded, host-staged, loopback and peer contexts, for
 * R < 1 or R > sm_ens_max(), r out of range and null pointers; SM_ERR_STATE
 * while some replica has no gauge field; SM_ERR_HIP (sm_last_error() names the
 * bytes asked for) when an allocation fails, after which the context stays
 * usable. Synchronous.
 * even_odd = 1 for every replica: replica r does what sm_hmc_trajectory does
 * with even_odd = 1 and p[r] -- the same draws, phi_e = Dhat chi_e, H =
 * kinetic + gauge + Re <X, phi_e> with X from ONE batched even-odd solve of R
 * columns on the replicas' own links and masses (sm_eo_cg_batch's solver), the
 * force from the bilinear of l = (X, (1/2m) H'_oe X) and r = (Y, (1/2m) H_oe Y),
 * Y = Dhat^dag X. It samples the same gauge distribution with about 0.4x the
 * CG iterations. What is said above about bitwise independence, the draws, sp
 * and gauge_action, rejected replicas and the agreement with a lone chain
 * holds for it too. Odd Nx or Nt with even_odd = 1 is SM_ERR_ARG (an odd
 * periodic lattice has no checkerboard); the ensemble stays usable for the
 * plain action, whose path and results do not change, and plain and even-odd
 * trajectories may alternate on one ensemble. The even-odd fields are
 * allocated at the first even-odd trajectory, not by sm_ens_create: 208 B per
 * site and replica (checkerboard links 32, six half-lattice fields 96, the
 * batched even-odd solver's workspace 80).
 * Not in this version: t-sharded ensembles, mixed precision, the sm_hmc
 * program. */
typedef struct sm_ens sm_ens;
int sm_ens_max(void);   /* = sm_cg_batch_max() */
int sm_ens_create(sm_ctx *ctx, int R, sm_ens **out);   /* allocates all fields */
int sm_ens_destroy(sm_ens *e);
int sm_ens_size(const sm_ens *e, int *R);
/* Replica r's field, as sm_upload_gauge / sm_download_gauge / sm_fill_gauge_dev */
int sm_ens_upload_gauge(sm_ens *e, int r, const double *U0, const double *U1);
int sm_ens_download_gauge(sm_ens *e, int r, double *U0, double *U1);
int sm_ens_fill_gauge(sm_ens *e, int r, uint64_t seed, double sigma);
/* sp[r] = sum Re U_01, gauge_action[r] = beta[r] sum Re(1 - U_01) of replica r:
 * one launch and one synchronisation for all R, bitwise sm_plaquette's values */
int sm_ens_plaquette(sm_ens *e, const double *beta /* R */, double *sp /* R */, double *gauge_action /* R */);
/* The pion correlator of every replica on its current field with its own mass
 * m0[r], from nsrc point sources common to all replicas; the definitions are
 * sm_pion_correlator's (unit vector at (src_x[s], src_t[s]) of plane a, S_a =
 * D^-1 phi, absolute t). C[(r*nsrc + s)*Nt + t]; res[(r*nsrc + s)*2 + a]
 * (nullable). For each (source, spin) pair ONE batched solve of R columns,
 * column r on replica r's links and mass, and one slice launch per source for
 * all replicas.
 * solver 0: y = (D D^dag)^-1 phi, S = D^dag y. Replica r's C and res are
 * bitwise what sm_pion_correlator (default settings) returns on a lone context
 * holding the same field with m0[r].
 * solver 1: the even-odd system as under sm_pion_solver; res reports the
 * even-odd solves. Needs even Nx and Nt: SM_ERR_ARG naming the checkerboard
 * otherwise, and the ensemble stays usable for solver 0. Its fields are those
 * of the even-odd action, allocated at first use.
 * A replica's C and res depend on its field, its mass and the arguments only:
 * bitwise the same at R = 1, at any position and next to any neighbours; fixed
 * summation order, no atomics, so repeated calls agree bitwise. Always fp64:
 * none of the precision switches reaches it. It works in the ensemble's chi,
 * phi, x and solver workspaces, free between trajectories; new memory is the
 * source coordinates and C on the device. A trajectory after a measurement is
 * bitwise the trajectory without it; the context's gauge field, solvers and
 * sm_pion_correlator are untouched. SM_ERR_ARG for a null ensemble, m0, src_*
 * or C, solver not 0 or 1, nsrc < 1 or 2 nsrc > sm_cg_batch_max(), a
 * coordinate outside the lattice, max_iter < 0; SM_ERR_STATE while some replica
 * has no gauge field; SM_ERR_HIP naming the bytes when an allocation fails (the
 * ensemble stays usable). Synchronous. */
int sm_ens_pion_correlator(sm_ens *e, const double *m0 /* R */, double tol, int max_iter, int solver, int nsrc,
                           const int *src_x, const int *src_t, double *C /* R*nsrc*Nt, host */,
                           sm_cg_result *res /* R*2*nsrc, nullable */);
int sm_ens_hmc_trajectory(sm_ens *e, const sm_hmc_params *p /* R */, uint64_t traj, sm_hmc_result *out /* R */);
/* sm_hmc_run per replica (the reference's statistics and acceptance
 * definition; out[r].cg_link_bytes = 32). The series are R rows of Nmeas.
 * save_prefix (nullable): after measurement i replica r's field goes to
 * <save_prefix>_r<r>_<i>.ctxt in the 28-byte record format. */
int sm_ens_hmc_run(sm_ens *e, const sm_hmc_params *p /* R */, int hot_start, uint64_t first_traj, int Ntherm,
                   int Nmeas, int Nsteps, const char *save_prefix, sm_hmc_summary *out /* R */,
                   double *sp_series /* R*Nmeas, nullable */, double *gs_series /* R*Nmeas, nullable */);

/* ==== topological charge and Wilson flow ======================================
 * Gauge observables beyond the plaquette, for a context's field and for every
 * replica of an ensemble (schwingermodel_amd/csrc/sm_flow.cpp, sm_flow.hip).
 * Not in the reference, which measures the plaquette only; conventions are
 * those of sm_plaquette (plane 0 = U_t, plane 1 = U_x, U_01 the same
 * expression in the same order). One pass over the field gives
 *   action = sum_n (1 - Re U_01(n))          (beta = 1; the caller scales it)
 *   q_geo  = (1/2 pi) sum_n atan2(Im U_01(n), Re U_01(n))
 *   q_sin  = (1/2 pi) sum_n Im U_01(n)
 * q_geo is the geometric charge, an integer up to rounding on any field;
 * q_sin the field-theoretic one, which approaches q_geo under flow. The sums
 * run in sm_plaquette's grid and order without atomics: repeated calls agree
 * bitwise, and action is bitwise sm_plaquette's gauge_action at beta = 1.
 * The flow integrates d theta_mu(n) / dt = -d/d theta_mu(n) sum (1 - Re U_01),
 * whose right-hand side Z_mu(n) = -Im(U_mu(n) conj(S_mu(n))) is sm_gauge_force
 * at beta = 1 (S: sm_staples), by Luescher's third-order scheme in its
 * one-accumulator form; one step of size eps, A one double per link:
 *   A = eps Z(W);                        W <- W exp(i A / 4)
 *   A = (8/9) eps Z(W) - (17/36) A;      W <- W exp(i A)
 *   A = (3/4) eps Z(W) - A;              W <- W exp(i A)
 * with exp(i y) = (cos y, sin y) and the plain complex product, as the
 * leapfrog's link update. Each stage is ONE fused launch (both staple forces,
 * the accumulator, both rotated links, written to the other of two field
 * buffers; 80-96 B of traffic per site), for all replicas of an ensemble.
 * series[k], k = 0 .. sm_flow_points(p) - 1: the three sums after
 * k * meas_every steps, at flow time t = k * meas_every * eps; point 0 is the
 * unflowed field, and nsteps = 0 is one point and no stage (bitwise
 * sm_topology). Every stage and measurement of a flow is enqueued at once; the
 * sums collect on the device and one copy brings them back: about 3 nsteps
 * launches plus two per point, no host round trip in between.
 * A flow is a measurement: the context's gauge field, the ensemble's fields
 * and every solver workspace are bitwise what they were before the call, and
 * a trajectory or a solve after a flow is bitwise the one without it. The
 * context flows in two field buffers and an accumulator of its own, allocated
 * at its first flow with nsteps > 0 and freed by sm_destroy: 80 B per site (2 x
 * 32 + 16), plus 24 B per measured point. The ensemble flows in its kept-field
 * backup, chi and momenta, free between trajectories: its new memory is 24 B
 * per replica and point.
 * Replica r's values, series and flowed field are bitwise those of a lone
 * one-shard context holding the same field: the same at R = 1, at any position
 * and next to any neighbours.
 * sm_topology works on every context sm_plaquette works on (t-sharded,
 * host-staged, loopback, peer; the same ghost links and global sums; every
 * shard receives the global values). The two flow calls are for one-shard
 * contexts: SM_ERR_ARG naming the restriction on sharded, host-staged,
 * loopback and peer contexts (not in this version: the stages would need a
 * ghost exchange of a field that is not the context's U). SM_ERR_ARG also for
 * null pointers (U0_out / U1_out: both or neither), eps <= 0 or not finite,
 * nsteps < 0, meas_every < 1; SM_ERR_STATE before a gauge upload or while some
 * replica has no field; SM_ERR_HIP naming the bytes asked for when an
 * allocation fails, after which the context or ensemble stays usable. Always
 * fp64. All four calls are synchronous.
 * Not in this version: flow on t-shards, a charge column in sm_hmc_run /
 * sm_ens_hmc_run, mixed precision, other smearings. */
typedef struct { double action, q_geo, q_sin; } sm_topo;
typedef struct { double eps; int nsteps; int meas_every; } sm_flow_params;
int sm_flow_points(const sm_flow_params *p);   /* 1 + nsteps / meas_every; < 0 for bad params */
int sm_topology(sm_ctx *ctx, sm_topo *out);
int sm_wilson_flow(sm_ctx *ctx, const sm_flow_params *p, sm_topo *series /* points */,
                   double *U0_out, double *U1_out /* nullable: the flowed field, host */);
int sm_ens_topology(sm_ens *e, sm_topo *out /* R */);
int sm_ens_wilson_flow(sm_ens *e, const sm_flow_params *p, sm_topo *series /* R * points, replica-major */,
                       double *U_out /* nullable, host: R x (plane 0, plane 1) of V complex */);

/* ==== stochastic quark loops: chiral condensate and eta correlator ==========
 * Traces of D^-1 per time slice, estimated with noise vectors, for a context's
 * field and for every replica of an ensemble
 * (schwingermodel_amd/csrc/sm_loops.cpp, sm_loops.hip). Not in the reference.
 * Noise vector k of `seed` is complex Z2 x Z2 noise, eta_k,a(n) = (+-1 +- i) /
 * sqrt(2), drawn on the device and bitwise what sm_fill_noise(seed, k, ...)
 * writes on the host. With psi_k = D^-1 eta_k and gamma5 = diag(1, -1) (the
 * convention behind the pion's gamma5-hermiticity), per vector and time slice
 *   S_k(t) = sum_x sum_a conj(eta_k,a(x,t)) psi_k,a(x,t)   -> E_k S_k(t) = Tr_t D^-1
 *   P_k(t) = sum_x (conj(eta_k,0) psi_k,0 - conj(eta_k,1) psi_k,1)(x,t)
 *                                                  -> E_k P_k(t) = Tr_t gamma5 D^-1
 * so that the chiral condensate is (Nf / V) Re sum_t mean_k S_k(t), and the
 * disconnected piece of the flavour-singlet pseudoscalar comes from products
 * P_k(t) P_k'(t + dt) of different vectors (schwingermodel_amd/loops.py has
 * the estimators). t is the absolute time coordinate.
 * Layout: loops[((k*Nt) + t)*4 + c], c = Re S, Im S, Re P, Im P, on the host;
 * res[k] (nullable) reports vector k's solve. The ensemble:
 * loops[(((r*nnoise) + k)*Nt + t)*4 + c], res[r*nnoise + k] (nullable), replica
 * r with mass m0[r] and seed seed[r].
 * solver 0: y = (D D^dag)^-1 eta by the batched CG (sm_cg_batch's solver: one
 * launch per iteration for all columns), then ONE fused launch that forms psi =
 * D^dag y at each site in registers, regenerates eta from its counter and adds
 * up the slices: it reads y and the links (32 + 32 B per site and column, the
 * links from cache after a shared field's first column) and stores neither psi
 * nor eta. The context solves its nnoise vectors in chunks of at most
 * sm_cg_batch_max() columns (nnoise itself is not capped) and follows
 * sm_cg_batch_precision exactly as sm_pion_correlator does; the ensemble makes
 * one batched solve of R columns per vector, column r on replica r's links and
 * mass, and one contraction launch for all replicas, always fp64.
 * solver 1: the even-odd system of sm_pion_solver = 1 on the noise (phihat_e,
 * the batched even-odd solve, S_e, S_o, back to the full layout: the same code
 * the pion correlator runs), then the contraction on the stored psi. Always
 * fp64; res reports the even-odd solves. Needs even Nx and Nt: SM_ERR_ARG
 * naming the checkerboard otherwise, and solver 0 keeps working.
 * Vector k's loops and res[k] depend on the field, m0, tol, max_iter, seed and
 * k only: not on nnoise or the chunking, and they are bitwise the same on
 * every call (fixed summation order, no atomics). Replica r's loops and res
 * are bitwise sm_quark_loops' on a lone context holding that field with m0[r]
 * and seed[r], with either solver: the same at R = 1, at any position and next
 * to any neighbours.
 * These are measurements: the context's gauge field, the ensemble's fields and
 * the HMC state are not written; a trajectory, sm_cg_batch or
 * sm_pion_correlator after a call is bitwise the one without it.
 * Memory. The context works in sm_cg_batch's workspace and staging (solver 1:
 * sm_pion_solver = 1's), for min(nnoise, sm_cg_batch_max()) columns; the
 * ensemble in its chi, phi, x and solver workspaces (solver 1: its even-odd
 * fields), free between trajectories. New memory: 32 B per vector and time
 * slice on the device (per replica for the ensemble) and 1 KiB of seeds.
 * SM_ERR_ARG for a null context, ensemble, loops (ensemble: m0, seed),
 * nnoise < 1, solver not 0 or 1, max_iter < 0 and on sharded, host-staged,
 * loopback and peer contexts; SM_ERR_STATE before a gauge upload or while some
 * replica has no field; SM_ERR_HIP naming the bytes asked for when an
 * allocation fails, after which the context or ensemble stays usable. Both
 * calls are synchronous.
 * Not in this version: dilution, t-shards, a loops column in sm_hmc_run /
 * sm_ens_hmc_run. */
int sm_quark_loops(sm_ctx *ctx, double m0, double tol, int max_iter, int solver, int nnoise, uint64_t seed,
                   double *loops /* nnoise*Nt*4, host */, sm_cg_result *res /* nnoise, nullable */);
int sm_ens_quark_loops(sm_ens *e, const double *m0 /* R */, double tol, int max_iter, int solver, int nnoise,
                       const uint64_t *seed /* R */, double *loops /* R*nnoise*Nt*4, host */,
                       sm_cg_result *res /* R*nnoise, nullable */);

/* Gather the sharded gauge field to shard 0 (SaveConf's MPI_Gatherv,
 * src/gauge_conf.cpp:378-396): U0/U1 on shard 0 receive the global
 * Nx x Nt field (n = x*Nt + t); other shards may pass NULL. RCCL transport
 * or one shard only. */
int sm_gather_gauge(sm_ctx *ctx, double *U0, double *U1);

#ifdef __cplusplus
}
#endif
#endif
