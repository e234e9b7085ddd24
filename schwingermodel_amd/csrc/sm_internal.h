// sm_internal.h -- private interface between the C-ABI host layer (sm_capi.cpp)
// and the gfx950 kernels (sm_kernels.hip). Not installed; include/sm_hip.h is
// the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sm_cg_host.h"

namespace sm {

// Device field layout: the reference's SoA spinor, i.e.
// two planes of complex<double> (double2), plane stride V = Nx*Wt sites,
// site n = x*Wt + t (t fastest). U: plane 0 = U_t (mu=0), plane 1 = U_x.
// A face is one t-column for all x, stored [plane][x] (plane stride Nx).

// Neighbour sources of a t-domain. For one GPU (nshard == 1) the "faces" are
// aliases into the field itself (periodic wrap, xs = Wt); for a t-shard they
// are the received halo buffers (xs = 1).
struct TFaces {
    const double2 *lo;   // psi at local t = -1   : lo[x*lo_xs] (+ lo_ps for plane 1)
    const double2 *hi;   // psi at local t = Wt   : hi[x*hi_xs] (+ hi_ps for plane 1)
    long lo_xs, lo_ps, hi_xs, hi_ps;
    // proj = 1: spin-projected t-faces (t-shards), ONE complex per x and side:
    // hi = the forward hop's spin combination at t = Wt (D: p0 - p1, D^dag:
    // p0 + p1; force: l0 + l1 / r0 - r1), lo = the backward hop's whole product
    // conj(U_t(t = -1)) * combination (D: p0 + p1, D^dag: p0 - p1), formed by
    // the sending shard with its own link (launch_pack_faces_proj).
    int proj = 0;
};
enum FaceKind { FACE_D = 0, FACE_DDAG = 1, FACE_FORCE_L = 2, FACE_FORCE_R = 3 };

struct PeerView;  // sm_peer.h

struct Geometry {
    int Nx, Wt;          // local block (all x, Wt t-values)
    int t0, Ntg;         // global t offset of this shard, global Nt
    long V;              // Nx*Wt
};

// One-pass CG scalar state after evaluating one pass's partials (the
// redundant-scalar path of small grids keeps it per pass parity, sm_cgfused.hip).
struct CGRed {
    double2 rn, alpha, beta;
    double2 alpha2, beta2;   // alpha, beta of the pass before (two-direction CG)
    double err;
    int k, done, converged, pad;
};

// Scalars of one CG solve, resident on the device (no host round trip per
// iteration). Mirrors the locals of conjugate_gradient(),
// src/conjugate_gradient.cpp:6-14.
struct CGScalars {
    double2 rn;          // r_norm2 (complex, as the reference keeps it)
    double2 alpha, beta;
    double2 alpha2, beta2;  // two-direction CG: alpha_{j-1}, beta_{j-1} while alpha, beta are alpha_j, beta_j
    double2 sum;         // last globally reduced dot
    double phi_norm;     // sqrt(Re <phi,phi>)
    double tol;
    double err;          // sqrt(Re <r,r>) of the last iteration
    int k;               // iterations executed
    int done;            // 1 once converged: every later CG kernel is a no-op
    int converged;
    int max_iter;        // one-pass path: the device stops itself at k == max_iter
    double2 sum3[3];     // one-pass path, multi-shard: all-reduced <d,Ad>, <r,Ad>, (|r|^2,|Ad|^2)
    CGRed red[2];        // one-pass path, redundant scalars: state S_i in red[i & 1]; red[1] = S_-1
    double2 sumr[2][3];  // recompute-Ad pass on t-shards, redundant scalars: pass i's all-reduced sums in sumr[i & 1]
};

enum Epilogue { EPI_NONE = 0, EPI_DOT = 1 };

// ---- launchers (sm_kernels.hip) -------------------------------------------
struct LaunchCfg {
    int bt;              // threads per block along t (64/128/256)
    int xchunk;          // rows marched per block
    int xcd_remap;       // 1: consecutive tiles of one XCD are x-adjacent (L2 reuse of halo rows)
    int variant;         // dslash code variant (sm_kernels.hip)
};
constexpr int kMaxPartials = 1 << 16;
LaunchCfg dslash_config(const Geometry &g);

// out = D in (dagger=0) or D^dagger in (dagger=1). EPI_DOT additionally
// writes per-block partials of sum aux * conj(out) to `partials`.
void launch_dslash(hipStream_t s, const Geometry &g, const LaunchCfg &c, int dagger,
                   const double2 *in, double2 *out, const double2 *U, const double2 *loU,
                   const TFaces &f, double mass, const double2 *aux, double2 *partials,
                   const CGScalars *skip_if_done, int tb0 = 0, int tbn = -1);
int dslash_blocks(const Geometry &g, const LaunchCfg &c);

void launch_force(hipStream_t s, const Geometry &g, const double2 *U, const double2 *l,
                  const double2 *r, const TFaces &fl, const TFaces &fr, double *F);

int reduce_blocks(long n);   // grid size used by the BLAS-1 reductions of n complex
void launch_dot_partial(hipStream_t s, long n, const double2 *a, const double2 *b, double2 *partials);
void launch_sum_partials(hipStream_t s, int nparts, const double2 *partials, double2 *out);

void launch_copy(hipStream_t s, long n, const double2 *src, double2 *dst);
void launch_cg_init(hipStream_t s, long n, const double2 *phi, const double2 *Ax, double2 *r,
                    double2 *d, double2 *part_rr, double2 *part_pp);
void launch_cg_finalize_init(hipStream_t s, int nparts, const double2 *part_rr,
                             const double2 *part_pp, CGScalars *sc, double tol);
void launch_cg_alpha(hipStream_t s, int nparts, const double2 *part, CGScalars *sc);
void launch_cg_update_xr(hipStream_t s, long n, double2 *x, double2 *r, const double2 *d,
                         const double2 *Ad, CGScalars *sc, double2 *part);
void launch_cg_beta(hipStream_t s, int nparts, const double2 *part, CGScalars *sc);
void launch_cg_update_d(hipStream_t s, long n, double2 *d, const double2 *r, const CGScalars *sc);

// Multi-GPU helpers: partial -> local sum (into sc->sum) and global-sum
// consumers that take the already all-reduced value.
void launch_sum_to_scalar(hipStream_t s, int nparts, const double2 *part, CGScalars *sc);
void launch_cg_alpha_from_sum(hipStream_t s, CGScalars *sc);
void launch_cg_beta_from_sum(hipStream_t s, CGScalars *sc);
void launch_cg_init_from_sums(hipStream_t s, const double2 *rr_pp, CGScalars *sc, double tol);

// ---- fused CG iteration (sm_cgfused.hip) ----
constexpr int kFusedWaveCols = 60;  // output t-columns per wave (64 lanes - 2x2 halo)
struct CGFusedCfg {
    int NWT, TBk;        // wave tiles along t (60 columns each; 56 for sm_cgra.hip), blocks along t (4 waves)
    int xchunk, XB;      // rows per block, blocks along x
    int remap;
    int fold = 0;        // sm_cgra.hip: folded hopping-bracket arithmetic (dirac_bracket_folded)
    int wpb = 4;         // sm_cgra.hip: waves per block (1, 2, 4)
    int rev_odd = 0;     // sm_cgra.hip: odd one-shard tail passes march backwards over reversed tiles
    int strip = 0;       // sm_cgra.hip: the block's 4 waves share one t-strip (one shard; TBk = strips)
    int xbal = 0;        // sm_cgra.hip: XB balanced chunks of Nx / XB rows instead of xchunk-row chunks
};
CGFusedCfg cg_fused_config(const Geometry &g);
int cg_fused_blocks(const CGFusedCfg &c);
// The two-direction one-pass iteration with a stored Ad (mode 4): partials are
// 3 per block; d_{j-1} in dold, d_{j-2} in rold (faces fd / fr), Ad_{j-1} in aold.
void launch_cg_onepass(hipStream_t s, const Geometry &g, const CGFusedCfg &c, int nshard,
                       const double2 *dold, const double2 *rold, const double2 *aold, double2 *dnew,
                       double2 *anew, double2 *x, const double2 *U, const double2 *fd, const double2 *fr,
                       const double2 *fa, const double2 *fU, double mass, int first, CGScalars *sc,
                       double2 *partials, int tb0, int tbn,
                       const double2 *prev_partials = nullptr,  // != null: redundant scalars (see below)
                       long pass = 0);
// Two-direction pass that recomputes Ad_{j-1} = D D^dag d_{j-1} in-kernel
// instead of storing Ad (sm_cgra.hip): 160 B/site; d_i in d[i % 3] as below.
// Faces (t-shard, 4-deep [col -4..-1, Wt..Wt+3][plane][x]): f1 = d_{j-1},
// f2 = d_{j-2} (the previous pass's f1), fU = U.
constexpr int kRAWaveCols = 56;  // output t-columns per wave (64 lanes - 2x4 halo)
CGFusedCfg cg_ra_config(const Geometry &g);
// t-strip blocks on (strip = 1: 4 waves, 248 owned columns per block) or off;
// sets wpb / TBk accordingly and returns TBk
int cg_ra_set_strip(CGFusedCfg &c, const Geometry &g, int strip);
// Returns the link bytes per site the launched pass reads: 32 (complex links),
// 20 (codes, 16-bit flag words) or 17 (codes, packed flag bytes); 0 if nothing launched.
int launch_cg_ra(hipStream_t s, const Geometry &g, const CGFusedCfg &c, int nshard, const double2 *d1,
                 const double2 *d2, double2 *dn, double2 *x, const double2 *U, const double2 *f1,
                 const double2 *f2, const double2 *fU, double mass, long pass, CGScalars *sc, double2 *partials,
                 int tb0, int tbn, const double2 *prev_partials = nullptr, const double *Uang = nullptr,
                 const double *fUang = nullptr, double2 *fsend = nullptr, int pbase = 0,
                 unsigned *tick = nullptr, int ntiles = 0, double2 *gsum = nullptr, double2 *out3 = nullptr,
                 int red_sums = 0, int link_fmt = 1, double2 *fsendh = nullptr, const PeerView *peer = nullptr,
                 unsigned long long pseq = 0, int pstore = 0, int sched = 0, hipEvent_t stop = nullptr);
// Resident blocks per CU of the t-shard pass kernel at c's block size (0 if
// the runtime cannot tell); link_fmt 0 = complex links, 1 / 2 = the code forms.
int cg_ra_shard_blocks_per_cu(const CGFusedCfg &c, int link_fmt);
// (tick != null: ticketed tail over the ntiles tiles of every launch of the
// pass -- the last block forms the scalars in sc, or writes the shard's three
// sums to out3; tick holds 1 + ceil(ntiles / 64) zeroed counters, gsum 3 per group)
constexpr int kMaxTickGroups = 1024;
// (partial slot of a tile: pbase + (t-block - tb0) * XB + x-chunk; fsend (t-shards):
// the blocks owning columns 0..3 / Wt-4..Wt-1 also write d_j's 4-deep send
// faces, lo at fsend and hi at fsendh (default fsend + 8 Nx), as
// launch_pack_faces_k would; peer (device copy of the peer view): those faces
// go out as write-through system-scope stores (fsend / fsendh then point into
// the neighbours' regions) and the tail all-reduces the shard's sums itself,
// collective number pseq, into out3)
// Link codes of U for the passes above (Uang: 20 instead of 32 B/site of
// links, sm_linkcode.h): writes the codes v of n links to Ua[0, n) and their
// flag words to the n uint16 right after them, and per block the count of
// links the pass's decoder does NOT rebuild bitwise to partials; returns the
// block count.
int launch_link_codes(hipStream_t s, long n, const double2 *U, double *Ua, double2 *partials);
// Packed link flags (launch_cg_ra link_fmt 2): one byte per site holding the
// U_t and U_x flag nibbles, written after the flag words of the V-site code
// block / of the 4-deep face block (sm_linkcode.h sm_lc_nibble; only for
// fields whose every flag word fits a nibble)
void launch_link_nibbles(hipStream_t s, long V, const double *Ua);
void launch_face_nibbles(hipStream_t s, int Nx, const double *fUa);
// Diagnostic: encode + decode each of n links (the pass's functions) into
// out (may be null); per block (count not rebuilt bitwise, largest
// per-component error) to partials; returns the block count.
int launch_link_code_check(hipStream_t s, long n, const double2 *U, double2 *out, double2 *partials);
// Recompute-Ad CG: after the last pass add alpha_{k-1} d_{k-1} to the rows
// whose x update is still pending (parity != k & 1; x row = site / Wt).
void launch_cg_ra_finish_x(hipStream_t s, const Geometry &g, double2 *x, const double2 *d0, const double2 *d1,
                           const double2 *d2, const CGScalars *sc);
// prev_partials != null (one shard, fold 2): redundant scalars as in
// cg_onepass_kernel: every block evaluates pass j-1's scalars from its partials
// (cg1_redundant); the caller keeps the partials by pass parity and flushes.
// Pack the k-deep t-faces of a field: lo = columns 0..k-1, hi = columns Wt-k..Wt-1, [col][plane][x].
void launch_pack_faces_k(hipStream_t s, const Geometry &g, int k, const double2 *field, double2 *lo, double2 *hi);
// Two-direction form, after the last pass J = sc->k: if J is odd, x += alpha_{J-1} d_{J-1}
// (d_i lives in d[i % 3]).
void launch_cg_td_finish_x(hipStream_t s, long n, double2 *x, const double2 *d0, const double2 *d1,
                           const double2 *d2, const CGScalars *sc);
// Redundant scalars (small one-shard grids): pass j writes its partials (by
// pass parity) and every block of pass j + 1 evaluates them itself (fixed
// order, bitwise the same in every block) -- no ticket, no scalar launch.
// launch_cg1_flush evaluates the last issued pass's partials into sc for the
// host (idempotent: the next pass recomputes the same state).
void launch_cg1_flush(hipStream_t s, int nparts, const double2 *partials, CGScalars *sc, long pass);
// stored-Ad pass: redundant scalars up to this grid size (64^2: 64 blocks, 11.2 vs 12.0 us per
// iteration with a scalar ticket; 128^2 11.6 vs 12.9 us)
constexpr int kRedundantMaxBlocks = 128;
void launch_cg1_scalars(hipStream_t s, int nparts, const double2 *partials, CGScalars *sc, int first);
void launch_cg1_local_sum(hipStream_t s, int nparts, const double2 *partials, CGScalars *sc);
// t-shard redundant scalars (sm_cgra.hip): S_J of the last issued pass J from its all-reduced sums
void launch_cg_ra_flush_sums(hipStream_t s, CGScalars *sc, long pass);
void launch_cg1_from_sums(hipStream_t s, CGScalars *sc, int first);
void launch_pack_faces2(hipStream_t s, const Geometry &g, const double2 *field, double2 *lo,
                        double2 *hi);

void launch_stream(hipStream_t s, int two, long n, const double2 *a, const double2 *b, double2 *out,
                   int blocks);

// ---- mixed-precision CG (sm_cgsp.hip; driver sm_cgmp.cpp) ----
// MPScalars, the device-resident scalars of a mixed solve: sm_cg_host.h
// The fp32 pass's tiles: the recompute-Ad pass's shape (ra) without its t-strips.
CGFusedCfg cg_sp_config(const Geometry &g, const CGFusedCfg &ra);
// Pass `pass` of a segment (0: the injected direction, no store): d_{j-1} in
// d1, d_{j-2} in d2, d_j to dn; 2 partials per tile for launch_cg_sp_scalars.
void launch_cg_sp(hipStream_t s, const Geometry &g, const CGFusedCfg &c, const float2 *d1, const float2 *d2, float2 *dn,
                  float2 *y, const float2 *U32, double mass, long pass, MPScalars *sc, double2 *partials);
void launch_cg_sp_scalars(hipStream_t s, int ntiles, const double2 *partials, MPScalars *sc, int first);
// U32 = the links as the fp32 pass reads them (pre-scaled, sm_cgsp.hip)
void launch_sp_convert_links(hipStream_t s, const Geometry &g, const double2 *U, float2 *U32);
// r = phi - Ax with per-block (|r|^2, |phi|^2); returns the block count
int launch_mp_residual(hipStream_t s, long n, const double2 *phi, const double2 *Ax, double2 *r, double2 *partials);
// those partials into sc: the true residual, the stop test, the next segment's M and injection beta
void launch_mp_update(hipStream_t s, int nparts, const double2 *partials, MPScalars *sc, int init, int restart,
                      double tol, double delta, int max_iter);
// d0 = r + sc->beta dprev in fp32 (sc->beta == 0: dprev = d0 = r)
void launch_mp_inject(hipStream_t s, long n, const double2 *r, float2 *dprev, float2 *d0, const MPScalars *sc);
// x += y plus the pending alpha_{J-1} d_{J-1} rows (dlast = d_{J-1}), y = 0; discard: y = 0 only
void launch_mp_fold(hipStream_t s, const Geometry &g, double2 *x, float2 *y, const float2 *dlast, const MPScalars *sc,
                    int discard);
void launch_mp_add(hipStream_t s, long n, double2 *x, const double2 *e);
void launch_mp_zero(hipStream_t s, long n, float2 *y);

// ---- batched multi-source CG and the pion correlator (sm_cgbatch.hip; driver sm_cgbatch.cpp) ----
// K columns, 2V complex apart, on one gauge field; one shard. A tile is one
// wave: 60 owned t-columns x xchunk rows. Partials are kept per granule of G
// rows (G from the lattice alone), so a column's sums do not depend on K.
constexpr int kBatchMax = 64;            // sm_cg_batch_max()
constexpr int kBatchRedMaxSlots = 512;   // redundant scalars up to this many partial slots per column
// tiles per launch the tile height aims at: one resident round (256 CUs x 4 SIMDs x 2 waves at the
// pass's 210-220 VGPRs); measured best of 1024..16384 at 64^2 and 256^2
constexpr int kBatchTargetTiles = 2048;
// Tiles, partial slots and scalar scheme of a batched solver, this one, the
// even-odd one (below) and the mixed one's passes alike.
struct BatchCfg {
    int NWT;        // wave tiles along t (even-odd: along k)
    int G, NG;      // rows per granule, granules per column of tiles
    int P;          // partial slots per column (NWT * NG), 3 complex each
    int red;        // 1: redundant scalars (every tile sums its column's previous partials; P <= kBatchRedMaxSlots)
    int xchunk;     // rows per tile (a multiple of G)
    int NCH;        // tiles along x
    int NB0;        // blocks per column of the start kernel
    long pstride;   // complex per column in the partials buffer
};
// A solver's tiles of `width` owned columns on `extent` columns per row, granules of small_G
// rows below Nx = 512 (8 from there), aiming at target_tiles tiles per launch
BatchCfg batch_config(const Geometry &g, int K, int width, int extent, int small_G, int target_tiles);
BatchCfg cg_batch_config(const Geometry &g, int K, int target_tiles = 0);
// The scalar machinery of the fp64 batched solvers (one copy, sm_cgbatch.hip's
// header has the scheme): the scalar step of pass `pass` without redundant
// scalars; with them the last issued pass's state into sc for the host (else
// nothing: the scalar kernel has evaluated it); the columns' scalars at the
// start (tol, max_iter, S_-1) from the start kernel's partials; and, after the
// last pass, x_b += alpha_{k-1} d_{k-1} on the columns of n complex whose
// iteration count is odd.
void launch_batch_scalars(hipStream_t s, const BatchCfg &c, int K, const double2 *partials, CGScalars *sc, long pass);
void launch_batch_flush(hipStream_t s, const BatchCfg &c, int K, const double2 *partials, CGScalars *sc, long pass);
void launch_batch_init_scalars(hipStream_t s, const BatchCfg &c, int K, const double2 *partials, CGScalars *sc,
                               double tol, int max_iter);
void launch_batch_finish_x(hipStream_t s, int K, long n, double2 *x, const double2 *d0, const double2 *d1,
                           const double2 *d2, const CGScalars *sc);
// The links and mass of each column: column b reads the field at U + b * ustride
// (complex) and uses massv[b]. One field for all columns (sm_cg_batch, the
// pion correlator): ustride = 0, massv = null and every column uses `mass`.
// Both are block-uniform in every batched kernel (scalar registers).
struct BatchLinks {
    const double2 *U;
    long ustride;
    double mass;
    const double *massv;  // device, K masses (m0 + 2), or null
};
inline BatchLinks shared_links(const double2 *U, double mass) { return BatchLinks{U, 0, mass, nullptr}; }
// out_b = D in_b (dagger = 0) or D^dag in_b (1), one thread per site, K columns in one launch
void launch_batch_apply(hipStream_t s, const Geometry &g, int K, int dagger, const double2 *in, double2 *out,
                        const BatchLinks &l);
// x = phi, T = D^dag phi, d0 = r_0 = phi - D T, and the columns' scalars (tol, max_iter, S_-1)
void launch_cg_batch_init(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *phi, double2 *x,
                          double2 *T, double2 *d0, const BatchLinks &l, double tol, int max_iter, double2 *partials,
                          CGScalars *sc);
// pass j of every column that is not done (and, without redundant scalars, its scalar step)
void launch_cg_batch_pass(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *dold,
                          const double2 *rold, const double2 *aold, double2 *dnew, double2 *anew, double2 *x,
                          const BatchLinks &l, long pass, CGScalars *sc, double2 *partials);
// ---- mixed-precision batched CG (sm_cgbatchsp.hip; driver sm_cgbatchmp.cpp) ----
// Every launch serves the columns of `mask` (bit b = column b, K <= 64) and
// leaves the others alone. The direction ring d[3] holds d_i of the running
// round in d[i mod 3] for every column (d_{-1} in d[2]); ad[2]: Ad by pass parity.
static_assert(kBatchMax <= 64, "the batched mixed-precision kernels name their columns in a 64-bit mask");
// Pass `pass` of a round (0: the injected direction, no d store; even passes
// >= 2 update y) and its scalar step, c's tiles; partials: K x 2 c.P complex.
void launch_cg_batch_sp(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, unsigned long long mask,
                        float2 *const d[3], float2 *const ad[2], float2 *y, const float2 *U32, double mass, long pass,
                        MPScalars *sc, double2 *partials);
int batch_mp_blocks(const Geometry &g);  // blocks per column of the three kernels below (the lattice's alone)
// r_b = phi_b - Ax_b and launch_mp_update's step on column b's scalars; partials: K x batch_mp_blocks(g)
void launch_batch_mp_residual(hipStream_t s, const Geometry &g, int K, unsigned long long mask, const double2 *phi,
                              const double2 *Ax, double2 *r, double2 *partials, MPScalars *sc, int init, int restart,
                              double tol, double delta, int max_iter);
// d[0] = fp32(r) + beta_b d_prev, d[2] = d_prev = the ended segment's last direction, wherever the ring holds it
void launch_batch_mp_inject(hipStream_t s, const Geometry &g, int K, unsigned long long mask, const double2 *r,
                            float2 *const d[3], const MPScalars *sc);
// x_b += y_b plus the pending alpha_{J-1} d_{J-1} after an odd J_b, y_b = 0; columns of `discard`: y_b = 0 only
void launch_batch_mp_fold(hipStream_t s, const Geometry &g, int K, unsigned long long mask, unsigned long long discard,
                          double2 *x, float2 *y, float2 *const d[3], const MPScalars *sc);

void launch_point_sources(hipStream_t s, const Geometry &g, int K, const int *sx, const int *st, double2 *phi);
void launch_pion_slices(hipStream_t s, const Geometry &g, int nsrc, const double2 *S, double *C);

// ---- gauge field / molecular dynamics (sm_gauge.hip) ----
// fU: the 2-deep U faces (nshard > 1; ignored for one shard, which wraps).
int gauge_reduce_blocks(const Geometry &g);
void launch_plaquette(hipStream_t s, const Geometry &g, int nshard, const double2 *U, const double2 *fU,
                      double beta, double2 *field, double2 *partials);
void launch_staple_force(hipStream_t s, const Geometry &g, int nshard, const double2 *U, const double2 *fU,
                         double beta, double *F, double2 *staples);
void launch_md_update(hipStream_t s, const Geometry &g, double2 *U, double *P, const double *F, double eps,
                      int do_p, double coef);
void launch_kinetic(hipStream_t s, const Geometry &g, const double *P, double2 *partials);
void launch_draw_momenta(hipStream_t s, const Geometry &g, uint64_t seed, double *P);
void launch_draw_source(hipStream_t s, const Geometry &g, uint64_t seed, double2 *chi);
void launch_draw_gauge(hipStream_t s, const Geometry &g, uint64_t seed, double sigma, double2 *U);

// ---- replica ensemble (sm_ens.cpp): the MD kernels above for R fields in one launch ----
// One shard. Replica r = blockIdx.y; its fields lie r * 2V elements into each
// array (complex for U, chi and spinors, doubles for P and F). Every reduction
// keeps the one-field kernel's grid (gauge_reduce_blocks(g) blocks of 256) per
// replica and writes row r of `partials` (gauge_reduce_blocks(g) apart);
// launch_ens_sums sums rows in launch_sum_partials' order, so a replica's sums
// are bitwise those of the one-field path on the same field.
struct EnsPar {
    double beta;
    double eps;      // tau / md_steps
    uint64_t seed;   // sm_traj_seed(seed, traj)
};
void launch_ens_draws(hipStream_t s, const Geometry &g, int R, const EnsPar *par, double *P, double2 *chi);
// do_p: P += eps_r F; then U *= exp(i (cfac eps_r) P), cfac = 0.5 or 1
void launch_ens_md_update(hipStream_t s, const Geometry &g, int R, double2 *U, double *P, const double *F,
                          const EnsPar *par, int do_p, double cfac);
void launch_ens_staple_force(hipStream_t s, const Geometry &g, int R, const double2 *U, const EnsPar *par, double *F);
void launch_ens_plaquette(hipStream_t s, const Geometry &g, int R, const double2 *U, const EnsPar *par,
                          double2 *partials);
void launch_ens_kinetic(hipStream_t s, const Geometry &g, int R, const double *P, double2 *partials);
void launch_ens_dot(hipStream_t s, const Geometry &g, int R, const double2 *a, const double2 *b, double2 *partials);
void launch_ens_sums(hipStream_t s, const Geometry &g, int nrows, const double2 *partials, double2 *out);
// F_r = phi_dag_partialD_phi(U_r, l_r, r_r) (sm_kernels.hip, launch_force's arithmetic)
void launch_ens_force(hipStream_t s, const Geometry &g, int R, const double2 *U, const double2 *l, const double2 *r,
                      double *F);

// ---- topological charge and Wilson flow (sm_flow.hip; host: sm_flow.cpp) ----
// The three sums of a field: blocks write two rows of gauge_reduce_blocks(g)
// partials, (sum 1 - Re U_01, sum atan2(Im U_01, Re U_01)) then (sum Im U_01, 0);
// the ensemble form writes replica r's row pair 2 r rows in. launch_topo_sums
// sums nfields row pairs into out[i * ostride + 0, 1, 2] in launch_sum_partials'
// order, so a replica's sums are bitwise the one-field path's.
void launch_topo(hipStream_t s, const Geometry &g, int nshard, const double2 *U, const double2 *fU,
                 double2 *partials);
void launch_ens_topo(hipStream_t s, const Geometry &g, int R, const double2 *U, double2 *partials);
void launch_topo_sums(hipStream_t s, const Geometry &g, int nfields, const double2 *partials, double *out,
                      long ostride);
// Stage 0, 1 or 2 of a flow step of size eps, one shard: A = ca (eps Z(Uin)) - cb A,
// Wout = Uin exp(i rot A) with (ca, cb, rot) = (1, 0, 1/4), (8/9, 17/36, 1), (3/4, 1, 1);
// stage 0 does not read A, stage 2 does not write it. Wout must not be Uin.
// A: 2V doubles per field, Uin / Wout: 2V complex.
void launch_flow_stage(hipStream_t s, const Geometry &g, int stage, double eps, const double2 *Uin, double *A,
                       double2 *Wout);
void launch_ens_flow_stage(hipStream_t s, const Geometry &g, int R, int stage, double eps, const double2 *Uin,
                           double *A, double2 *Wout);

// ---- even-odd checkerboard (sm_eo.hip) ----
void launch_to_cb(hipStream_t s, const Geometry &g, const double2 *full, double2 *e, double2 *o);
void launch_from_cb(hipStream_t s, const Geometry &g, const double2 *e, const double2 *o, double2 *full);
// Received t-faces of checkerboard fields ([side][plane][col][x], 8*Nx
// complex each; sm_eo.hip); all null on one shard (periodic wrap).
struct EoFaces {
    const double2 *v = nullptr, *ue = nullptr, *uo = nullptr;
};
void launch_pack_cb_faces(hipStream_t s, const Geometry &g, const double2 *f, double2 *out);
// out_p = a*aux_p + b*H in_q (H: the hopping bracket of D / D^dag), parity p;
// inf / uqf: faces of `in` and Uq when t-sharded (else null)
void launch_eo_hop(hipStream_t s, const Geometry &g, int dagger, int p, const double2 *in, const double2 *Up,
                   const double2 *Uq, const double2 *aux, double a, double b, double2 *out,
                   const double2 *inf = nullptr, const double2 *uqf = nullptr);
// Fused Dhat / Dhat^dag (both hops in one marching pass); aux != null adds
// per-block partials of sum aux * conj(out) (eo_fused_blocks of them).
struct EoFusedCfg {
    int NWT, TBk, xchunk, XB;
};
EoFusedCfg eo_fused_config(const Geometry &g);
int eo_fused_blocks(const EoFusedCfg &c);
void launch_eo_dhat_fused(hipStream_t s, const Geometry &g, const EoFusedCfg &c, int dagger, const double2 *v,
                          const double2 *Ue, const double2 *Uo, double mass, double2 *out, const double2 *aux,
                          double2 *partials, const EoFaces &f);

// Folded even-odd CG iteration j (sm_eo.hip, eo_dhat_fused_kernel MODE 1/2):
// which = 0: pass A (r_j, d_j, x update; W = Dhat^dag d_j; partial |r_j|^2),
// which = 1: pass B (Ad_j = Dhat W; <d_j,Ad_j>, <r_j,Ad_j>, |Ad_j|^2). The 3
// partials per block feed launch_cg1_scalars (sm_cgfused.hip).
struct EoCgPass {
    const double2 *dold, *rold;
    double2 *dnew, *rnew, *x, *W, *ad;
    const double2 *rf = nullptr, *af = nullptr, *wf = nullptr;  // t-sharded faces of rold, ad, W
    int first;
};
void launch_eo_cg_pass(hipStream_t s, const Geometry &g, const EoFusedCfg &c, int which, const EoCgPass &q,
                       const double2 *Ue, const double2 *Uo, double mass, const EoFaces &f, CGScalars *sc,
                       double2 *partials);

// One-pass even-odd CG iteration on Dhat Dhat^dag (sm_eotd.hip, one shard):
// the two-direction recurrence, four checkerboard hops in registers; 3
// partials per block ((|W|^2, 0), <r,Ad>, (|r|^2, |Ad|^2)) for cg1_scalars.
constexpr int kEoTdWaveCols = 56;
struct EoTdCfg {
    int NWT, TBk, xchunk, XB;
};
EoTdCfg eo_td_config(const Geometry &g);
int eo_td_blocks(const EoTdCfg &c);
// t-shards: 4-deep checkerboard faces ([side][plane][col][x], 16*Nx complex)
// of d_{j-1}, d_{j-2}, Ad_{j-1} and both link parities; all null on one shard.
struct EoTdFaces {
    const double2 *d1 = nullptr, *d2 = nullptr, *ad = nullptr, *ue = nullptr, *uo = nullptr;
};
void launch_eo_td(hipStream_t s, const Geometry &g, const EoTdCfg &c, const double2 *d1, const double2 *d2,
                  const double2 *aold, double2 *dn, double2 *anew, double2 *x, const double2 *Ue, const double2 *Uo,
                  double mass, long pass, CGScalars *sc, double2 *partials, const EoTdFaces &f,
                  unsigned *tick = nullptr, double2 *gsum = nullptr, double2 *out3 = nullptr,  // tick: ticketed tail
                  int red = 0);  // red: t-shard scalars from sc->sumr (out3 = this pass's sumr slot)
void launch_pack_cb_faces4(hipStream_t s, const Geometry &g, const double2 *f, double2 *out);

// ---- batched one-pass even-odd CG (sm_eobatch.hip; driver sm_eobatch.cpp) ----
// K columns on the half lattice, V complex apart (two planes of V/2); one shard.
// A tile is one wave: kEoTdWaveCols owned k-columns x xchunk rows. Partials per
// granule of G rows (G from the lattice alone, even), summed in slot order.
// tiles per launch the tile height aims at: one resident round (256 CUs x 4 SIMDs x 1 wave at the
// pass's register count)
constexpr int kEoBatchTargetTiles = 1024;
BatchCfg eo_batch_config(const Geometry &g, int K, int target_tiles = 0);  // BatchCfg, the scalar launchers: above
// The checkerboard links and mass of each column: column b reads Ue / Uo + b * ustride
// (complex) and uses massv[b]; ustride = 0 and massv = null: one field and `mass` for all.
struct EoBatchLinks {
    const double2 *Ue, *Uo;
    long ustride;
    double mass;
    const double *massv;  // device, K masses (m0 + 2), or null
};
// full layout (K x 2V complex) <-> checkerboard (K x V per parity); either parity may be null
// (from: its sites become 0). Fields and links alike.
void launch_eob_to_cb(hipStream_t s, const Geometry &g, int K, const double2 *full, double2 *e, double2 *o);
void launch_eob_from_cb(hipStream_t s, const Geometry &g, int K, const double2 *e, const double2 *o, double2 *full);
// out_p = hop of in_q on column b's links, scaled with column b's mass m: mode 0: -0.5 H in,
// 1: m aux + (0.5/m) H in, 2: (0.5/m) H in (launch_eo_hop's arithmetic)
void launch_eob_hop(hipStream_t s, const Geometry &g, int K, int dagger, int p, int mode, const double2 *in,
                    const double2 *aux, double2 *out, const EoBatchLinks &l);
// out = Dhat v (dagger = 0) or Dhat^dag v (1): two hops through the odd work field T
void launch_eob_dhat(hipStream_t s, const Geometry &g, int K, int dagger, const double2 *v, double2 *T, double2 *out,
                     const EoBatchLinks &l);
// x = phi, d0 = r_0 = phi - Dhat Dhat^dag phi (T, W, A: work), and the columns' scalars
void launch_eo_batch_init(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *phi, double2 *x,
                          double2 *T, double2 *W, double2 *A, double2 *d0, const EoBatchLinks &l, double tol,
                          int max_iter, double2 *partials, CGScalars *sc);
// pass j of every column that is not done (and, without redundant scalars, its scalar step)
void launch_eo_batch_pass(hipStream_t s, const Geometry &g, const BatchCfg &c, int K, const double2 *d1,
                          const double2 *d2, const double2 *aold, double2 *dn, double2 *anew, double2 *x,
                          const EoBatchLinks &l, long pass, CGScalars *sc, double2 *partials);

// ---- pion correlator of K columns / R replicas (sm_pion.hip; host sm_pion.cpp) ----
// Which point source each of K columns carries: sx / st (device) hold the
// sources' coordinates; per_col: column k = source k / 2, spin k % 2 (the
// context's correlator), else source s0, spin a0 in every column (one column
// per replica).
struct PionCols {
    const int *sx, *st;
    int s0, a0, per_col;
};
// The unit vectors into zeroed fields: full != null: K full-layout columns (2V
// complex apart); else K checkerboard columns (V complex apart), e or o by the site's parity.
void launch_pion_sources(hipStream_t s, const Geometry &g, int K, const PionCols &src, double2 *full, double2 *e,
                         double2 *o);
// out_b += a_b (inv_mass = 0) or out_b += a_b / m_b (1) on K half-lattice columns, m_b column b's mass of l
void launch_pion_eo_add(hipStream_t s, const Geometry &g, int K, int inv_mass, const double2 *a, double2 *out,
                        const EoBatchLinks &l);
// C[r * cstride + t] = the slice sums of replica r's spin-0 / spin-1 propagators A_r, B_r (R full-layout
// columns each), added in launch_pion_slices' order
void launch_ens_pion_slices(hipStream_t s, const Geometry &g, int R, const double2 *A, const double2 *B, double *C,
                            long cstride);

// ---- stochastic quark loops (sm_loops.hip; host sm_loops.cpp) ----
// Which noise vector each of K columns carries: column b = vector k[b] of seed[b] (device arrays).
struct LoopNoise {
    const uint64_t *seed, *k;
};
// The K noise vectors: full != null: K full-layout columns (2V complex apart); else K checkerboard
// columns (V complex apart), e or o by the site's parity. Every site is written.
void launch_loops_noise(hipStream_t s, const Geometry &g, int K, const LoopNoise &nz, double2 *full, double2 *e,
                        double2 *o);
// out[b * ostride + 4 t + c], c = Re S, Im S, Re P, Im P of column b: the slice sums of conj(eta_b) psi_b
// with eta_b regenerated from nz and psi_b = D^dag in_b on column b's links and mass of l, formed in
// registers (load_psi = 0), or psi_b = in_b read from memory (1; l is not read). One launch for all K.
void launch_loops_contract(hipStream_t s, const Geometry &g, int K, int load_psi, const double2 *in,
                           const BatchLinks &l, const LoopNoise &nz, double *out, long ostride);

// ---- mixed-precision even-odd CG (sm_eosp.hip; driver sm_eomp.cpp) ----
// Pass `pass` of a segment on float2 checkerboard fields (0: the injected
// direction, no d store; even passes >= 2 update y): d_{j-1} in d1, d_{j-2} in
// d2, Ad_{j-1} in aold (not read by pass 0), d_j to dn, Ad_j to anew; the
// eo_td_config tiles, 2 partials per block for launch_cg_sp_scalars.
void launch_eo_sp(hipStream_t s, const Geometry &g, const EoTdCfg &c, const float2 *d1, const float2 *d2,
                  const float2 *aold, float2 *dn, float2 *anew, float2 *y, const float2 *Ue32, const float2 *Uo32,
                  double mass, long pass, const MPScalars *sc, double2 *partials);
// the checkerboard links as the fp32 pass reads them (pre-scaled, signed; sm_eosp.hip)
void launch_eo_sp_convert_links(hipStream_t s, const Geometry &g, const double2 *Ue, const double2 *Uo, float2 *Ue32,
                                float2 *Uo32);
// x += y plus the pending alpha_{J-1} d_{J-1} after an odd last pass (dlast = d_{J-1}), y = 0; discard: y = 0 only
void launch_eo_mp_fold(hipStream_t s, long n, double2 *x, float2 *y, const float2 *dlast, const MPScalars *sc,
                       int discard);

// Pack the t = 0 and t = Wt-1 columns (both planes) into contiguous faces.
void launch_pack_faces(hipStream_t s, const Geometry &g, const double2 *field, double2 *lo_face,
                       double2 *hi_face);
// Spin-projected faces (TFaces::proj) of `field` for the operator `kind`:
// lo_face (my t = 0, sent down) = the forward combination, hi_face (my
// t = Wt-1, sent up) = conj(U_t) * the backward combination; Nx complex each.
void launch_pack_faces_proj(hipStream_t s, const Geometry &g, const double2 *field, const double2 *U, int kind,
                            double2 *lo_face, double2 *hi_face);

// ---- device-initiated shard transport (sm_peer.hip, layout in sm_peer.h) ----
// n (<= 3) face exchanges of cnt doubles per field and side, as exchange_faces_on:
// slo[f] goes down (arriving as the receiver's rhi[f]), shi[f] up (its rlo[f])
struct PeerXfer {
    const double *slo[3], *shi[3];
    double *rlo[3], *rhi[3];
    int n;
    long cnt;
};
// in-place sum of n <= 8 doubles over every shard, in rank order
void launch_peer_allreduce(hipStream_t s, double *dev, int n, const PeerView &v, unsigned long long seq);
// the exchange through the receivers' mailboxes (two kernels; tick: a zeroed counter)
void launch_peer_exchange(hipStream_t s, const PeerXfer &x, const PeerView &v, unsigned long long seq,
                          unsigned *tick);
// launch_pack_faces_proj's faces stored into the neighbours' apply slot seq % 4, then the handoff
void launch_peer_pack_proj(hipStream_t s, const Geometry &g, const double2 *field, const double2 *U, int kind,
                           const PeerView &v, unsigned long long seq, unsigned *tick);
void launch_peer_put(hipStream_t s, const double *src, long cnt, double *dst_remote);
void launch_peer_get(hipStream_t s, const double *src_local, long cnt, double *dst);

}  // namespace sm
