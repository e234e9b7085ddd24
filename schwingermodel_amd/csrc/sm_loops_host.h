// sm_loops_host.h -- the quark loops' host-side index arithmetic (sm_loops.cpp),
// free of any device call so that tools/loops_host_check.cpp can run it under
// the host sanitizers: where vector k of replica r lies in the caller's arrays,
// how nnoise columns are cut into batches, and the argument checks of
// sm_quark_loops / sm_ens_quark_loops in the order they are made.
#pragma once
#include <stddef.h>

namespace sm_loops_host {

// loops[(((r * nnoise) + k) * Nt + t) * 4 + c], res[r * nnoise + k]; a lone context is r = 0
inline size_t loops_index(int nnoise, int Nt, int r, int k, int t, int c) {
    return ((((size_t)r * (size_t)nnoise) + (size_t)k) * (size_t)Nt + (size_t)t) * 4 + (size_t)c;
}
inline size_t res_index(int nnoise, int r, int k) { return (size_t)r * (size_t)nnoise + (size_t)k; }
inline size_t loops_doubles(int R, int nnoise, int Nt) { return (size_t)R * (size_t)nnoise * (size_t)Nt * 4; }

// The lone context solves vectors [k0, k0 + K) of chunk i together, K <= batch_max
inline int chunk_count(int nnoise, int batch_max) { return (nnoise + batch_max - 1) / batch_max; }
inline int chunk_first(int batch_max, int i) { return i * batch_max; }
inline int chunk_size(int nnoise, int batch_max, int i) {
    const int left = nnoise - i * batch_max;
    return left < batch_max ? left : batch_max;
}

enum Refusal {
    LOOPS_OK = 0,
    LOOPS_NULL,          // loops (ensemble: also m0 or seed) is null
    LOOPS_SOLVER,        // solver not 0 or 1
    LOOPS_NNOISE,        // nnoise < 1
    LOOPS_MAX_ITER,      // max_iter < 0
    LOOPS_CHECKERBOARD,  // solver 1 on odd Nx or Nt
};

// m0 / seed: the ensemble's arrays (a lone context passes any non-null pointer)
inline Refusal args_refusal(const void *m0, const void *seed, const void *loops, int solver, int nnoise, int max_iter,
                            int Nx, int Nt) {
    if (!m0 || !seed || !loops) return LOOPS_NULL;
    if (solver != 0 && solver != 1) return LOOPS_SOLVER;
    if (nnoise < 1) return LOOPS_NNOISE;
    if (max_iter < 0) return LOOPS_MAX_ITER;
    if (solver == 1 && (Nx % 2 || Nt % 2)) return LOOPS_CHECKERBOARD;
    return LOOPS_OK;
}

}  // namespace sm_loops_host
