// sm_pion_host.h -- the pion correlator's host-side index arithmetic
// (sm_pion.cpp), free of any device call so that tools/pion_host_check.cpp can
// run it under the host sanitizers: where replica r's slice and solve reports
// lie in the caller's arrays, which half-lattice slot a site has, and the
// argument checks of sm_ens_pion_correlator in the order it makes them.
#pragma once
#include <stddef.h>

namespace sm_pion_host {

// C[(r * nsrc + s) * Nt + t], res[(r * nsrc + s) * 2 + a]
inline size_t c_index(int nsrc, int Nt, int r, int s, int t) {
    return ((size_t)r * (size_t)nsrc + (size_t)s) * (size_t)Nt + (size_t)t;
}
inline size_t res_index(int nsrc, int r, int s, int a) { return ((size_t)r * (size_t)nsrc + (size_t)s) * 2 + (size_t)a; }

// Site (x, t) on the checkerboard: its parity (0 even, 1 odd) and its slot in
// that parity's plane of Nx * Nt / 2 sites (eob_to_cb_kernel's map).
inline int site_parity(int x, int t) { return (x + t) & 1; }
inline size_t site_half_index(int Nt, int x, int t) { return (size_t)x * (size_t)(Nt / 2) + (size_t)(t >> 1); }

enum Refusal {
    PION_OK = 0,
    PION_NULL,          // m0, src_x, src_t or C is null
    PION_SOLVER,        // solver not 0 or 1
    PION_NSRC,          // nsrc < 1 or 2 nsrc above the batch cap
    PION_MAX_ITER,      // max_iter < 0
    PION_COORD,         // a source outside the lattice (*bad = its index)
    PION_CHECKERBOARD,  // solver 1 on odd Nx or Nt
};

inline Refusal args_refusal(const void *m0, const int *src_x, const int *src_t, const void *C, int solver, int nsrc,
                            int batch_max, int max_iter, int Nx, int Nt, int *bad) {
    if (!m0 || !src_x || !src_t || !C) return PION_NULL;
    if (solver != 0 && solver != 1) return PION_SOLVER;
    if (nsrc < 1 || 2 * (long)nsrc > batch_max) return PION_NSRC;
    if (max_iter < 0) return PION_MAX_ITER;
    for (int s = 0; s < nsrc; ++s)
        if (src_x[s] < 0 || src_x[s] >= Nx || src_t[s] < 0 || src_t[s] >= Nt) {
            if (bad) *bad = s;
            return PION_COORD;
        }
    if (solver == 1 && (Nx % 2 || Nt % 2)) return PION_CHECKERBOARD;
    return PION_OK;
}

}  // namespace sm_pion_host
