// pion_host_check.cpp -- the pion correlator's host index arithmetic and argument
// checks (csrc/sm_pion_host.h) under the host sanitizers: no device.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/pion_host_check.cpp -o build/pion_host_check && build/pion_host_check
//
// Covers: the C and res layouts tile their arrays exactly once in (r, s, t) /
// (r, s, a) order; the checkerboard slot of a site is a bijection per parity;
// and every refusal of sm_ens_pion_correlator, in the order it is made.
#include <cstdio>
#include <vector>

#include "../schwingermodel_amd/csrc/sm_pion_host.h"

using namespace sm_pion_host;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void layouts(int R, int nsrc, int Nt) {
    std::vector<int> C((size_t)R * nsrc * Nt, 0), res((size_t)R * nsrc * 2, 0);
    size_t next = 0;
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < nsrc; ++s)
            for (int t = 0; t < Nt; ++t) {
                const size_t i = c_index(nsrc, Nt, r, s, t);
                CHECK(i == next++);
                CHECK(i < C.size());
                if (i < C.size()) ++C[i];
            }
    next = 0;
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < nsrc; ++s)
            for (int a = 0; a < 2; ++a) {
                const size_t i = res_index(nsrc, r, s, a);
                CHECK(i == next++);
                CHECK(i < res.size());
                if (i < res.size()) ++res[i];
            }
    for (int v : C) CHECK(v == 1);
    for (int v : res) CHECK(v == 1);
}

static void checkerboard(int Nx, int Nt) {
    std::vector<int> hit[2];
    hit[0].assign((size_t)Nx * Nt / 2, 0);
    hit[1].assign((size_t)Nx * Nt / 2, 0);
    for (int x = 0; x < Nx; ++x)
        for (int t = 0; t < Nt; ++t) {
            const int p = site_parity(x, t);
            const size_t h = site_half_index(Nt, x, t);
            CHECK(p == ((x + t) % 2));
            CHECK(h < hit[p].size());
            if (h < hit[p].size()) ++hit[p][h];
        }
    for (int p = 0; p < 2; ++p)
        for (int v : hit[p]) CHECK(v == 1);
}

static void refusals() {
    const double m0[1] = {0.0};
    double C[1];
    int sx[32] = {0}, st[32] = {0};
    int bad = -1;
    auto call = [&](const void *m, const int *x, const int *t, const void *c, int solver, int nsrc, int max_iter,
                    int Nx, int Nt) { return args_refusal(m, x, t, c, solver, nsrc, 64, max_iter, Nx, Nt, &bad); };
    CHECK(call(m0, sx, st, C, 0, 1, 10, 6, 10) == PION_OK);
    CHECK(call(m0, sx, st, C, 1, 1, 0, 6, 10) == PION_OK);
    CHECK(call(nullptr, sx, st, C, 0, 1, 10, 6, 10) == PION_NULL);
    CHECK(call(m0, nullptr, st, C, 0, 1, 10, 6, 10) == PION_NULL);
    CHECK(call(m0, sx, nullptr, C, 0, 1, 10, 6, 10) == PION_NULL);
    CHECK(call(m0, sx, st, nullptr, 0, 1, 10, 6, 10) == PION_NULL);
    CHECK(call(m0, sx, st, C, 2, 1, 10, 6, 10) == PION_SOLVER);
    CHECK(call(m0, sx, st, C, -1, 1, 10, 6, 10) == PION_SOLVER);
    CHECK(call(m0, sx, st, C, 0, 0, 10, 6, 10) == PION_NSRC);
    CHECK(call(m0, sx, st, C, 0, -3, 10, 6, 10) == PION_NSRC);
    CHECK(call(m0, sx, st, C, 0, 33, 10, 6, 10) == PION_NSRC);   // 2 nsrc above the cap: no coordinate is read
    CHECK(call(m0, sx, st, C, 0, 32, 10, 6, 10) == PION_OK);     // the cap itself
    CHECK(call(m0, sx, st, C, 0, 1, -1, 6, 10) == PION_MAX_ITER);
    sx[2] = 6;
    CHECK(call(m0, sx, st, C, 0, 3, 10, 6, 10) == PION_COORD && bad == 2);
    CHECK(call(m0, sx, st, C, 0, 2, 10, 6, 10) == PION_OK);      // sources past nsrc are not looked at
    sx[2] = -1;
    CHECK(call(m0, sx, st, C, 0, 3, 10, 6, 10) == PION_COORD && bad == 2);
    sx[2] = 5;
    st[1] = 10;
    CHECK(call(m0, sx, st, C, 0, 3, 10, 6, 10) == PION_COORD && bad == 1);
    st[1] = -1;
    CHECK(call(m0, sx, st, C, 0, 3, 10, 6, 10) == PION_COORD && bad == 1);
    st[1] = 9;
    CHECK(call(m0, sx, st, C, 0, 3, 10, 6, 10) == PION_OK);
    sx[2] = 4;
    st[1] = 8;
    CHECK(call(m0, sx, st, C, 1, 3, 10, 5, 9) == PION_CHECKERBOARD);
    CHECK(call(m0, sx, st, C, 1, 3, 10, 6, 9) == PION_CHECKERBOARD);
    CHECK(call(m0, sx, st, C, 1, 3, 10, 5, 10) == PION_CHECKERBOARD);
    CHECK(call(m0, sx, st, C, 0, 3, 10, 5, 9) == PION_OK);       // solver 0 has no checkerboard
}

int main() {
    layouts(1, 1, 1);
    layouts(3, 4, 10);
    layouts(64, 32, 9);
    checkerboard(6, 10);
    checkerboard(16, 62);
    checkerboard(8, 122);
    refusals();
    if (failures) return 1;
    std::puts("pion_host_check ok");
    return 0;
}
