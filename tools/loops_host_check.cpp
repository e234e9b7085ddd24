// loops_host_check.cpp -- the quark loops' host index arithmetic and argument
// checks (csrc/sm_loops_host.h) under the host sanitizers: no device.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/loops_host_check.cpp -o build/loops_host_check && build/loops_host_check
//
// Covers: the loops and res layouts tile their arrays exactly once in
// (r, k, t, c) / (r, k) order; the chunks of a lone context's nnoise vectors
// cover 0 .. nnoise - 1 once, in order, none above the batch cap; and every
// refusal of sm_quark_loops / sm_ens_quark_loops, in the order it is made.
#include <cstdio>
#include <vector>

#include "../schwingermodel_amd/csrc/sm_loops_host.h"

using namespace sm_loops_host;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void layouts(int R, int nnoise, int Nt) {
    std::vector<int> L(loops_doubles(R, nnoise, Nt), 0), res((size_t)R * nnoise, 0);
    size_t next = 0, rnext = 0;
    for (int r = 0; r < R; ++r)
        for (int k = 0; k < nnoise; ++k) {
            const size_t j = res_index(nnoise, r, k);
            CHECK(j == rnext++);
            CHECK(j < res.size());
            if (j < res.size()) ++res[j];
            for (int t = 0; t < Nt; ++t)
                for (int c = 0; c < 4; ++c) {
                    const size_t i = loops_index(nnoise, Nt, r, k, t, c);
                    CHECK(i == next++);
                    CHECK(i < L.size());
                    if (i < L.size()) ++L[i];
                }
        }
    for (int v : L) CHECK(v == 1);
    for (int v : res) CHECK(v == 1);
    // the ensemble's contraction launch: replica r's vector k lies r * (4 nnoise Nt) doubles behind replica 0's
    for (int r = 0; r < R; ++r)
        for (int k = 0; k < nnoise; ++k)
            CHECK(loops_index(nnoise, Nt, r, k, 0, 0) ==
                  loops_index(nnoise, Nt, 0, k, 0, 0) + (size_t)r * 4 * (size_t)nnoise * (size_t)Nt);
}

static void chunks(int nnoise, int cap) {
    std::vector<int> hit((size_t)nnoise, 0);
    int next = 0;
    const int n = chunk_count(nnoise, cap);
    CHECK(n >= 1);
    for (int i = 0; i < n; ++i) {
        const int k0 = chunk_first(cap, i), K = chunk_size(nnoise, cap, i);
        CHECK(K >= 1 && K <= cap);
        CHECK(k0 == next);
        for (int b = 0; b < K; ++b) {
            CHECK(k0 + b < nnoise);
            if (k0 + b < nnoise) ++hit[(size_t)(k0 + b)];
        }
        next = k0 + K;
    }
    CHECK(next == nnoise);
    for (int v : hit) CHECK(v == 1);
}

static void refusals() {
    const double m0[1] = {0.0};
    const unsigned long long seed[1] = {1};
    double L[1];
    auto call = [&](const void *m, const void *s, const void *l, int solver, int nnoise, int max_iter, int Nx, int Nt) {
        return args_refusal(m, s, l, solver, nnoise, max_iter, Nx, Nt);
    };
    CHECK(call(m0, seed, L, 0, 1, 10, 6, 10) == LOOPS_OK);
    CHECK(call(m0, seed, L, 1, 1, 0, 6, 10) == LOOPS_OK);
    CHECK(call(m0, seed, L, 0, 1000, 10, 6, 10) == LOOPS_OK);     // nnoise is not capped at the batch size
    CHECK(call(nullptr, seed, L, 0, 1, 10, 6, 10) == LOOPS_NULL);
    CHECK(call(m0, nullptr, L, 0, 1, 10, 6, 10) == LOOPS_NULL);
    CHECK(call(m0, seed, nullptr, 0, 1, 10, 6, 10) == LOOPS_NULL);
    CHECK(call(nullptr, seed, L, 2, 0, -1, 5, 9) == LOOPS_NULL);  // nulls come first
    CHECK(call(m0, seed, L, 2, 1, 10, 6, 10) == LOOPS_SOLVER);
    CHECK(call(m0, seed, L, -1, 1, 10, 6, 10) == LOOPS_SOLVER);
    CHECK(call(m0, seed, L, 2, 0, 10, 6, 10) == LOOPS_SOLVER);    // then the solver
    CHECK(call(m0, seed, L, 0, 0, 10, 6, 10) == LOOPS_NNOISE);
    CHECK(call(m0, seed, L, 1, -5, 10, 6, 10) == LOOPS_NNOISE);
    CHECK(call(m0, seed, L, 0, 0, -1, 6, 10) == LOOPS_NNOISE);    // then nnoise
    CHECK(call(m0, seed, L, 0, 1, -1, 6, 10) == LOOPS_MAX_ITER);
    CHECK(call(m0, seed, L, 1, 1, -1, 5, 9) == LOOPS_MAX_ITER);   // then max_iter
    CHECK(call(m0, seed, L, 1, 3, 10, 5, 9) == LOOPS_CHECKERBOARD);
    CHECK(call(m0, seed, L, 1, 3, 10, 6, 9) == LOOPS_CHECKERBOARD);
    CHECK(call(m0, seed, L, 1, 3, 10, 5, 10) == LOOPS_CHECKERBOARD);
    CHECK(call(m0, seed, L, 0, 3, 10, 5, 9) == LOOPS_OK);         // solver 0 has no checkerboard
}

int main() {
    layouts(1, 1, 1);
    layouts(1, 70, 10);
    layouts(3, 3, 62);
    layouts(64, 16, 9);
    const int caps[] = {1, 2, 64};
    for (int cap : caps)
        for (int n = 1; n <= 3 * cap + 2; ++n) chunks(n, cap);
    chunks(70, 64);
    chunks(1000, 64);
    refusals();
    if (failures) return 1;
    std::puts("loops_host_check ok");
    return 0;
}
