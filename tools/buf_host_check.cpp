// buf_host_check.cpp -- BufGroup (csrc/sm_buf.h) on fake raw calls, under the
// host sanitizers: no device. The failure paths of every lazily allocated GPU
// workspace are this type's, and a GPU test could reach them only by exhausting
// a card's memory.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/buf_host_check.cpp -o build/buf_host_check && build/buf_host_check
//
// The raw calls here are malloc / free with a log of every (kind, bytes) asked
// for and of every free (kind, which request it returns), and a failure
// injected at a chosen request. Covers, for a set of 8 requests of mixed kinds
// and a failure at every position: SM_ERR_HIP, every slot null, exactly the
// earlier allocations freed and each by its own kind, the message's who / what /
// bytes, and a full build afterwards in the original order; release() twice
// and release() before the destructor; a regrow frees the whole old set before
// its first request. Leaks and double frees are the sanitizer's to find.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../schwingermodel_amd/csrc/sm_buf.h"

using namespace sm_host;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct sm_ctx {
    int tag;
};

namespace {

struct Event {
    bool free;      // else an allocation (also a failed one: index -1)
    BufKind kind;
    size_t bytes;   // asked for; of the allocation a free returns
    long index;     // which successful allocation (in order since reset) it is / returns
    bool operator==(const Event &o) const {
        return free == o.free && kind == o.kind && bytes == o.bytes && index == o.index;
    }
};

constexpr int kFakeError = 2;  // "out of memory"

std::vector<Event> g_log;
std::map<void *, Event> g_live;  // by pointer: the allocation's event
long g_allocs = 0, g_requests = 0, g_fail_at = -1;
int g_bad_free = 0, g_bad_ctx = 0;
sm_ctx g_ctx{7};
std::string g_err;

void reset(long fail_at) {
    g_log.clear();
    g_allocs = g_requests = 0;
    g_fail_at = fail_at;
    g_err.clear();
}

}  // namespace

namespace sm_host {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int buf_raw_alloc(sm_ctx *c, BufKind kind, void **p, size_t bytes) {
    if (kind == BufKind::streamed && c != &g_ctx) ++g_bad_ctx;
    if (g_requests++ == g_fail_at) {
        g_log.push_back(Event{false, kind, bytes, -1});
        *p = nullptr;
        return kFakeError;
    }
    *p = std::malloc(bytes ? bytes : 1);
    const Event e{false, kind, bytes, g_allocs++};
    g_log.push_back(e);
    g_live[*p] = e;
    return 0;
}

void buf_raw_free(sm_ctx *c, BufKind kind, void *p) {
    if (kind == BufKind::streamed && c != &g_ctx) ++g_bad_ctx;
    auto it = g_live.find(p);
    if (it == g_live.end()) {  // null, a pointer never handed out, or freed before
        ++g_bad_free;
        return;
    }
    g_log.push_back(Event{true, kind, it->second.bytes, it->second.index});
    if (kind != it->second.kind) ++g_bad_free;
    g_live.erase(it);
    std::free(p);
}

const char *buf_raw_error(int err) { return err == kFakeError ? "fake out of memory" : "fake error"; }

}  // namespace sm_host

namespace {

// A workspace shaped like the library's: arrays of slots, mixed types and kinds.
struct Ws {
    float *d[3] = {};
    double *w = nullptr;
    char *codes = nullptr;
    long *partials = nullptr;
    int *h_sc = nullptr, *sc = nullptr;
    BufGroup bufs{"check solver", &g_ctx};
};

struct Req {
    BufKind kind;
    size_t bytes;
    const char *what;
};

// the requests of build(ws, K) in order
std::vector<Req> requests(size_t K) {
    return {{BufKind::streamed, 4 * 10 * K, "direction buffer"}, {BufKind::streamed, 4 * 10 * K, "direction buffer"},
            {BufKind::streamed, 4 * 10 * K, "direction buffer"}, {BufKind::device, 8 * 30 * K, "work"},
            {BufKind::device, 13, "codes"},                      {BufKind::device, sizeof(long) * 5 * K, "partials"},
            {BufKind::pinned, sizeof(int) * K, "pinned scalars"}, {BufKind::device, sizeof(int) * K, "scalars"}};
}

int build(Ws &ws, size_t K) {
    BufGroup &b = ws.bufs;
    int rc = SM_OK;
    for (float *&d : ws.d)
        if (rc == SM_OK) rc = b.add(&d, 10 * K, BufKind::streamed, "direction buffer");
    if (rc == SM_OK) rc = b.add(&ws.w, 30 * K, BufKind::device, "work");
    if (rc == SM_OK) rc = b.add_bytes(&ws.codes, 13, BufKind::device, "codes");
    if (rc == SM_OK) rc = b.add(&ws.partials, 5 * K, BufKind::device, "partials");
    if (rc == SM_OK) rc = b.add(&ws.h_sc, K, BufKind::pinned, "pinned scalars");
    if (rc == SM_OK) rc = b.add(&ws.sc, K, BufKind::device, "scalars");
    return rc;
}

bool all_null(const Ws &ws) {
    return !ws.d[0] && !ws.d[1] && !ws.d[2] && !ws.w && !ws.codes && !ws.partials && !ws.h_sc && !ws.sc;
}
bool none_null(const Ws &ws) {
    return ws.d[0] && ws.d[1] && ws.d[2] && ws.w && ws.codes && ws.partials && ws.h_sc && ws.sc;
}

// allocations first .. first + n - 1 of req (allocation indices from index0), then their frees if asked
std::vector<Event> expect_allocs(const std::vector<Req> &req, size_t n, long index0 = 0) {
    std::vector<Event> e;
    for (size_t i = 0; i < n; ++i) e.push_back(Event{false, req[i].kind, req[i].bytes, index0 + (long)i});
    return e;
}
void append_frees(std::vector<Event> &e, const std::vector<Req> &req, size_t n, long index0 = 0) {
    for (size_t i = 0; i < n; ++i) e.push_back(Event{true, req[i].kind, req[i].bytes, index0 + (long)i});
}

void failure_at_every_position() {
    const size_t K = 3;
    const std::vector<Req> req = requests(K);
    const size_t N = req.size();
    CHECK(N >= 6);
    for (size_t i = 0; i < N; ++i) {
        Ws ws;
        reset((long)i);
        CHECK(build(ws, K) == SM_ERR_HIP);
        CHECK(all_null(ws));
        CHECK(ws.bufs.empty());
        CHECK(g_live.empty());
        // the i allocations, the failed request, then exactly those i freed, each by its own kind
        std::vector<Event> want = expect_allocs(req, i);
        want.push_back(Event{false, req[i].kind, req[i].bytes, -1});
        append_frees(want, req, i);
        CHECK(g_log == want);
        CHECK(g_err.find("check solver: allocating ") == 0);
        CHECK(g_err.find(" " + std::to_string(req[i].bytes) + " bytes ") != std::string::npos);
        CHECK(g_err.find(std::string("(") + req[i].what + ")") != std::string::npos);
        CHECK(g_err.find("fake out of memory") != std::string::npos);
        // the next call builds the whole set, in the original order
        reset(-1);
        CHECK(build(ws, K) == SM_OK);
        CHECK(none_null(ws));
        CHECK(!ws.bufs.empty());
        CHECK(g_log == expect_allocs(req, N));
        CHECK(g_live.size() == N);
        // the destructor frees it, each by its own kind
    }
    CHECK(g_live.empty());
    std::vector<Event> want = expect_allocs(req, N);
    append_frees(want, req, N);
    CHECK(g_log == want);
}

void release_is_idempotent() {
    const std::vector<Req> req = requests(2);
    reset(-1);
    {
        Ws ws;
        CHECK(ws.bufs.empty());
        ws.bufs.release();  // of an empty group
        CHECK(g_log.empty());
        CHECK(build(ws, 2) == SM_OK);
        ws.bufs.release();
        CHECK(all_null(ws) && ws.bufs.empty() && g_live.empty());
        const size_t after_first = g_log.size();
        CHECK(after_first == 2 * req.size());
        ws.bufs.release();
        CHECK(g_log.size() == after_first);
        // release() followed by the destructor
    }
    CHECK(g_log.size() == 2 * req.size());
}

void regrow_frees_the_old_set_first() {
    const std::vector<Req> small = requests(2), large = requests(5);
    const size_t N = small.size();
    reset(-1);
    {
        Ws ws;
        CHECK(build(ws, 2) == SM_OK);
        ws.bufs.release();
        CHECK(build(ws, 5) == SM_OK);
        CHECK(none_null(ws));
        std::vector<Event> want = expect_allocs(small, N);
        append_frees(want, small, N);
        const std::vector<Event> grown = expect_allocs(large, N, (long)N);
        want.insert(want.end(), grown.begin(), grown.end());
        CHECK(g_log == want);
    }
    CHECK(g_live.empty());
    // a regrow whose third request fails leaves nothing behind either
    reset((long)N + 2);
    {
        Ws ws;
        CHECK(build(ws, 2) == SM_OK);
        ws.bufs.release();
        CHECK(build(ws, 5) == SM_ERR_HIP);
        CHECK(all_null(ws) && ws.bufs.empty() && g_live.empty());
    }
}

// slots of two groups side by side, as in sm_ctx: one's failure leaves the other's alone
void groups_are_independent() {
    reset(1);
    double *a = nullptr, *b = nullptr;
    BufGroup ga("a"), gb("b");
    CHECK(ga.add(&a, 4, BufKind::device, "a") == SM_OK);
    CHECK(gb.add(&b, 4, BufKind::pinned, "b") == SM_ERR_HIP);
    CHECK(a && !b && !ga.empty() && gb.empty());
    CHECK(g_err.find("b: allocating 32 bytes (b) failed") == 0);
}

}  // namespace

int main() {
    failure_at_every_position();
    release_is_idempotent();
    regrow_frees_the_old_set_first();
    groups_are_independent();
    CHECK(g_live.empty());
    CHECK(g_bad_free == 0);
    CHECK(g_bad_ctx == 0);
    if (failures) return 1;
    std::puts("buf_host_check ok");
    return 0;
}
