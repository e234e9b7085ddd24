// sm_buf.h -- BufGroup: the owner of every lazily allocated GPU workspace.
//
// A group owns a set of allocations whose pointers live in ordinary raw-pointer
// fields next to it (kernels, launchers and the d[3] / a[2] arrays keep taking
// raw pointers). It is all or nothing: a request that fails frees everything the
// group holds and nulls every slot, so a *_ready function that tests empty()
// can never find, or leave, a half-built workspace; the next call builds again.
// The destructor frees what is left. No HIP here: the three raw calls below are
// defined once in the library (sm_capi.cpp) and once more, with malloc and
// injected failures, in tools/buf_host_check.cpp.
#pragma once
#include "../../include/sm_hip.h"

#include <cstddef>
#include <vector>

struct sm_ctx;

namespace sm_host {

int fail(int code, const char *fmt, ...);

// device: hipMalloc; pinned: hipHostMalloc; streamed: the context's placement
// rule for the buffers a CG pass streams (stream_malloc, sm_place.cpp)
enum class BufKind { device, pinned, streamed };

// 0 and *p, or the error's code with *p = nullptr and no sticky error left (c: the streamed kind's context)
int buf_raw_alloc(sm_ctx *c, BufKind kind, void **p, size_t bytes);
void buf_raw_free(sm_ctx *c, BufKind kind, void *p);
const char *buf_raw_error(int err);

class BufGroup {
  public:
    explicit BufGroup(const char *who, sm_ctx *c = nullptr) : who_(who), c_(c) {}
    BufGroup(const BufGroup &) = delete;
    BufGroup &operator=(const BufGroup &) = delete;
    ~BufGroup() { release(); }

    // *slot = `count` T of `kind`. On failure: release(), SM_ERR_HIP as
    // "<who>: allocating <bytes> bytes (<what>) failed: <HIP error>".
    template <class T>
    int add(T **slot, size_t count, BufKind kind, const char *what) {
        return add_bytes(slot, sizeof(T) * count, kind, what);
    }
    template <class T>
    int add_bytes(T **slot, size_t bytes, BufKind kind, const char *what) {
        void *p = nullptr;
        if (const int err = buf_raw_alloc(c_, kind, &p, bytes)) {
            release();
            return fail(SM_ERR_HIP, "%s: allocating %zu bytes (%s) failed: %s", who_, bytes, what, buf_raw_error(err));
        }
        *slot = static_cast<T *>(p);
        recs_.push_back(Rec{reinterpret_cast<void **>(slot), kind});
        return SM_OK;
    }
    // frees every allocation by its kind's call, in the order of the requests, and nulls its slot
    void release() {
        for (const Rec &r : recs_) {
            buf_raw_free(c_, r.kind, *r.slot);
            *r.slot = nullptr;
        }
        recs_.clear();
    }
    bool empty() const { return recs_.empty(); }

  private:
    struct Rec {
        void **slot;
        BufKind kind;
    };
    const char *who_;
    sm_ctx *c_;
    std::vector<Rec> recs_;
};

}  // namespace sm_host
