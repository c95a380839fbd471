// f110_host_util.h — what every host file of libf110.so shares (host only, private): the error
// path of the C ABI and the one device allocator of the handle types.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>
#include <vector>

#include "../../include/f110.h"

// One thread-local error string per library (f110_host.cpp); returns `code`.
int f110_set_error(int code, const std::string &msg);

namespace f110 {

inline int fail(int code, const std::string &msg) { return f110_set_error(code, msg); }

// "<fn>: <HIP's error text>" under `code` (F110_E_HIP, or F110_E_ALLOC for a create's allocations)
inline int hip_fail(const char *fn, hipError_t e, int code = F110_E_HIP) {
    return fail(code, std::string(fn) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return ::f110::hip_fail(#expr, e_); \
    } while (0)

// The device buffers of one handle (a context, a replay ring, an n-step accumulator, a track, a
// map-table entry): allocated one by one, freed together by release() or the destructor, with the
// handle's device current.  A create that fails half way and the handle's destroy free through
// this one path.
struct DeviceArena {
    int device = 0;
    std::vector<void *> allocs;

    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { release(); }

    // n elements of T plus `slack` bytes (the replay and n-step buffers keep 16 behind their
    // vectorised row copies), or `empty_bytes` where that is 0; `zero` fills all of it.  The two
    // corner cases of a memset that fails after its hipMalloc succeeded, decided once: the pointer
    // is always recorded, so release() frees it, and *p is never published on failure.
    template <class T>
    hipError_t alloc(T **p, size_t n, bool zero, size_t slack = 0, size_t empty_bytes = 0) {
        size_t bytes = n * sizeof(T) + slack;
        if (bytes == 0) bytes = empty_bytes;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        allocs.push_back(q);
        if (zero) e = hipMemset(q, 0, bytes);
        if (e == hipSuccess) *p = static_cast<T *>(q);
        return e;
    }

    // a buffer (with `slack` bytes more) holding a copy of the n elements at src; a failed copy frees
    // the buffer at once and leaves *p untouched
    template <class T>
    hipError_t upload(const T **p, const T *src, size_t n, size_t slack = 0) {
        T *d = nullptr;
        hipError_t e = alloc(&d, n, /*zero=*/false, slack);
        if (e != hipSuccess) return e;
        e = hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            allocs.pop_back();
            return e;
        }
        *p = d;
        return hipSuccess;
    }

    void release() {
        if (allocs.empty()) return;
        (void)hipSetDevice(device);
        for (void *q : allocs) (void)hipFree(q);
        allocs.clear();
    }
};

}  // namespace f110
