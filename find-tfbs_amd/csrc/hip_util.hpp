// HIP helpers of the host drivers: the error macro, the owning device buffer, the
// page-locked array and the event and stream handles.  Every holder frees what it owns
// in its destructor and cannot be copied.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "tfbs_internal.hpp"

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return tfbs::fail(TFBS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));               \
    } while (0)

namespace tfbs {

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// Device memory that only grows.  ensure: geometric (the pipelined callers' buffers);
// ensure_exact: the asked size (buffers sized to a scratch budget).
template <typename T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), n(o.n) { o.p = nullptr, o.cap = o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p, o.p), std::swap(cap, o.cap), std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t want) {
        n = want;
        if (want <= cap) return TFBS_OK;
        // geometric growth (hipFree waits for the device: a buffer regrown per call
        // would serialise the pipelined callers), the exact size if that fails
        return grow(std::max<size_t>({want, cap + cap / 2, 16}), want);
    }
    int ensure_exact(size_t want, size_t floor = 1) {
        n = want;
        if (want <= cap) return TFBS_OK;
        const size_t c = std::max(want, floor);
        return grow(c, c);
    }
    template <class Alloc>
    int put(const std::vector<T, Alloc> &v, hipStream_t s) {
        int rc = ensure(v.size());
        if (rc) return rc;
        if (!v.empty()) HIP_TRY(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        return TFBS_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = n = 0;
    }

private:
    int grow(size_t c, size_t least) {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, c * sizeof(T));
        if (e != hipSuccess && c > least) {
            (void)hipGetLastError();
            c = least;
            e = hipMalloc(&p, c * sizeof(T));
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(TFBS_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        cap = c;
        return TFBS_OK;
    }
};

// A page-locked array, allocated once at its first use.
template <typename T>
struct PinnedArray : NoCopy {
    T *p = nullptr;
    ~PinnedArray() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t alloc(size_t count) {
        return p ? hipSuccess : hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault);
    }
    T &operator[](size_t i) const { return p[i]; }
    explicit operator bool() const { return p != nullptr; }
};

struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() { return hipEventCreate(&e); }                                       // timed
    hipError_t create_untimed() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    operator hipEvent_t() const { return e; }
};

struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

}  // namespace tfbs
