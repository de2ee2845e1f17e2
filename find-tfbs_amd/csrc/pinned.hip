// PinnedBytes (batch.hpp): page-locked host bytes with a pageable fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "batch.hpp"

namespace tfbs {
int PinnedBytes::reserve(size_t n) {
    if (n <= cap) return TFBS_OK;
    // geometric with headroom (page-locking is slow: ~5 ms per 20 MB; the BGZF slots' batches
    // vary 2x in size, and each regrowth stalled the GPU between a batch and its copy back);
    // the old capacity is read before release() clears it
    size_t want = std::max<size_t>({n + n / 2, 2 * cap, (size_t)1 << 20});
    release();
    if (hipHostMalloc((void **)&p, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        want = n;  // the exact size, then pageable memory
        if (hipHostMalloc((void **)&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
        }
    }
    pinned = p != nullptr;
    if (!pinned) {  // page-locked memory exhausted: pageable memory (slower copies, same results)
        p = static_cast<uint8_t *>(malloc(want));
        if (!p) return tfbs::fail(TFBS_E_NOMEM, "host staging buffer");
    }
    cap = want;
    return TFBS_OK;
}
void PinnedBytes::release() {
    if (p) {
        if (pinned) (void)hipHostFree(p);
        else free(p);
    }
    p = nullptr;
    cap = 0;
}
PinnedBytes::~PinnedBytes() { release(); }

}  // namespace tfbs
