// The inner-range counting shared by the dense scan kernels (scan_kernels.hip,
// scan_dinuc.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tfbs_internal.hpp"

namespace tfbs {

// Count, for every inner range of this pass, the hit windows whose match range
// overlaps it (main.rs:503 with Range::overlaps, range.rs:18-21), and add the
// counts to the lane that owns the pattern_id slot.  Rare: only runs when a
// ballot found a hit, so the inner ranges are loaded here, not kept in registers.
template <int NCH>
__device__ __forceinline__ void count_hits(const uint64_t (&hit)[NCH], const int32_t (&pos)[NCH], uint32_t L,
                                           const int32_t *inner, uint32_t n_pass, uint32_t slot, uint32_t lane,
                                           uint32_t (&acc)[kMaxInnerPass]) {
#pragma unroll
    for (int kk = 0; kk < kMaxInnerPass; kk++) {
        if ((uint32_t)kk >= n_pass) break;
        const int32_t s = inner[2 * kk];
        const uint32_t span = (uint32_t)(inner[2 * kk + 1] - s);
        uint32_t cnt = 0;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (!hit[c]) continue;
            int32_t p = pos[c];
            asm volatile("" : "+v"(p));  // keep the overlap test here, not hoisted into the hot loop
            const bool ov = (uint32_t)(p - s) <= span || (uint32_t)(p + (int32_t)L - 1 - s) <= span;
            cnt += __popcll(hit[c] & __ballot(ov));
        }
        acc[kk] += (lane == slot) ? cnt : 0u;
    }
}

}  // namespace tfbs
