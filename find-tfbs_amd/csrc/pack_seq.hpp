// A patched sequence packed as the variant-effect and mutation-scan kernels read it
// (scan_effects.hip, scan_mutscan.hip): 2-bit words and N-mask words with the batch image's
// pads behind them, and a base's position from the sequence's position runs.  Host only.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "batch.hpp"

namespace tfbs {

// 2-bit words and N-mask words of a sequence with the batch image's pads behind it, sized so
// that what follows starts at a 32-base boundary: 2 (ceil(n / 32) + 2) words (at least the 3
// pads), ceil(n / 32) + 2 mask words.
inline uint32_t mask_words(uint32_t n) { return (n + 31) / 32 + 2; }
inline void pack_seq(const std::vector<uint8_t> &nuc, uint32_t *w, uint32_t *m) {
    const uint32_t n = (uint32_t)nuc.size();
    memset(w, 0, 8 * (size_t)mask_words(n));
    if (m) memset(m, 0, 4 * (size_t)mask_words(n));
    for (uint32_t p = 0; p < n; p++) {  // N (4) packs as A, masked by its N bit
        w[p / 16] |= (uint32_t)(nuc[p] & 3u) << (2 * (p % 16));
        if (m && nuc[p] == 4) m[p / 32] |= 1u << (p % 32);
    }
}
inline bool has_n(const std::vector<uint8_t> &nuc) { return !nuc.empty() && memchr(nuc.data(), 4, nuc.size()); }
inline uint64_t pos_at(const PosRuns &r, uint32_t i) {
    size_t k = 0;
    while (k + 1 < r.r.size() && r.r[k + 1].at <= i) k++;
    return r.r[k].p + (i - r.r[k].at);
}

}  // namespace tfbs
