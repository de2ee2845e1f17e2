// The exact scoring code of the brute-force kernels (scan_hits.hip, scan_best.hip) and the
// small host helpers of their drivers.  A HIP header: only .hip sources include it.
//
// A lane takes the bases of its window 16 at a time: two packed words and two N-mask
// words funnel-shifted to the window's phase.  It has up to four 64-window chunks' windows
// in flight: their words are loaded together and a column's weights are fetched once.  The
// strand is wave-uniform: a mono column's four weights come through one scalar load and
// three selects, a dinucleotide strand's rows (at most 31 x 16 ints) sit in the wave's LDS
// slice, where the 16 entries of a row lie on 16 banks (lanes on one entry broadcast).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <string>

#include "hits.hpp"
#include "scan.hpp"

namespace tfbs {

constexpr uint32_t kHitWaves = 4;                       // waves (pairs) per workgroup
constexpr uint32_t kHitBlock = 64 * kHitWaves;
constexpr int kHitChunks = 4;                           // 64-window chunks a lane has in flight
constexpr uint32_t kHitDiInts = (kDiMaxLen - 1) * 16;   // a dinucleotide strand's rows
constexpr uint64_t kHitsMaxPairs = 1ull << 30;          // pairs per launch: the grid stays below 2^31

typedef const __attribute__((address_space(4))) DevHitStrand CStrand;  // wave-uniform: scalar loads
struct alignas(16) Col4 {  // one mono column: [A,C,G,T]
    int32_t x, y, z, w;
};
typedef const __attribute__((address_space(4))) Col4 CInt4;

// The 16 bases from base q of a haplotype (2 bits each, base q lowest) and their N bits.
__device__ __forceinline__ void bases16(const uint32_t *W, const uint32_t *M, uint32_t q, uint32_t &bits,
                                        uint32_t &nm) {
    const uint32_t wi = q >> 4;
    bits = __builtin_amdgcn_alignbit(W[wi + 1], W[wi], 2 * (q & 15));
    nm = M ? __builtin_amdgcn_alignbit(M[(q >> 5) + 1], M[q >> 5], q & 31) : 0u;
}

// Wrapping column sums of the windows at bases i[0 .. NCH) (one per 64-window chunk in
// flight: their words are loaded together, a column's weights once); an N column adds 0.
template <int NCH>
__device__ __forceinline__ void score_mono(const uint32_t *W, const uint32_t *M, const uint32_t (&i)[NCH], uint32_t L,
                                           CInt4 *wq, uint32_t (&s)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; c++) s[c] = 0;
    for (uint32_t g = 0; g < L; g += 16) {  // (wave-uniform trip counts)
        uint32_t bits[NCH], nm[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) bases16(W, M, i[c] + g, bits[c], nm[c]);
        const uint32_t cnt = min(16u, L - g);
        for (uint32_t t = 0; t < cnt; t++) {
            CInt4 &w = wq[g + t];
            const int32_t wa = w.x, wc = w.y, wg = w.z, wt = w.w;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint32_t b = bits[c] & 3u;
                const int32_t v = b == 0 ? wa : b == 1 ? wc : b == 2 ? wg : wt;
                s[c] += (nm[c] & 1u) ? 0u : (uint32_t)v;
                bits[c] >>= 2;
                nm[c] >>= 1;
            }
        }
    }
}

// Wrapping pair sums of the windows at bases i[0 .. NCH) (L <= 32 bases); a pair holding an
// N adds 0.
template <int NCH>
__device__ __forceinline__ void score_dinuc(const uint32_t *W, const uint32_t *M, const uint32_t (&i)[NCH],
                                            uint32_t L, const int32_t *rows, uint32_t (&s)[NCH]) {
    uint32_t prev[NCH], prevn[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) s[c] = 0, prev[c] = 0, prevn[c] = 1;  // (no pair ends on the first base)
    for (uint32_t g = 0; g < L; g += 16) {
        uint32_t bits[NCH], nm[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) bases16(W, M, i[c] + g, bits[c], nm[c]);
        const uint32_t cnt = min(16u, L - g);
        for (uint32_t t = 0; t < cnt; t++) {
            const uint32_t j = g + t;  // the pair (base j - 1, base j) is row j - 1
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint32_t b = bits[c] & 3u, n = nm[c] & 1u;
                const int32_t v = j ? rows[16 * (j - 1) + 4 * prev[c] + b] : 0;
                s[c] += (n | prevn[c]) ? 0u : (uint32_t)v;
                prev[c] = b;
                prevn[c] = n;
                bits[c] >>= 2;
                nm[c] >>= 1;
            }
        }
    }
}

// A dinucleotide strand's rows into a wave's LDS slice (L <= kDiMaxLen: check_dipwm_length).
__device__ __forceinline__ void stage_dinuc_rows(int32_t *slice, const int32_t *weights, uint32_t w_off, uint32_t L,
                                                 uint32_t lane) {
    const uint32_t n = min((L - 1) * 16, kHitDiInts);
    for (uint32_t x = lane; x < n; x += 64) slice[x] = weights[w_off + x];
}

template <typename T>
struct Buf {  // a device buffer that only grows
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return TFBS_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(TFBS_E_HIP, std::string("hipMalloc (hit lists): ") + hipGetErrorString(e));
        }
        cap = n;
        return TFBS_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

#define HITS_TRY(expr)                                                                       \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(TFBS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The scratch budget of an environment variable in MiB (fractions too; read at the call).
inline uint64_t scratch_budget(const char *name, double dflt_mb) {
    const char *env = getenv(name);
    const double mb = env && *env ? strtod(env, nullptr) : dflt_mb;
    return mb > 0 ? (uint64_t)std::min(mb * 1048576.0, 9.0e18) : 0;
}

}  // namespace tfbs
