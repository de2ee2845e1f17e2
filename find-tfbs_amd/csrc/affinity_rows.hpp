// Affinity rows (tfbs_batch_affinity_rows; include/tfbs_amd.h, "Affinity rows"): the interface of
// affinity_rows.hip to ctx_outputs.hip, the exact logarithm that its kernels and the host share,
// and the host-only definition (affinity.cpp) that the device's text equals byte for byte.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "hits.hpp"
#include "scores.hpp"

namespace tfbs {

// mlog2(x) = floor(1000 * log2(x)) for x >= 1 (0 .. 63999) and -1 for x = 0, exactly: with
// e = bitlen(x) - 1 and xn = x << (63 - e) it is 1000 e + max{j : P[j] <= xn} over
// P[j] = ceil(2^63 * 2^(j / 1000)) (affinity_log_table.hpp; P[0] = 2^63 <= xn, and 2^(j / 1000)
// is irrational for j != 0, so the integer comparison is the real one).  Ten steps of a binary
// search; integers only.  The kernels (affinity_rows.hip, P staged in LDS) and the host share it.
#if defined(__HIPCC__)
#define TFBS_HD __host__ __device__
#else
#define TFBS_HD
#endif
TFBS_HD inline int32_t affinity_mlog2(uint64_t x, const uint64_t *P) {
    if (x == 0) return -1;
    const uint32_t e = 63u - (uint32_t)__builtin_clzll(x);
    const uint64_t xn = x << (63u - e);
    uint32_t lo = 0, hi = 1000;  // P[lo] <= xn, and (hi == 1000 or xn < P[hi])
#pragma unroll
    for (int k = 0; k < 10; k++) {  // 1000 -> 500 -> 250 -> 125 -> 63 -> 32 -> 16 -> 8 -> 4 -> 2 -> 1
        const uint32_t mid = (lo + hi) >> 1;
        const bool up = P[mid] <= xn;  // (mid == lo once hi - lo == 1: no change)
        lo = up ? mid : lo;
        hi = up ? hi : mid;
    }
    return (int32_t)(1000u * e + lo);
}
#undef TFBS_HD

// mlog2 on the host from the committed table.
int32_t affinity_mlog2_host(uint64_t x);

// The row's INFO value: "LOG2AFF=<lo>,<hi>;AFF=<xlo>,<xhi>;TOP=<top>;freqs=<zero>/<one>/<two>".
std::string affinity_row_info(int64_t lo, int64_t hi, uint64_t xlo, uint64_t xhi, int32_t top, uint64_t zero,
                              uint64_t one, uint64_t two);

// The specification on one candidate row's per-sample values (left[s], right[s]: the two
// haplotypes' affinity sums, each below 2^63): true and info / gts appended when the row exists
// (n > 0, spread > 0, spread >= min_spread, 0 counting as 1); *maf set.
bool affinity_as_genotypes(const uint64_t *left, const uint64_t *right, size_t n, int32_t top, uint64_t min_spread,
                           uint32_t *maf, std::string &info, std::string &gts);

struct AffinityRowsState;
void affinity_rows_state_destroy(AffinityRowsState *s);
// The affinity rows of regions [r0, r1) of B (resident as img on `device`): their text appended
// to *out with POS from *fake (advanced per row), or -- out null -- counted only.  *n_rows: the
// rows.  *state, *frame (the row kinds' shared tables and scratch: the score rows' state) and
// *aff (the affinity kernel's tables) are made on the first call; the timers of *frame and *aff
// are left alone.  Synchronises `stream`.
int affinity_rows_run(AffinityRowsState **state, ScoresState **frame, AffinityState **aff, int device, void *stream,
                      const Patterns &P, const ScanImage &img, const Batch &B, size_t r0, size_t r1,
                      const std::string &chrom, uint32_t min_maf, uint64_t min_spread, uint32_t *fake, std::string *out,
                      uint64_t *n_rows);
// The last affinity_rows_run's times (ms): the affinity kernel, fold + statistics, the text kernel
// (HIP events, summed over the chunks), copy-back + host part (wall).
void affinity_rows_last_ms(const AffinityRowsState *s, double out[4]);
// mlog2 of x[0 .. n) on `device` in one launch of the kernels' own function.
int affinity_mlog2_device(const uint64_t *x, size_t n, int device, int32_t *out);

// scan_affinity.hip: the affinity kernel over one chunk of whole haplotypes for a caller that
// keeps the records on the device, as best_prepare / best_launch_chunk (scores.hpp).
// affinity_prepare makes *state (the tables and the tops; a pattern set that affinity_tops refuses
// is refused) and gives the strands; affinity_region_check is the affinity call's refusal of a
// region of 2^23 bases.  AffinityState's own timers are left alone.
int affinity_prepare(AffinityState **state, int device, void *stream, const Patterns &P, uint32_t *n_strands);
int affinity_region_check(const AffinityState *state, const Batch &B, size_t r, const RegionH &R);
int affinity_launch_chunk(AffinityState *state, void *stream, const ScanImage &img, const uint32_t *ids,
                          const uint64_t *hap_off, size_t nh, uint64_t nrec, const uint64_t **d_hap_off,
                          const DevAffRec **recs, double *kernel_ms);

}  // namespace tfbs
