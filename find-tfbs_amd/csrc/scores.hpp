// Score rows (tfbs_batch_score_rows; include/tfbs_amd.h, "Score rows"): the interface of
// score_rows.hip to ctx_outputs.hip, and the host-only definition (scores.cpp) that the device's
// text equals byte for byte.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "hits.hpp"

namespace tfbs {

// A sample's class and DS numerator from d = x - lo (0 <= d <= spread, spread > 0):
// cls 0 / 1 / 2 = 0|0 / 0|1 / 1|1, t = round_half_even(20000 d / spread).  Integers only;
// the kernels (score_rows.hip) and the host function share it.
#if defined(__HIPCC__)
#define TFBS_HD __host__ __device__
#else
#define TFBS_HD
#endif
TFBS_HD inline void score_class(uint64_t d, uint64_t spread, uint32_t *cls, uint32_t *t) {
    *cls = d == 0 ? 0u : d == spread ? 2u : 4 * d < spread ? 0u : 4 * d < 3 * spread ? 1u : 2u;
    const uint64_t num = 20000 * d, q = num / spread, rem = num - q * spread;  // (d < 2^33: no overflow)
    *t = (uint32_t)(2 * rem > spread ? q + 1 : 2 * rem == spread ? q + (q & 1) : q);
}
#undef TFBS_HD

// counts_as_genotypes' rule on the three class counts (main.rs:482-489).
inline uint64_t maf_of(uint64_t zero, uint64_t one, uint64_t two) {
    if (zero >= one && zero >= two) return one + two;
    if (two >= zero && two >= one) return zero + one;
    return zero + two;
}

// chromosome.replace("chr", "") (aggregate.cpp)
std::string strip_chr(const std::string &c);

// The row's INFO value: "SCORES=<lo>,<hi>;freqs=<zero>/<one>/<two>".
std::string score_info(int64_t lo, int64_t hi, uint64_t zero, uint64_t one, uint64_t two);

// A sample's field from d = x - lo appended to gts ("\t0|0:0.0", "\t1|1:2.0" or 11 bytes), its
// class counted: the score rows' and the affinity rows' host definitions share it.
void append_row_field(std::string &gts, uint64_t d, uint64_t spread, uint64_t (&cnt)[3]);

// The specification on one candidate row's per-sample values (left[s], right[s]: the two
// haplotypes' best scores): true and info / gts appended when the row exists (n > 0,
// spread > 0, spread >= min_spread); *maf set.
bool scores_as_genotypes(const int32_t *left, const int32_t *right, size_t n, uint64_t min_spread, uint32_t *maf,
                         std::string &info, std::string &gts);

// The head of a written row after "<chr>\t<POS>\t": "<bed>,<name>,<start>-<end>\t.\t.\t.\tPASS\t<info>\tGT:DS".
std::string score_row_head(const Batch &B, const InnerKey &k, uint16_t pattern_id, const std::string &info);

struct ScoresState;
void scores_state_destroy(ScoresState *s);
// The score rows of regions [r0, r1) of B (resident as img on `device`): their text appended
// to *out with POS from *fake (advanced per row), or -- out null -- counted only.  *n_rows:
// the rows.  *state and *best are made on the first call.  Synchronises `stream`.
int scores_run(ScoresState **state, BestState **best, int device, void *stream, const Patterns &P,
               const ScanImage &img, const Batch &B, size_t r0, size_t r1, const std::string &chrom, uint32_t min_maf,
               uint64_t min_spread, uint32_t *fake, std::string *out, uint64_t *n_rows);
// The last scores_run's times (ms): the best kernel, fold + statistics, the text kernel (HIP
// events, summed over the chunks), copy-back + host part (wall).
void scores_last_ms(const ScoresState *s, double out[4]);

// scan_best.hip: the best kernel over one chunk of whole haplotypes for a caller that keeps the
// records on the device.  best_prepare makes *state (the tables) and gives the strands;
// best_launch_chunk uploads the chunk's haplotypes (batch indices ids[0 .. nh)) and their
// records' places (hap_off, nrec records in all), runs the kernel and waits for it:
// record (k, strand, range) is (*recs)[(*d_hap_off)[k] + strand * n_ranges + range].
// *kernel_ms += the kernel's time.  BestState's own timers are left alone.
int best_prepare(BestState **state, int device, void *stream, const Patterns &P, uint32_t *n_strands);
int best_launch_chunk(BestState *state, void *stream, const ScanImage &img, const uint32_t *ids,
                      const uint64_t *hap_off, size_t nh, uint64_t nrec, const uint64_t **d_hap_off,
                      const DevBestRec **recs, double *kernel_ms);

}  // namespace tfbs
