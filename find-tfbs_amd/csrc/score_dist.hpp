// Exact score distributions of PWM / dinucleotide strands under a uniform background
// (include/tfbs_amd.h, "Thresholds from a p-value"): what the host twin (score_dist.cpp)
// and the device path (score_dist.hip) share -- the limit checks and the entry points.
// The arithmetic of the two is written twice on purpose: each is the other's check.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "patterns.hpp"

namespace tfbs {

constexpr uint32_t kDistMaxLen = 63;              // 4^L fits 128 bits
constexpr uint64_t kDistMaxBinsMono = 1ull << 24;
constexpr uint64_t kDistMaxBinsDi = 1ull << 22;   // four tables, one per last base
constexpr uint32_t kDistStepTile = 256;           // bins a workgroup takes in a gather step
constexpr uint32_t kDistScanTile = 1024;          // bins a workgroup takes in the suffix sum

// One strand as the distribution code takes it.  Step j (a column, or a dinucleotide row)
// moves a bin by shift = weight - lo_j >= 0; after step j the bins 0 .. span[j] - 1 are
// live and bin b stands for the score b + lo_0 + .. + lo_j.
struct DistStrand {
    uint32_t index = 0;           // pattern index (creation order)
    uint32_t L = 0;               // bases
    uint32_t steps = 0;           // columns (mono) or rows (dinucleotide)
    uint32_t width = 4;           // shifts per step: 4 (mono) or 16
    std::vector<uint32_t> shift;  // steps x width
    std::vector<uint32_t> span;   // per step: live bins after it
    uint64_t bins = 1;            // span after the last step (1 for a strand without steps)
    int64_t base = 0;             // the score of bin 0 of the final table
    bool di() const { return width == 16; }
    uint32_t tables() const { return di() ? 4 : 1; }
};

// A strand as an error message names it: 'name' (+) or 'name' (-).
std::string strand_label(const Pat &p);
// The limits of a strand (TFBS_E_ARG naming it) and, when it passes, its steps.
int dist_strand(const Patterns &P, size_t i, DistStrand *out);
int dist_check_pvalue(double p);
// Every PWM / DIPWM strand of the set, in creation order.
int dist_strands(const Patterns &P, std::vector<DistStrand> *out);

// device == -1: the host twin; >= 0: that HIP device.
int score_tails(const Patterns &P, int device, size_t i, const int32_t *scores, size_t n, uint64_t *lo, uint64_t *hi);
int pvalue_thresholds(const Patterns &P, int device, double p, int32_t *min_scores);

// score_dist.hip
int dev_score_tails(const DistStrand &S, int device, const int32_t *scores, size_t n, uint64_t *lo, uint64_t *hi);
int dev_pvalue_thresholds(const std::vector<DistStrand> &S, int device, double p, int32_t *min_scores);

}  // namespace tfbs
