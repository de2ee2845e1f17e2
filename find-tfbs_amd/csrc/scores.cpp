// Host side of the score rows (include/tfbs_amd.h, "Score rows"): the definition of a row from
// its per-sample values, which the device's text equals byte for byte, and the rows' heads.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "scores.hpp"

namespace tfbs {

std::string score_info(int64_t lo, int64_t hi, uint64_t zero, uint64_t one, uint64_t two) {
    char buf[128];
    const int m = snprintf(buf, sizeof buf, "SCORES=%" PRId64 ",%" PRId64 ";freqs=%" PRIu64 "/%" PRIu64 "/%" PRIu64, lo,
                           hi, zero, one, two);
    return std::string(buf, (size_t)m);
}

void append_row_field(std::string &gts, uint64_t d, uint64_t spread, uint64_t (&cnt)[3]) {
    uint32_t cls, t;
    score_class(d, spread, &cls, &t);
    cnt[cls]++;
    if (d == 0) gts += "\t0|0:0.0";
    else if (d == spread) gts += "\t1|1:2.0";
    else {
        char buf[16];
        const int m = snprintf(buf, sizeof buf, "\t%s:%u.%04u", cls == 0 ? "0|0" : cls == 1 ? "0|1" : "1|1", t / 10000,
                               t % 10000);
        gts.append(buf, (size_t)m);
    }
}

bool scores_as_genotypes(const int32_t *left, const int32_t *right, size_t n, uint64_t min_spread, uint32_t *maf,
                         std::string &info, std::string &gts) {
    if (n == 0) return false;
    int64_t lo = (int64_t)left[0] + right[0], hi = lo;
    for (size_t i = 1; i < n; i++) {
        const int64_t x = (int64_t)left[i] + right[i];
        lo = std::min(lo, x);
        hi = std::max(hi, x);
    }
    const uint64_t spread = (uint64_t)(hi - lo);
    if (spread == 0 || spread < min_spread) return false;
    uint64_t cnt[3] = {0, 0, 0};
    gts.reserve(gts.size() + n * 11);
    for (size_t i = 0; i < n; i++) append_row_field(gts, (uint64_t)((int64_t)left[i] + right[i] - lo), spread, cnt);
    *maf = (uint32_t)maf_of(cnt[0], cnt[1], cnt[2]);
    info += score_info(lo, hi, cnt[0], cnt[1], cnt[2]);
    return true;
}

std::string score_row_head(const Batch &B, const InnerKey &k, uint16_t pattern_id, const std::string &info) {
    auto it = B.pats->names.find(pattern_id);
    std::string h = B.beds[k.bed];
    h += ',';
    if (it != B.pats->names.end()) h += it->second;
    char buf[96];
    h.append(buf, (size_t)snprintf(buf, sizeof buf, ",%" PRIu64 "-%" PRIu64 "\t.\t.\t.\tPASS\t", k.s, k.e));
    h += info;
    h += "\tGT:DS";
    return h;
}

}  // namespace tfbs

extern "C" {

int tfbs_scores_as_genotypes(const int32_t *left, const int32_t *right, size_t n, uint64_t min_spread, uint32_t *maf,
                             char *info, size_t info_cap, char *genotypes, size_t gt_cap) {
    if (!maf || (n && (!left || !right))) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::string a, g;
    if (!tfbs::scores_as_genotypes(left, right, n, min_spread, maf, a, g)) return 0;
    if (!info || !genotypes || a.size() + 1 > info_cap || g.size() + 1 > gt_cap)
        return tfbs::fail(TFBS_E_ARG, "output capacity too small");
    memcpy(info, a.c_str(), a.size() + 1);
    memcpy(genotypes, g.c_str(), g.size() + 1);
    return 1;
}

}  // extern "C"
