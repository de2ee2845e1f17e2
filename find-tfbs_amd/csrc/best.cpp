// Host side of the best sites (include/tfbs_amd.h, "Best sites"): a region's distinct
// inner ranges and the TSV of best records.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <string>

#include "key_tsv.hpp"

namespace tfbs {
namespace {

struct BestPolicy {
    using Rec = tfbs_best;
    using Value = const tfbs_best *;  // null: "none"
    static constexpr const char *word = "best", *all_kind = "best", *hap_dots = "\t.\t.\t.\t.\t.\t";
    // The best over the pattern_id's strands: the highest score, ties to the strand earlier in creation order.
    Value value_of(const tfbs_best *hap_block, const std::vector<uint32_t> &strands, uint32_t nr, uint32_t slot) const {
        const tfbs_best *v = nullptr;
        for (uint32_t p : strands) {
            const tfbs_best *x = hap_block + (size_t)p * nr + slot;
            if (x->n_windows && (!v || x->score > v->score)) v = x;
        }
        return v;
    }
    bool differs(Value a, Value b) const { return !a != !b || (a && a->score != b->score); }
    void columns(std::string &out, const Batch &B, uint32_t, Value v, const Value *base) const {
        char buf[160];
        if (v)
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "%c\t%" PRIu64 "\t%" PRIu64 "\t%d\t",
                                             B.pats->pats[v->pattern].direction == TFBS_DIR_N ? '-' : '+', v->start,
                                             v->end, v->score));
        else
            out += ".\t.\t.\t.\t";
        if (v && base && *base)
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "%" PRId64, (int64_t)v->score - (int64_t)(*base)->score));
        else
            out += '.';
    }
};

}  // namespace

int best_tsv(const Batch &B, const tfbs_best *best, size_t n, const std::string &chrom, int mode, std::string &out) {
    if (mode != TFBS_BEST_ALL && mode != TFBS_BEST_DIFF) return fail(TFBS_E_ARG, "best mode is TFBS_BEST_ALL or TFBS_BEST_DIFF");
    return key_tsv(BestPolicy{}, B, best, n, chrom, mode == TFBS_BEST_DIFF, out);
}

}  // namespace tfbs

extern "C" {

int tfbs_batch_region_num_ranges(const tfbs_batch *b, size_t region, size_t *n) {
    if (!b || !n) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (region >= b->b.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region");
    *n = b->b.rh[region].ranges.size();
    return TFBS_OK;
}

int tfbs_batch_region_range(const tfbs_batch *b, size_t region, size_t k, uint64_t *start, uint64_t *end) {
    if (!b || !start || !end) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (region >= b->b.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region");
    const auto &ranges = b->b.rh[region].ranges;  // inner_keys: ascending (start, end), no repeats
    if (k >= ranges.size()) return tfbs::fail(TFBS_E_ARG, "bad range index");
    *start = ranges[k].first;
    *end = ranges[k].second;
    return TFBS_OK;
}

int tfbs_batch_best_tsv(const tfbs_batch *b, const tfbs_best *best, size_t n, const char *chromosome, int mode,
                        char **text, size_t *len) {
    if (!b || !chromosome || !text || !len || (n && !best)) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::string out;
    if (int rc = tfbs::best_tsv(b->b, best, n, chromosome, mode, out)) return rc;
    return tfbs::text_out(out, text, len);
}

}  // extern "C"
