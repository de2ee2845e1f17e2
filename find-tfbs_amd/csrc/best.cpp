// Host side of the best sites (include/tfbs_amd.h, "Best sites"): a region's distinct
// inner ranges and the TSV of best records.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <map>
#include <string>

#include "hits.hpp"

namespace tfbs {
namespace {

// The value of (haplotype, pattern_id, key): the best over the pattern_id's strands, the
// highest score, ties to the strand earlier in creation order; null: "none".
const tfbs_best *value_of(const tfbs_best *hap_block, const std::vector<uint32_t> &strands, uint32_t nr, uint32_t slot) {
    const tfbs_best *v = nullptr;
    for (uint32_t p : strands) {
        const tfbs_best *x = hap_block + (size_t)p * nr + slot;
        if (x->n_windows && (!v || x->score > v->score)) v = x;
    }
    return v;
}

inline bool differs(const tfbs_best *a, const tfbs_best *b) {
    return !a != !b || (a && a->score != b->score);
}

struct BestLine {
    std::string &out;
    const std::string &chrom;
    const Batch &B;
    char region[48];
    void head(const InnerKey *k, const Pat *p) { tsv_key_head(out, chrom, region, B, k, p); }
    void hap(uint32_t h, uint32_t carriers, const std::string &ids) {
        char buf[64];
        head(nullptr, nullptr);
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%u\thap\t.\t.\t.\t.\t.\t", h, carriers));
        out += ids;
        out += '\n';
    }
    void value(const InnerKey &k, const Pat &first, uint32_t h, uint32_t carriers, const char *kind, const tfbs_best *v,
               const tfbs_best *base) {
        char buf[160];
        head(&k, &first);
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%u\t%s\t", h, carriers, kind));
        if (v)
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "%c\t%" PRIu64 "\t%" PRIu64 "\t%d\t",
                                             B.pats->pats[v->pattern].direction == TFBS_DIR_N ? '-' : '+', v->start,
                                             v->end, v->score));
        else
            out += ".\t.\t.\t.\t";
        if (v && base) out.append(buf, (size_t)snprintf(buf, sizeof buf, "%" PRId64, (int64_t)v->score - (int64_t)base->score));
        else out += '.';
        out += "\t.\n";
    }
};

}  // namespace

void tsv_key_head(std::string &out, const std::string &chrom, const char *region, const Batch &B, const InnerKey *k,
                  const Pat *p) {
    char buf[96];
    out += chrom;
    out += '\t';
    out += region;
    if (!k) {
        out += "\t.\t.\t.\t.\t.";
        return;
    }
    out += '\t';
    out += B.beds[k->bed];
    out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%" PRIu64 "\t%" PRIu64 "\t", k->s, k->e));
    out += p->name;
    out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u", (unsigned)p->pattern_id));
}

int best_tsv(const Batch &B, const tfbs_best *best, size_t n, const std::string &chrom, int mode, std::string &out) {
    if (mode != TFBS_BEST_ALL && mode != TFBS_BEST_DIFF) return fail(TFBS_E_ARG, "best mode is TFBS_BEST_ALL or TFBS_BEST_DIFF");
    const Patterns &P = *B.pats;
    const uint32_t np = (uint32_t)P.pats.size();
    std::map<uint16_t, std::vector<uint32_t>> by_pid;  // ascending pattern_id -> its strands in creation order
    for (uint32_t p = 0; p < np; p++) by_pid[P.pats[p].pattern_id].push_back(p);
    BestLine L{out, chrom, B, {0}};
    size_t at = 0;
    uint32_t prev = 0;
    bool any = false;
    while (at < n) {
        const uint32_t r = best[at].region;
        if (r >= B.rh.size() || (any && r <= prev)) return fail(TFBS_E_ARG, "best records: regions not ascending inside the batch");
        any = true;
        prev = r;
        const RegionH &R = B.rh[r];
        const uint32_t U = R.hap_count, nr = (uint32_t)R.ranges.size();
        const size_t block = (size_t)U * np * nr;
        if (block == 0 || n - at < block) return fail(TFBS_E_ARG, "best records: not a whole region");
        const tfbs_best *blk = best + at;
        size_t x = 0;
        for (uint32_t h = 0; h < U; h++)  // dense and sorted: the block reshapes to [h][p][k]
            for (uint32_t p = 0; p < np; p++)
                for (uint32_t k = 0; k < nr; k++, x++)
                    if (blk[x].region != r || blk[x].haplotype != h || blk[x].pattern != p || blk[x].range != k)
                        return fail(TFBS_E_ARG, "best records: not a whole region sorted by (haplotype, pattern, range)");
        at += block;
        snprintf(L.region, sizeof L.region, "%" PRIu64 "-%" PRIu64, R.ms, R.me);
        auto val = [&](uint32_t h, const std::vector<uint32_t> &strands, const InnerKey &k) {
            return value_of(blk + (size_t)h * np * nr, strands, nr, (uint32_t)k.slot);
        };
        auto carriers = [&](uint32_t h) { return B.hap_carriers[R.hap_begin + h]; };
        uint32_t base = 0;
        if (mode == TFBS_BEST_DIFF) {
            std::vector<std::vector<uint32_t>> ids;
            if (int rc = region_baseline(B, R, ids, &base)) return rc;
            for (uint32_t h = 0; h < U; h++) L.hap(h, carriers(h), carrier_id_text(B, ids, h, base));
        }
        for (const InnerKey &k : R.keys) {  // sorted by (s, e, bed): the rows' order; each once
            if (k.slot < 0) continue;       // an empty inner range
            for (const auto &ps : by_pid) {
                const Pat &first = P.pats[ps.second[0]];
                if (mode == TFBS_BEST_ALL) {
                    for (uint32_t h = 0; h < U; h++) L.value(k, first, h, carriers(h), "best", val(h, ps.second, k), nullptr);
                    continue;
                }
                const tfbs_best *vb = val(base, ps.second, k);
                bool wrote = false;
                for (uint32_t h = 0; h < U; h++) {
                    if (h == base) continue;
                    const tfbs_best *vh = val(h, ps.second, k);
                    if (!differs(vh, vb)) continue;
                    if (!wrote) L.value(k, first, base, carriers(base), "base", vb, nullptr);
                    wrote = true;
                    L.value(k, first, h, carriers(h), "alt", vh, vb);
                }
            }
        }
    }
    return TFBS_OK;
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
