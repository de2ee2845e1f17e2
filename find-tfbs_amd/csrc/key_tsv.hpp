// The TSV of dense per-key records -- one per (distinct haplotype, pattern strand, inner range),
// whole regions sorted [h][p][k] -- shared by the best sites (best.cpp) and the binding
// affinities (affinity.cpp): the record-block walk and its refusals, the strands of a
// pattern_id, the `hap` lines and the all / base / alt emission over a region's keys.
//
// A policy supplies what differs:
//   Rec, Value           the record type; the value of (haplotype, pattern_id, key)
//   word, all_kind       "best" / "affinity" in the refusals; the kind word of mode "all"
//   hap_dots             a `hap` line's columns between `hap` and carrier_ids
//   value_of(hap_block, strands, nr, slot)   the fold over a pattern_id's strands
//   differs(a, b)        whether a haplotype's value earns an `alt` line against the baseline's
//   columns(out, B, first, v, base)   a value line after its kind column, up to delta (base null: ".")
#pragma once

#include <cinttypes>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "hits.hpp"

namespace tfbs {

template <class Policy>
int key_tsv(const Policy &pol, const Batch &B, const typename Policy::Rec *recs, size_t n, const std::string &chrom,
            bool diff, std::string &out) {
    using Value = typename Policy::Value;
    const std::string what = std::string(Policy::word) + " records: ";
    const Patterns &P = *B.pats;
    const uint32_t np = (uint32_t)P.pats.size();
    std::map<uint16_t, std::vector<uint32_t>> by_pid;  // ascending pattern_id -> its strands in creation order
    for (uint32_t p = 0; p < np; p++) by_pid[P.pats[p].pattern_id].push_back(p);
    char region[48], buf[96];
    // the first seven columns: chrom, region, then bed / inner range / name / pattern_id, or "."
    // for all five (k null: a `hap` line); then haplotype, carriers and kind
    auto head = [&](const InnerKey *k, const Pat *p, uint32_t h, uint32_t carriers, const char *kind) {
        out += chrom;
        out += '\t';
        out += region;
        if (!k) {
            out += "\t.\t.\t.\t.\t.";
        } else {
            out += '\t';
            out += B.beds[k->bed];
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%" PRIu64 "\t%" PRIu64 "\t", k->s, k->e));
            out += p->name;
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u", (unsigned)p->pattern_id));
        }
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%u\t%s", h, carriers, kind));
    };
    size_t at = 0;
    uint32_t prev = 0;
    bool any = false;
    while (at < n) {
        const uint32_t r = recs[at].region;
        if (r >= B.rh.size() || (any && r <= prev)) return fail(TFBS_E_ARG, what + "regions not ascending inside the batch");
        any = true;
        prev = r;
        const RegionH &R = B.rh[r];
        const uint32_t U = R.hap_count, nr = (uint32_t)R.ranges.size();
        const size_t block = (size_t)U * np * nr;
        if (block == 0 || n - at < block) return fail(TFBS_E_ARG, what + "not a whole region");
        const typename Policy::Rec *blk = recs + at;
        size_t x = 0;
        for (uint32_t h = 0; h < U; h++)  // dense and sorted: the block reshapes to [h][p][k]
            for (uint32_t p = 0; p < np; p++)
                for (uint32_t k = 0; k < nr; k++, x++)
                    if (blk[x].region != r || blk[x].haplotype != h || blk[x].pattern != p || blk[x].range != k)
                        return fail(TFBS_E_ARG, what + "not a whole region sorted by (haplotype, pattern, range)");
        at += block;
        snprintf(region, sizeof region, "%" PRIu64 "-%" PRIu64, R.ms, R.me);
        auto val = [&](uint32_t h, const std::vector<uint32_t> &strands, const InnerKey &k) {
            return pol.value_of(blk + (size_t)h * np * nr, strands, nr, (uint32_t)k.slot);
        };
        auto carriers = [&](uint32_t h) { return B.hap_carriers[R.hap_begin + h]; };
        auto line = [&](const InnerKey &k, uint32_t first, uint32_t h, const char *kind, const Value &v, const Value *base) {
            head(&k, &P.pats[first], h, carriers(h), kind);
            out += '\t';
            pol.columns(out, B, first, v, base);
            out += "\t.\n";
        };
        uint32_t base = 0;
        if (diff) {
            std::vector<std::vector<uint32_t>> ids;
            if (int rc = region_baseline(B, R, ids, &base)) return rc;
            for (uint32_t h = 0; h < U; h++) {
                head(nullptr, nullptr, h, carriers(h), "hap");
                out += Policy::hap_dots;
                out += carrier_id_text(B, ids, h, base);
                out += '\n';
            }
        }
        for (const InnerKey &k : R.keys) {  // sorted by (s, e, bed): the rows' order; each once
            if (k.slot < 0) continue;       // an empty inner range
            for (const auto &ps : by_pid) {
                const uint32_t first = ps.second[0];
                if (!diff) {
                    for (uint32_t h = 0; h < U; h++) line(k, first, h, Policy::all_kind, val(h, ps.second, k), nullptr);
                    continue;
                }
                const Value vb = val(base, ps.second, k);
                bool wrote = false;
                for (uint32_t h = 0; h < U; h++) {
                    if (h == base) continue;
                    const Value vh = val(h, ps.second, k);
                    if (!pol.differs(vh, vb)) continue;
                    if (!wrote) line(k, first, base, "base", vb, nullptr);
                    wrote = true;
                    line(k, first, h, "alt", vh, &vb);
                }
            }
        }
    }
    return TFBS_OK;
}

}  // namespace tfbs
