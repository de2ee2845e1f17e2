// Host side of the hit lists (include/tfbs_amd.h, "Hit lists"): a region's distinct
// haplotypes and membership read back from the batch, and the TSV of a hit list.
#include "hits.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>

namespace tfbs {

void region_haplotype(const Batch &B, const RegionH &R, uint32_t h, std::vector<uint8_t> &nucs,
                      std::vector<uint64_t> &pos) {
    const DevHap &d = B.haps[R.hap_begin + h];
    nucs.resize(d.len);
    pos.resize(d.len);
    for (uint32_t i = 0; i < d.len; i++) {
        uint8_t c = (B.words[d.word_off + i / 16] >> (2 * (i % 16))) & 3u;
        if ((d.flags & HAP_HAS_N) && ((B.nmask[d.nmask_off + i / 32] >> (i % 32)) & 1u)) c = 4;
        nucs[i] = c;
        pos[i] = R.es + (uint64_t)(int64_t)((d.flags & HAP_HAS_POS) ? B.posrel[d.pos_off + i] : (int32_t)i);
    }
}

namespace {

// out[id] = the distinct index of haplotype id (2 * n_samples entries).
int dense_membership(const Batch &B, const RegionH &R, std::vector<uint32_t> &out) {
    if (int rc = region_membership(B, R)) return rc;
    out.assign(2 * (size_t)B.n_samples, R.ref_local < 0 ? 0u : (uint32_t)R.ref_local);
    for (size_t i = 0; i < R.nonref_id.size(); i++) out[R.nonref_id[i]] = R.nonref_local[i];
    return TFBS_OK;
}

struct Line {
    std::string &out;
    const std::string &chrom;
    char region[48];
    void head(uint32_t h, uint32_t carriers, const char *kind) {
        char buf[64];
        out += chrom;
        out += '\t';
        out += region;
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%u\t%s\t", h, carriers, kind));
    }
    void hap(uint32_t h, uint32_t carriers, const std::string &ids) {
        head(h, carriers, "hap");
        out += ".\t.\t.\t.\t.\t.\t";
        out += ids;
        out += '\n';
    }
    void hit(uint32_t h, uint32_t carriers, const char *kind, const Pat &p, const tfbs_hit &x) {
        char buf[96];
        head(h, carriers, kind);
        out += p.name;
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%c\t%" PRIu64 "\t%" PRIu64 "\t%d\t.\n",
                                         (unsigned)p.pattern_id, p.direction == TFBS_DIR_N ? '-' : '+', x.start, x.end,
                                         x.score));
    }
};

using Key = std::tuple<uint32_t, uint64_t, uint64_t>;  // (pattern, start, end)
inline Key key_of(const tfbs_hit &x) { return Key(x.pattern, x.start, x.end); }

}  // namespace

int region_baseline(const Batch &B, const RegionH &R, std::vector<std::vector<uint32_t>> &ids, uint32_t *base) {
    const uint32_t U = R.hap_count;
    ids.assign(U, {});
    if (B.keep_membership && U) {
        std::vector<uint32_t> memb;
        if (int rc = dense_membership(B, R, memb)) return rc;
        for (uint32_t id = 0; id < memb.size(); id++)
            if (memb[id] < U) ids[memb[id]].push_back(id);
    }
    // the baseline: most carrier ids, ties to the haplotype holding the lowest id
    uint32_t b = 0;
    auto low = [&](uint32_t h) { return ids[h].empty() ? UINT32_MAX : ids[h][0]; };
    for (uint32_t h = 1; h < U; h++) {
        const uint32_t ch = B.hap_carriers[R.hap_begin + h], cb = B.hap_carriers[R.hap_begin + b];
        if (ch > cb || (ch == cb && low(h) < low(b))) b = h;
    }
    *base = b;
    return TFBS_OK;
}

std::string carrier_id_text(const Batch &B, const std::vector<std::vector<uint32_t>> &ids, uint32_t h, uint32_t base) {
    if (h == base) return "*";
    if (!B.keep_membership) return ".";
    std::string out;
    for (size_t k = 0; k < ids[h].size(); k++) {
        if (k) out += ',';
        out += std::to_string(ids[h][k]);
    }
    return out;
}

int hits_tsv(const Batch &B, const tfbs_hit *hits, size_t n, const std::string &chrom, int mode, std::string &out) {
    const Patterns &P = *B.pats;
    for (size_t i = 0; i < n; i++) {
        const tfbs_hit &x = hits[i];
        if (x.region >= B.rh.size() || x.haplotype >= B.rh[x.region].hap_count || x.pattern >= P.pats.size())
            return fail(TFBS_E_ARG, "hit outside the batch");
        if (i && std::make_tuple(hits[i - 1].region, hits[i - 1].haplotype, hits[i - 1].pattern, hits[i - 1].window) >
                     std::make_tuple(x.region, x.haplotype, x.pattern, x.window))
            return fail(TFBS_E_ARG, "hits not sorted by (region, haplotype, pattern, window)");
    }
    Line L{out, chrom, {0}};
    auto set_region = [&](const RegionH &R) { snprintf(L.region, sizeof L.region, "%" PRIu64 "-%" PRIu64, R.ms, R.me); };
    if (mode == TFBS_HITS_ALL) {
        for (size_t i = 0; i < n; i++) {
            const tfbs_hit &x = hits[i];
            if (!i || hits[i - 1].region != x.region) set_region(B.rh[x.region]);
            L.hit(x.haplotype, B.hap_carriers[B.rh[x.region].hap_begin + x.haplotype], "hit", P.pats[x.pattern], x);
        }
        return TFBS_OK;
    }
    if (mode != TFBS_HITS_DIFF) return fail(TFBS_E_ARG, "hits mode is TFBS_HITS_ALL or TFBS_HITS_DIFF");
    size_t at = 0;
    for (size_t r = 0; r < B.rh.size(); r++) {
        const RegionH &R = B.rh[r];
        set_region(R);
        const uint32_t U = R.hap_count;
        // each haplotype's hits [first[h], first[h + 1]) and ascending carrier ids
        std::vector<size_t> first(U + 1, at);
        for (uint32_t h = 0; h < U; h++) {
            first[h] = at;
            while (at < n && hits[at].region == r && hits[at].haplotype == h) at++;
        }
        first[U] = at;
        if (at < n && hits[at].region == r) return fail(TFBS_E_ARG, "hits not sorted by (region, haplotype, pattern, window)");
        std::vector<std::vector<uint32_t>> ids;
        uint32_t base = 0;
        if (int rc = region_baseline(B, R, ids, &base)) return rc;
        std::map<Key, uint32_t> nb;  // the baseline's hits per key
        if (U)
            for (size_t i = first[base]; i < first[base + 1]; i++) nb[key_of(hits[i])]++;
        for (uint32_t h = 0; h < U; h++) {
            const uint32_t car = B.hap_carriers[R.hap_begin + h];
            L.hap(h, car, carrier_id_text(B, ids, h, base));
            if (h == base) {
                for (size_t i = first[h]; i < first[h + 1]; i++) L.hit(h, car, "base", P.pats[hits[i].pattern], hits[i]);
                continue;
            }
            std::map<Key, uint32_t> nh, seen;
            for (size_t i = first[h]; i < first[h + 1]; i++) nh[key_of(hits[i])]++;
            for (size_t i = first[h]; i < first[h + 1]; i++) {  // the last n_h - n_b under a key are gains
                const Key k = key_of(hits[i]);
                const auto it = nb.find(k);
                if (seen[k]++ >= (it == nb.end() ? 0u : it->second)) L.hit(h, car, "gain", P.pats[hits[i].pattern], hits[i]);
            }
            seen.clear();
            for (size_t i = first[base]; i < first[base + 1]; i++) {  // the last n_b - n_h of the baseline's are losses
                const Key k = key_of(hits[i]);
                const auto it = nh.find(k);
                if (seen[k]++ >= (it == nh.end() ? 0u : it->second)) L.hit(h, car, "loss", P.pats[hits[i].pattern], hits[i]);
            }
        }
    }
    if (at != n) return fail(TFBS_E_ARG, "hits not sorted by (region, haplotype, pattern, window)");
    return TFBS_OK;
}

int text_out(const std::string &s, char **text, size_t *len) {
    char *p = (char *)malloc(s.size() + 1);
    if (!p) return fail(TFBS_E_NOMEM, "malloc");
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    *text = p;
    *len = s.size();
    return TFBS_OK;
}

}  // namespace tfbs

extern "C" {

int tfbs_batch_region_haplotype(const tfbs_batch *b, size_t region, uint32_t h, uint8_t *nucs, uint64_t *pos,
                                size_t cap, size_t *n, uint32_t *carriers) {
    if (!b || !n) return tfbs::fail(TFBS_E_ARG, "null argument");
    const tfbs::Batch &B = b->b;
    if (region >= B.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region");
    const tfbs::RegionH &R = B.rh[region];
    if (h >= R.hap_count) return tfbs::fail(TFBS_E_ARG, "bad haplotype index");
    const uint32_t len = B.haps[R.hap_begin + h].len;
    *n = len;
    if (carriers) *carriers = B.hap_carriers[R.hap_begin + h];
    if (cap < len) return tfbs::fail(TFBS_E_ARG, "output capacity too small");
    if (len && (!nucs || !pos)) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::vector<uint8_t> c;
    std::vector<uint64_t> p;
    tfbs::region_haplotype(B, R, h, c, p);
    if (len) {
        memcpy(nucs, c.data(), len);
        memcpy(pos, p.data(), 8 * (size_t)len);
    }
    return TFBS_OK;
}

int tfbs_batch_region_membership(const tfbs_batch *b, size_t region, uint32_t *out) {
    if (!b || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    const tfbs::Batch &B = b->b;
    if (region >= B.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region");
    if (!B.keep_membership) return tfbs::fail(TFBS_E_STATE, "batch created without membership");
    std::vector<uint32_t> m;
    if (int rc = tfbs::dense_membership(B, B.rh[region], m)) return rc;
    if (!m.empty()) memcpy(out, m.data(), 4 * m.size());
    return TFBS_OK;
}

int tfbs_batch_hits_tsv(const tfbs_batch *b, const tfbs_hit *hits, size_t n, const char *chromosome, int mode,
                        char **text, size_t *len) {
    if (!b || !chromosome || !text || !len || (n && !hits)) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::string out;
    if (int rc = tfbs::hits_tsv(b->b, hits, n, chromosome, mode, out)) return rc;
    return tfbs::text_out(out, text, len);
}

}  // extern "C"
