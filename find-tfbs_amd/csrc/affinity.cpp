// Host side of the binding affinity (include/tfbs_amd.h, "Binding affinity"): the weight
// a(d) from the committed tables, the pattern_ids' reference scores and the TSV of affinity
// records.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "affinity_log_table.hpp"
#include "affinity_rows.hpp"
#include "affinity_tables.hpp"
#include "key_tsv.hpp"
#include "score_dist.hpp"

namespace tfbs {

uint64_t affinity_weight(uint64_t d) {
    if (d > kAffLast) return 0;
    return (uint64_t)(((unsigned __int128)kAffT1[d % 1000] * kAffT2[d / 1000]) >> 64) >> 22;
}

int affinity_tops(const Patterns &P, std::vector<int32_t> *tops) {
    std::map<uint16_t, int64_t> top;  // per pattern_id
    for (const Pat &p : P.pats) {
        if (p.kind != TFBS_KIND_PWM && p.kind != TFBS_KIND_DIPWM) continue;
        const bool di = p.kind == TFBS_KIND_DIPWM;
        const uint32_t steps = di ? (p.len ? p.len - 1 : 0) : p.len, width = di ? 16 : 4;
        const int32_t *w = di ? p.w16.data() : p.w5.data();
        const size_t stride = di ? 16 : 5;
        uint64_t mag = 0;
        int64_t c = 0;
        for (uint32_t j = 0; j < steps; j++) {
            const int32_t *col = w + stride * j;
            const int64_t lo = *std::min_element(col, col + width), hi = *std::max_element(col, col + width);
            mag += (uint64_t)std::max(std::llabs(lo), std::llabs(hi));
            if (mag > (uint64_t)INT32_MAX)
                return fail(TFBS_E_ARG, "the scores of strand " + strand_label(p) + " can wrap int32");
            c += std::max<int64_t>(0, hi);
        }
        int64_t &t = top[p.pattern_id];  // (0 at first: no strand's sum is below it)
        t = std::max(t, c);
    }
    tops->clear();
    for (const Pat &p : P.pats)
        tops->push_back(p.kind == TFBS_KIND_PWM || p.kind == TFBS_KIND_DIPWM ? (int32_t)top[p.pattern_id] : 0);
    return TFBS_OK;
}

uint32_t affinity_max_strands(const Patterns &P) {
    std::map<uint16_t, uint32_t> n;
    uint32_t most = 0;
    for (const Pat &p : P.pats) most = std::max(most, ++n[p.pattern_id]);
    return most;
}

int32_t affinity_mlog2_host(uint64_t x) { return affinity_mlog2(x, kAffLogP); }

std::string affinity_row_info(int64_t lo, int64_t hi, uint64_t xlo, uint64_t xhi, int32_t top, uint64_t zero,
                              uint64_t one, uint64_t two) {
    char buf[224];
    const int m = snprintf(buf, sizeof buf,
                           "LOG2AFF=%" PRId64 ",%" PRId64 ";AFF=%" PRIu64 ",%" PRIu64 ";TOP=%d;freqs=%" PRIu64 "/%" PRIu64
                           "/%" PRIu64,
                           lo, hi, xlo, xhi, top, zero, one, two);
    return std::string(buf, (size_t)m);
}

bool affinity_as_genotypes(const uint64_t *left, const uint64_t *right, size_t n, int32_t top, uint64_t min_spread,
                           uint32_t *maf, std::string &info, std::string &gts) {
    if (n == 0) return false;
    uint64_t xlo = left[0] + right[0], xhi = xlo;  // (each below 2^63: no wrap)
    for (size_t i = 1; i < n; i++) {
        const uint64_t x = left[i] + right[i];
        xlo = std::min(xlo, x);
        xhi = std::max(xhi, x);
    }
    const int64_t lo = affinity_mlog2_host(xlo), hi = affinity_mlog2_host(xhi);  // (mlog2 is monotone)
    const uint64_t spread = (uint64_t)(hi - lo);
    if (spread == 0 || spread < min_spread) return false;
    uint64_t cnt[3] = {0, 0, 0};
    gts.reserve(gts.size() + n * 11);
    for (size_t i = 0; i < n; i++)
        append_row_field(gts, (uint64_t)((int64_t)affinity_mlog2_host(left[i] + right[i]) - lo), spread, cnt);
    *maf = (uint32_t)maf_of(cnt[0], cnt[1], cnt[2]);
    info += affinity_row_info(lo, hi, xlo, xhi, top, cnt[0], cnt[1], cnt[2]);
    return true;
}

namespace {

struct AffinityPolicy {
    using Rec = tfbs_affinity;
    struct Value {  // the sums over the pattern_id's strands
        uint64_t a = 0, n = 0;
        bool none() const { return n == 0; }
    };
    static constexpr const char *word = "affinity", *all_kind = "aff", *hap_dots = "\t.\t.\t.\t.\t";
    std::vector<int32_t> tops;
    Value value_of(const tfbs_affinity *hap_block, const std::vector<uint32_t> &strands, uint32_t nr, uint32_t slot) const {
        Value v;
        for (uint32_t p : strands) {
            const tfbs_affinity &x = hap_block[(size_t)p * nr + slot];
            v.a += x.sum;
            v.n += x.n_windows;
        }
        return v;
    }
    bool differs(const Value &a, const Value &b) const { return a.none() != b.none() || a.a != b.a; }
    void columns(std::string &out, const Batch &, uint32_t first, const Value &v, const Value *base) const {
        char buf[96];
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "%d\t", tops[first]));
        if (!v.none()) out.append(buf, (size_t)snprintf(buf, sizeof buf, "%" PRIu64 "\t%" PRIu64 "\t", v.n, v.a));
        else out += ".\t.\t";
        if (base && !v.none() && !base->none())
            out.append(buf, (size_t)snprintf(buf, sizeof buf, "%" PRId64, (int64_t)(v.a - base->a)));
        else out += '.';
    }
};

}  // namespace

int affinity_tsv(const Batch &B, const tfbs_affinity *aff, size_t n, const std::string &chrom, int mode,
                 std::string &out) {
    if (mode != TFBS_AFFINITY_ALL && mode != TFBS_AFFINITY_DIFF)
        return fail(TFBS_E_ARG, "affinity mode is TFBS_AFFINITY_ALL or TFBS_AFFINITY_DIFF");
    AffinityPolicy pol;
    if (int rc = affinity_tops(*B.pats, &pol.tops)) return rc;
    return key_tsv(pol, B, aff, n, chrom, mode == TFBS_AFFINITY_DIFF, out);
}

}  // namespace tfbs

extern "C" {

uint64_t tfbs_affinity_weight(uint64_t d) { return tfbs::affinity_weight(d); }

int tfbs_patterns_affinity_tops(const tfbs_patterns *p, int32_t *out) {
    if (!p || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::vector<int32_t> tops;
    if (int rc = tfbs::affinity_tops(tfbs::patterns_of(p), &tops)) return rc;
    std::copy(tops.begin(), tops.end(), out);
    return TFBS_OK;
}

int tfbs_affinity_mlog2(const uint64_t *x, size_t n, int device, int32_t *out) {
    if (n && (!x || !out)) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (device < -1) return tfbs::fail(TFBS_E_ARG, "device is -1 (the host) or a HIP device");
    if (device >= 0) return tfbs::affinity_mlog2_device(x, n, device, out);
    for (size_t i = 0; i < n; i++) out[i] = tfbs::affinity_mlog2_host(x[i]);
    return TFBS_OK;
}

int tfbs_affinity_as_genotypes(const uint64_t *left, const uint64_t *right, size_t n, int32_t top, uint64_t min_spread,
                               uint32_t *maf, char *info, size_t info_cap, char *genotypes, size_t gt_cap) {
    if (!maf || (n && (!left || !right))) return tfbs::fail(TFBS_E_ARG, "null argument");
    for (size_t i = 0; i < n; i++)
        if ((left[i] | right[i]) >> 63) return tfbs::fail(TFBS_E_ARG, "an affinity sum of 2^63 or more");
    std::string a, g;
    if (!tfbs::affinity_as_genotypes(left, right, n, top, min_spread, maf, a, g)) return 0;
    if (!info || !genotypes || a.size() + 1 > info_cap || g.size() + 1 > gt_cap)
        return tfbs::fail(TFBS_E_ARG, "output capacity too small");
    memcpy(info, a.c_str(), a.size() + 1);
    memcpy(genotypes, g.c_str(), g.size() + 1);
    return 1;
}

int tfbs_batch_affinity_tsv(const tfbs_batch *b, const tfbs_affinity *aff, size_t n, const char *chromosome,
                            int mode, char **text, size_t *len) {
    if (!b || !chromosome || !text || !len || (n && !aff)) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::string out;
    if (int rc = tfbs::affinity_tsv(b->b, aff, n, chromosome, mode, out)) return rc;
    return tfbs::text_out(out, text, len);
}

}  // extern "C"
