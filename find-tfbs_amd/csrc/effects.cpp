// Host side of the variant effects (include/tfbs_amd.h, "Variant effects"): the TSV of
// effect records.
#include <cinttypes>
#include <cstdio>
#include <string>

#include "hits.hpp"

namespace tfbs {
namespace {

const char *const kStatusText[4] = {"scored", "multiallelic", "no_carrier", "unpatched"};

std::string allele_text(const std::vector<uint8_t> &codes) {
    std::string s;
    for (uint8_t c : codes) s += "ACGTN"[c < 5 ? c : 4];
    return s.empty() ? "." : s;
}

// A side's three fields (start, end, score), or "." each for a side without a window.
void side_text(std::string &out, uint32_t n, uint64_t start, uint64_t end, int32_t score) {
    char buf[96];
    if (n) out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%" PRIu64 "\t%" PRIu64 "\t%d", start, end, score));
    else out += "\t.\t.\t.";
}

}  // namespace

int effects_tsv(const Batch &B, const tfbs_effect *e, size_t n, const std::string &chrom, int mode, std::string &out) {
    if (mode != TFBS_EFFECTS_SITES && mode != TFBS_EFFECTS_ALL)
        return fail(TFBS_E_ARG, "effects mode is TFBS_EFFECTS_SITES or TFBS_EFFECTS_ALL");
    if (!B.keep_variants) return fail(TFBS_E_STATE, "batch built without tfbs_batch_keep_variants");
    const Patterns &P = *B.pats;
    const uint32_t np = (uint32_t)P.pats.size();
    size_t at = 0;
    uint32_t prev = 0;
    bool any = false;
    char buf[160];
    while (at < n) {
        const uint32_t r = e[at].region;
        if (r >= B.kept.size() || (any && r <= prev))
            return fail(TFBS_E_ARG, "effect records: regions not ascending inside the batch");
        any = true;
        prev = r;
        const RegionH &R = B.rh[r];
        const KeptRegion &K = B.kept[r];
        const size_t block = K.vars.size() * np;
        if (block == 0 || n - at < block) return fail(TFBS_E_ARG, "effect records: not a whole region");
        const tfbs_effect *x = e + at;
        at += block;
        const std::string head = chrom + '\t' + std::to_string(R.ms) + '-' + std::to_string(R.me) + '\t';
        for (uint32_t v = 0; v < K.vars.size(); v++) {
            const KeptVariant &kv = K.vars[v];
            // chrom region variant pos ref alt carriers
            std::string var = head;
            var.append(buf, (size_t)snprintf(buf, sizeof buf, "%u\t%" PRIu64 "\t", v, kv.pos));
            var += allele_text(kv.ref) + '\t' + allele_text(kv.alt);
            var.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t", kv.carriers));
            out += var;
            out += "var\t";
            out += kStatusText[kv.status < 4 ? kv.status : 3];
            out += "\t.\t.\t.\t.\t.\t.\t.\t.\t.\n";
            for (uint32_t p = 0; p < np; p++, x++) {  // dense and sorted: the block reshapes to [v][p]
                if (x->region != r || x->variant != v || x->pattern != p || x->status != kv.status)
                    return fail(TFBS_E_ARG, "effect records: not a whole region sorted by (variant, pattern)");
                if (kv.status != TFBS_VAR_SCORED || x->n_ref + (uint64_t)x->n_alt == 0) continue;
                const Pat &q = P.pats[p];
                const bool pr = x->n_ref && x->ref_score > q.min_score, pa = x->n_alt && x->alt_score > q.min_score;
                const char *kind = pa && !pr ? "gain"
                                   : pr && !pa ? "loss"
                                   : !pr       ? "none"
                                   : x->ref_score != x->alt_score ? "change" : "same";
                if (mode == TFBS_EFFECTS_SITES && (kind[0] == 'n' || kind[0] == 's')) continue;
                out += var;
                out += kind;
                out += '\t';
                out += q.name;
                out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%c", (unsigned)q.pattern_id,
                                                 q.direction == TFBS_DIR_N ? '-' : '+'));
                side_text(out, x->n_ref, x->ref_start, x->ref_end, x->ref_score);
                side_text(out, x->n_alt, x->alt_start, x->alt_end, x->alt_score);
                if (x->n_ref && x->n_alt)
                    out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%" PRId64 "\n",
                                                     (int64_t)x->alt_score - (int64_t)x->ref_score));
                else out += "\t.\n";
            }
        }
    }
    return TFBS_OK;
}

}  // namespace tfbs

extern "C" {

int tfbs_batch_effects_tsv(const tfbs_batch *b, const tfbs_effect *e, size_t n, const char *chromosome, int mode,
                           char **text, size_t *len) {
    if (!b || !chromosome || !text || !len || (n && !e)) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::string out;
    if (int rc = tfbs::effects_tsv(b->b, e, n, chromosome, mode, out)) return rc;
    return tfbs::text_out(out, text, len);
}

}  // extern "C"
