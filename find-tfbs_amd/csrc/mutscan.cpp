// Host side of the mutation scan (include/tfbs_amd.h, "Mutation scan"): the TSV of mutation
// records.
#include <cinttypes>
#include <cstdio>
#include <string>

#include "hits.hpp"

namespace tfbs {
namespace {

const char *const kKindText[5] = {"gain", "loss", "change", "same", "none"};

}  // namespace

int mutscan_tsv(const Batch &B, const tfbs_mutation *m, size_t n, const std::string &chrom, std::string &out) {
    const Patterns &P = *B.pats;
    char buf[256];
    for (size_t k = 0; k < n; k++) {  // one line per record: the records are self-contained
        const tfbs_mutation &x = m[k];
        if (x.region >= B.rh.size() || x.pattern >= P.pats.size() || x.ref > 3 || x.alt > 3 || x.kind > 4)
            return fail(TFBS_E_ARG, "mutation records: a region, pattern, base or kind out of range");
        const RegionH &R = B.rh[x.region];
        const Pat &q = P.pats[x.pattern];
        // chrom region pos ref alt kind name pattern_id strand
        out += chrom;
        out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%" PRIu64 "-%" PRIu64 "\t%" PRIu64 "\t%c\t%c\t%s\t",
                                         (uint64_t)R.ms, (uint64_t)R.me, x.pos, "ACGT"[x.ref], "ACGT"[x.alt],
                                         kKindText[x.kind]));
        out += q.name;
        out.append(buf, (size_t)snprintf(buf, sizeof buf,
                                         "\t%u\t%c\t%" PRIu64 "\t%" PRIu64 "\t%d\t%" PRIu64 "\t%" PRIu64 "\t%d\t%" PRId64 "\n",
                                         (unsigned)q.pattern_id, q.direction == TFBS_DIR_N ? '-' : '+', x.ref_start,
                                         x.ref_end, x.ref_score, x.alt_start, x.alt_end, x.alt_score,
                                         (int64_t)x.alt_score - (int64_t)x.ref_score));
    }
    return TFBS_OK;
}

}  // namespace tfbs

extern "C" {

int tfbs_batch_mutscan_tsv(const tfbs_batch *b, const tfbs_mutation *m, size_t n, const char *chromosome, char **text,
                           size_t *len) {
    if (!b || !chromosome || !text || !len || (n && !m)) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::string out;
    if (int rc = tfbs::mutscan_tsv(b->b, m, n, chromosome, out)) return rc;
    return tfbs::text_out(out, text, len);
}

}  // extern "C"
