// File-format entry points (f2-f4), for tests and embedding: the BCF reader, the FASTA fetch,
// BGZF files and the merge of ranges through the C API.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "io.hpp"
#include "tfbs_internal.hpp"

extern "C" {

struct tfbs_bcf {
    tfbs::Bcf b;
    std::vector<const tfbs::BcfRecord *> cur;
};

int tfbs_bcf_open(const char *path, tfbs_bcf **out) {
    if (!path || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    auto *b = new tfbs_bcf();
    int rc = b->b.open(path);
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return TFBS_OK;
}
void tfbs_bcf_close(tfbs_bcf *b) { delete b; }
int tfbs_bcf_select(tfbs_bcf *b, const size_t *idx, size_t n) {
    if (!b || (n && !idx)) return tfbs::fail(TFBS_E_ARG, "null argument");
    b->cur.clear();
    return b->b.select(std::vector<size_t>(idx, idx + n));
}
size_t tfbs_bcf_num_samples(const tfbs_bcf *b) { return b ? b->b.samples.size() : 0; }
int tfbs_bcf_indexed(const tfbs_bcf *b) { return b && b->b.indexed() ? 1 : 0; }
const char *tfbs_bcf_sample_name(const tfbs_bcf *b, size_t i) {
    return (b && i < b->b.samples.size()) ? b->b.samples[i].c_str() : nullptr;
}
int tfbs_bcf_fetch(tfbs_bcf *b, const char *chrom, uint64_t beg, uint64_t end, size_t *n) {
    if (!b || !chrom || !n) return tfbs::fail(TFBS_E_ARG, "null argument");
    const int rid = b->b.contig_index(chrom);
    if (rid < 0) return tfbs::fail(TFBS_E_ARG, std::string("unknown contig ") + chrom);
    const int rc = b->b.fetch(rid, beg, end, b->cur);
    if (rc) return rc;
    *n = b->cur.size();
    return TFBS_OK;
}
int tfbs_bcf_record(const tfbs_bcf *b, size_t i, uint64_t *pos, uint32_t *rlen, uint32_t *n_alleles, const char **ref,
                    const char **alt, const int32_t **gt) {
    if (!b || i >= b->cur.size()) return tfbs::fail(TFBS_E_ARG, "bad record index");
    const tfbs::BcfRecord *r = b->cur[i];
    if (pos) *pos = r->pos;
    if (rlen) *rlen = r->rlen;
    if (n_alleles) *n_alleles = r->n_alleles;
    if (ref) *ref = r->ref.c_str();
    if (alt) *alt = r->n_alleles >= 2 ? r->alt.c_str() : nullptr;
    if (gt) *gt = r->gt.empty() ? nullptr : r->gt.data();
    return TFBS_OK;
}

int tfbs_bcf_set_carriers_mode(tfbs_bcf *b, int on) {
    if (!b) return tfbs::fail(TFBS_E_ARG, "null argument");
    b->cur.clear();
    return b->b.set_carriers_mode(on != 0);
}
int tfbs_bcf_record_carriers(const tfbs_bcf *b, size_t i, const uint32_t **ids, size_t *n, int *gt_status) {
    if (!b || i >= b->cur.size()) return tfbs::fail(TFBS_E_ARG, "bad record index");
    const tfbs::BcfRecord *r = b->cur[i];
    if (ids) *ids = r->carriers.data();
    if (n) *n = r->carriers.size();
    if (gt_status) *gt_status = r->gt_status;
    return TFBS_OK;
}

int tfbs_fasta_fetch(const char *path, const char *chrom, uint64_t start, uint64_t stop, char **out, size_t *n) {
    if (!path || !chrom || !out || !n) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::Fasta f;
    int rc = f.open(path);
    if (rc) return rc;
    std::string s;
    rc = f.fetch(chrom, start, stop, s);
    if (rc) return rc;
    char *p = (char *)malloc(s.size() + 1);
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    *out = p;
    *n = s.size();
    return TFBS_OK;
}

int tfbs_bgzf_write_file(const char *path, const char *text, size_t n, int flushes) {
    if (!path || (n && !text)) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::BgzfWriter w;
    int rc = w.open(path);
    if (!rc) rc = w.write(text, n);
    for (int i = 0; !rc && i < flushes; i++) rc = w.flush();
    if (!rc) rc = w.close();
    return rc;
}

int tfbs_bgzf_read_file(const char *path, char **out, size_t *n) {
    if (!path || !out || !n) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::ifstream in(path, std::ios::binary);
    if (!in) return tfbs::fail(TFBS_E_IO, std::string("Could not open file ") + path);
    std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>()), txt;
    int rc = tfbs::bgzf_inflate(raw, txt);
    if (rc) return rc;
    char *p = (char *)malloc(txt.size() + 1);
    memcpy(p, txt.data(), txt.size());
    p[txt.size()] = 0;
    *out = p;
    *n = txt.size();
    return TFBS_OK;
}

int tfbs_merge_ranges(const uint64_t *starts, const uint64_t *ends, size_t n, uint64_t *out_s, uint64_t *out_e,
                      size_t *n_out) {
    if (!n_out || (n && (!starts || !ends || !out_s || !out_e))) return tfbs::fail(TFBS_E_ARG, "null argument");
    std::vector<std::pair<uint64_t, uint64_t>> r(n);
    for (size_t i = 0; i < n; i++) r[i] = {starts[i], ends[i]};
    auto m = tfbs::merge_ranges(r);
    for (size_t i = 0; i < m.size(); i++) {
        out_s[i] = m[i].first;
        out_e[i] = m[i].second;
    }
    *n_out = m.size();
    return TFBS_OK;
}

}  // extern "C"
