// The entry points of the hit lists, best sites, affinities, score rows, affinity rows, variant effects and mutation
// scans: the resident image handed to their drivers (scan_hits.hip, scan_best.hip, scan_affinity.hip, score_rows.hip,
// affinity_rows.hip); the last two
// (scan_effects.hip, scan_mutscan.hip) read the batch's kept variants instead.
#include "ctx.hpp"

using namespace tfbs;

// A result list handed out through the C API: *out a malloc'd copy (never null), *n its length.
template <typename T>
static int hand_out(const std::vector<T> &v, T **out, size_t *n) {
    T *p = static_cast<T *>(malloc(std::max<size_t>(1, v.size()) * sizeof(T)));
    if (!p) return tfbs::fail(TFBS_E_NOMEM, "malloc");
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    *out = p;
    *n = v.size();
    return TFBS_OK;
}

extern "C" {

// Hit lists and best sites (scan_hits.hip, scan_best.hip): a call's arguments checked (null_out:
// the entry point's own null rule), then *img.
static int resident_image(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, bool null_out, ScanImage *img) {
    if (!ctx || !b || null_out) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not resident on this ctx (tfbs_batch_upload)");
    if (r0 > r1 || r1 > b->b.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region range");
    if (b->b.haps.size() != ctx->img.haps.n) return tfbs::fail(TFBS_E_STATE, "regions added since the upload");
    *img = ScanImage{ctx->img.haps.p, ctx->img.words.p, ctx->img.nmask.p, ctx->img.posrel.p, ctx->img.regions.p, ctx->img.inner.p};
    return TFBS_OK;
}

int tfbs_batch_hits(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_hit **out, size_t *n) {
    ScanImage img;
    std::vector<tfbs_hit> v;
    if (int rc = resident_image(ctx, b, r0, r1, !out || !n, &img)) return rc;
    if (int rc = hits_run(&ctx->hits_state, ctx->device, ctx->stream, *ctx->pats, img, b->b, r0, r1, &v, nullptr))
        return rc;
    return hand_out(v, out, n);
}

int tfbs_batch_hits_count(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint64_t *per_region) {
    ScanImage img;
    if (int rc = resident_image(ctx, b, r0, r1, !per_region && r1 > r0, &img)) return rc;
    return hits_run(&ctx->hits_state, ctx->device, ctx->stream, *ctx->pats, img, b->b, r0, r1, nullptr, per_region);
}

int tfbs_ctx_last_hits_ms(const tfbs_ctx *ctx, double out[4]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    hits_last_ms(ctx->hits_state, out);
    return TFBS_OK;
}

int tfbs_batch_best(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_best **out, size_t *n) {
    ScanImage img;
    std::vector<tfbs_best> v;
    if (int rc = resident_image(ctx, b, r0, r1, !out || !n, &img)) return rc;
    if (int rc = best_run(&ctx->best_state, ctx->device, ctx->stream, *ctx->pats, img, b->b, r0, r1, &v)) return rc;
    return hand_out(v, out, n);
}

int tfbs_ctx_last_best_ms(const tfbs_ctx *ctx, double out[2]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    best_last_ms(ctx->best_state, out);
    return TFBS_OK;
}

// Binding affinity (scan_affinity.hip): as the best sites, the batch resident and no scan needed.
int tfbs_batch_affinity(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_affinity **out, size_t *n) {
    ScanImage img;
    std::vector<tfbs_affinity> v;
    if (ctx && b && b->b.pats != ctx->pats) return tfbs::fail(TFBS_E_ARG, "batch and ctx use different pattern sets");
    if (int rc = resident_image(ctx, b, r0, r1, !out || !n, &img)) return rc;
    if (int rc = affinity_run(&ctx->affinity_state, ctx->device, ctx->stream, *ctx->pats, img, b->b, r0, r1, &v)) return rc;
    return hand_out(v, out, n);
}

int tfbs_ctx_last_affinity_ms(const tfbs_ctx *ctx, double out[2]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    affinity_last_ms(ctx->affinity_state, out);
    return TFBS_OK;
}

// Score rows (score_rows.hip): the batch resident here and made with membership; no scan needed.
int tfbs_batch_score_rows(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome,
                          uint32_t min_maf, uint64_t min_spread, uint32_t *fake_position, char **text, size_t *len,
                          uint64_t *n_rows) {
    ScanImage img;
    if (int rc = resident_image(ctx, b, r0, r1, !chromosome || !n_rows || (text && (!len || !fake_position)), &img))
        return rc;
    if (!b->b.keep_membership) return tfbs::fail(TFBS_E_STATE, "batch created without membership");
    std::string out;
    uint32_t fake = fake_position ? *fake_position : 1;
    if (int rc = scores_run(&ctx->scores_state, &ctx->best_state, ctx->device, ctx->stream, *ctx->pats, img, b->b, r0, r1,
                            tfbs::strip_chr(chromosome), min_maf, min_spread, &fake, text ? &out : nullptr, n_rows))
        return rc;
    if (!text) return TFBS_OK;
    if (int rc = tfbs::text_out(out, text, len)) return rc;
    *fake_position = fake;
    return TFBS_OK;
}

int tfbs_ctx_last_scores_ms(const tfbs_ctx *ctx, double out[4]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    scores_last_ms(ctx->scores_state, out);
    return TFBS_OK;
}

// Affinity rows (affinity_rows.hip): as the score rows; the pattern set checked as the affinity call's.
int tfbs_batch_affinity_rows(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome,
                             uint32_t min_maf, uint64_t min_spread, uint32_t *fake_position, char **text, size_t *len,
                             uint64_t *n_rows) {
    ScanImage img;
    if (ctx && b && b->b.pats != ctx->pats) return tfbs::fail(TFBS_E_ARG, "batch and ctx use different pattern sets");
    if (int rc = resident_image(ctx, b, r0, r1, !chromosome || !n_rows || (text && (!len || !fake_position)), &img))
        return rc;
    if (!b->b.keep_membership) return tfbs::fail(TFBS_E_STATE, "batch created without membership");
    std::string out;
    uint32_t fake = fake_position ? *fake_position : 1;
    if (int rc = affinity_rows_run(&ctx->affinity_rows_state, &ctx->scores_state, &ctx->affinity_state, ctx->device,
                                   ctx->stream, *ctx->pats, img, b->b, r0, r1, tfbs::strip_chr(chromosome), min_maf,
                                   min_spread, &fake, text ? &out : nullptr, n_rows))
        return rc;
    if (!text) return TFBS_OK;
    if (int rc = tfbs::text_out(out, text, len)) return rc;
    *fake_position = fake;
    return TFBS_OK;
}

int tfbs_ctx_last_affinity_rows_ms(const tfbs_ctx *ctx, double out[4]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    affinity_rows_last_ms(ctx->affinity_rows_state, out);
    return TFBS_OK;
}

// Variant effects (scan_effects.hip): the batch need not be resident, only of the ctx's patterns.
int tfbs_batch_effects(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_effect **out, size_t *n) {
    if (!ctx || !b || !out || !n) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (b->b.pats != ctx->pats) return tfbs::fail(TFBS_E_ARG, "batch and ctx use different pattern sets");
    if (!b->b.keep_variants) return tfbs::fail(TFBS_E_STATE, "batch built without tfbs_batch_keep_variants");
    if (b->b.open) return tfbs::fail(TFBS_E_STATE, "region still open");
    if (r0 > r1 || r1 > b->b.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region range");
    std::vector<tfbs_effect> v;
    if (int rc = effects_run(&ctx->effects_state, ctx->device, ctx->stream, *ctx->pats, b->b, r0, r1, &v)) return rc;
    return hand_out(v, out, n);
}

int tfbs_ctx_last_effects_ms(const tfbs_ctx *ctx, double out[3]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    effects_last_ms(ctx->effects_state, out);
    return TFBS_OK;
}

// Mutation scan (scan_mutscan.hip): as the variant effects, the batch need not be resident.
static int mutscan_call(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint32_t kinds, bool null_out,
                        std::vector<tfbs_mutation> *v, uint64_t *total) {
    if (!ctx || !b || null_out) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (b->b.pats != ctx->pats) return tfbs::fail(TFBS_E_ARG, "batch and ctx use different pattern sets");
    if (!b->b.keep_variants) return tfbs::fail(TFBS_E_STATE, "batch built without tfbs_batch_keep_variants");
    if (b->b.open) return tfbs::fail(TFBS_E_STATE, "region still open");
    if (r0 > r1 || r1 > b->b.rh.size()) return tfbs::fail(TFBS_E_ARG, "bad region range");
    if (kinds == 0 || kinds > TFBS_MUT_ALL) return tfbs::fail(TFBS_E_ARG, "kinds is a non-empty mask of TFBS_MUT_*");
    return mutscan_run(&ctx->mutscan_state, ctx->device, ctx->stream, *ctx->pats, b->b, r0, r1, kinds, v, total);
}

int tfbs_batch_mutscan(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint32_t kinds, tfbs_mutation **out,
                       size_t *n) {
    std::vector<tfbs_mutation> v;
    uint64_t total = 0;
    if (int rc = mutscan_call(ctx, b, r0, r1, kinds, !out || !n, &v, &total)) return rc;
    if (total != v.size()) return tfbs::fail(TFBS_E_STATE, "mutation scan: the count and the fill disagree");
    return hand_out(v, out, n);
}

int tfbs_batch_mutscan_count(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint32_t kinds, uint64_t *n) {
    return mutscan_call(ctx, b, r0, r1, kinds, !n, nullptr, n);
}

int tfbs_ctx_last_mutscan_ms(const tfbs_ctx *ctx, double out[4]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    mutscan_last_ms(ctx->mutscan_state, out);
    return TFBS_OK;
}

uint32_t tfbs_mutscan_ring_max_length(void) { return tfbs::kMutRingMax; }


}  // extern "C"
