// MI355X (gfx950) variant-effect kernel: per (scored record, pattern strand) the best score
// among the windows the record touches on the reference sequence R and on the record's own
// sequence A, the lowest window attaining each and the two window counts (include/tfbs_amd.h,
// "Variant effects").  min_score and the inner ranges play no part.
//
// The pair a wave owns, the prologue (pair_head) and the scoring (score_mono<1>,
// score_dinuc<1>) are hit_score.hpp's, shared with scan_hits.hip and scan_best.hip, and so is
// the driver's base (PairState).  This file keeps the windows a wave scores and what it does
// with their scores.
//
//  * The host patches R once per region and A once per scored record, finds their common
//    prefix a and suffix z and packs both into one run of words (and N-mask words), A from a
//    32-base boundary of the run: a lane's side is a constant added to its base index under
//    one wave-uniform W / M.  Each sequence keeps the batch image's pads behind it.
//  * Window i of a side of n bases is affected iff i + L <= n, i + L > a and i < n - z: a
//    range [lo, lo + count) per side.  The wave's windows are R's affected windows followed by
//    A's in one index space, walked in 64-lane chunks: an SNV under a strand of 32 bases or
//    fewer is one chunk.  A lane beyond the last window scores the first one and is masked out.
//  * Per side a butterfly over the lanes takes the maximum of
//    (int64(score) << 32) | (0xFFFFFFFF - window) and the sum of the counts, as the best-site
//    kernel does; a lane without a window of the side holds (INT32_MIN, UINT32_MAX), the lowest
//    key there is.  Lane 0 writes one 32-byte record with two vector stores.
//  * The result is dense: record (chunk record k, strand s) lies at k * n_strands + s.  No
//    atomics, no count pass, no sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hit_score.hpp"
#include "pack_seq.hpp"  // mask_words, pack_seq, has_n, pos_at: shared with scan_mutscan.hip

namespace tfbs {
namespace {

struct EffArgs {
    PairSrc src;  // the tables; words / nmask: the chunk's packed image (haps unused)
    const DevEffVar *vars;
    uint32_t n_vars;
    uint64_t rec_cap;
    DevEffRec *recs;
};

// The affected windows [lo, lo + count) of a side of n bases under a strand of L bases.
__device__ __forceinline__ void affected_windows(uint32_t n, uint32_t L, uint32_t a, uint32_t z, uint32_t &lo,
                                                 uint32_t &count) {
    lo = a + 1 > L ? a + 1 - L : 0;
    const uint32_t hi = n >= L ? min(n - L + 1, n - z) : 0;
    count = hi > lo ? hi - lo : 0;
}

struct EffLane {  // a lane's running best and count on one side
    int32_t score = INT32_MIN;
    uint32_t window = UINT32_MAX, n = 0;
};

// A lane meets its windows of a side in ascending order: a strictly greater score (or the
// first window) replaces its best, so ties stay on the lowest window.
__device__ __forceinline__ void take(EffLane &b, bool mine, int32_t sc, uint32_t i) {
    const bool better = mine && (b.n == 0 || sc > b.score);
    b.score = better ? sc : b.score;
    b.window = better ? i : b.window;
    b.n += mine ? 1u : 0u;
}

__device__ __forceinline__ void reduce(EffLane &b) {
    long long key = (long long)(((unsigned long long)(uint32_t)b.score << 32) | (0xFFFFFFFFu - b.window));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const long long o = __shfl_xor(key, m);
        key = o > key ? o : key;
        b.n += (uint32_t)__shfl_xor((int)b.n, m);
    }
    b.score = (int32_t)(key >> 32);
    b.window = 0xFFFFFFFFu - (uint32_t)key;
}

// Grid: ceil(n_vars * n_strands / kHitWaves) workgroups of kHitBlock threads.
__global__ __launch_bounds__(kHitBlock) void scan_effects_kernel(EffArgs A) {
    __shared__ int32_t s_rows[kHitWaves][kHitDiInts];
    const PairHead H = pair_head(A.src, 0, A.n_vars, s_rows);
    if (!H.active) return;
    const DevEffVar d = A.vars[H.k];
    const bool scored = H.L != 0 && (H.kind == TFBS_KIND_PWM || H.di);
    uint32_t lo_r, n_r, lo_a, n_a;
    affected_windows(d.len_r, H.L, d.a, d.z, lo_r, n_r);
    affected_windows(d.len_a, H.L, d.a, d.z, lo_a, n_a);
    lo_r = __builtin_amdgcn_readfirstlane(lo_r);
    lo_a = __builtin_amdgcn_readfirstlane(lo_a);
    n_r = __builtin_amdgcn_readfirstlane(scored ? n_r : 0u);
    n_a = __builtin_amdgcn_readfirstlane(scored ? n_a : 0u);
    const uint32_t total = n_r + n_a;  // (0: both records' sides are the empty one)
    const PairScan P{A.src.words + d.word_off, d.has_n ? A.src.nmask + d.nmask_off : nullptr,
                     (CInt4 *)(A.src.weights + H.w_off), H.rows, H.L, total, H.di};
    EffLane r, a;
    for (uint32_t c0 = 0; c0 < total; c0 += 64) {
        const uint32_t t = c0 + H.lane;
        const bool exists = t < total;
        const uint32_t te = exists ? t : 0;  // (window 0 of the index space exists: reads stay inside the run)
        const bool alt = te >= n_r;
        const uint32_t i = alt ? lo_a + (te - n_r) : lo_r + te;
        const uint32_t ii[1] = {alt ? d.a_base + i : i};
        uint32_t s[1];
        SCORE_WINDOWS(1, P, ii, s);
        take(r, exists && !alt, (int32_t)s[0], i);
        take(a, exists && alt, (int32_t)s[0], i);
    }
    reduce(r);
    reduce(a);
    if (H.lane == 0 && H.p < A.rec_cap)
        A.recs[H.p] = DevEffRec{r.score, r.window, r.n, 0u, a.score, a.window, a.n, 0u};
}

}  // namespace

struct EffectsState : PairState {  // host: a chunk's image and records
    DevBuf<uint32_t> image;  // the chunk's descriptors, words and N-mask words: one upload
    DevBuf<DevEffRec> recs;
    double ms[3] = {0, 0, 0};
};

void effects_state_destroy(EffectsState *s) { delete s; }

void effects_last_ms(const EffectsState *s, double out[3]) {
    for (int k = 0; k < 3; k++) out[k] = s ? s->ms[k] : 0.0;
}

int effects_run(EffectsState **state, int device, void *stream_, const Patterns &P, const Batch &B, size_t r0,
                size_t r1, std::vector<tfbs_effect> *out) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!B.keep_variants) return fail(TFBS_E_STATE, "batch built without tfbs_batch_keep_variants");
    if (B.kept.size() != B.rh.size()) return fail(TFBS_E_STATE, "kept variants out of step with the regions");
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, stream, 2, "variant-effect tables")) return rc;
    EffectsState &S = **state;
    S.ms[0] = S.ms[1] = S.ms[2] = 0;
    const uint64_t ns = S.n_strands;
    if (ns == 0 || r0 == r1) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, "too many strands for the variant-effect kernel");
    const uint64_t budget = scratch_budget("TFBS_EFFECTS_SCRATCH_MB", 256.0);  // read at the call
    const uint64_t max_vars = std::max<uint64_t>(1, kHitsMaxPairs / ns);
    double t_prep = now_ms();

    // every record's block, unscored ones as they stay; a scored one's is filled by its chunk
    size_t total = out->size();
    const size_t base = total;
    for (size_t r = r0; r < r1; r++) total += B.kept[r].vars.size() * ns;
    out->resize(total);
    {
        size_t at = base;
        for (size_t r = r0; r < r1; r++)
            for (size_t v = 0; v < B.kept[r].vars.size(); v++)
                for (uint32_t p = 0; p < ns; p++, at++)
                    (*out)[at] = tfbs_effect{(uint32_t)r, (uint32_t)v, p, B.kept[r].vars[v].status,
                                             0, INT32_MIN, UINT32_MAX, 0, INT32_MIN, UINT32_MAX, 0, 0, 0, 0};
    }

    struct HostVar {  // a scored record of the chunk
        size_t out_at;     // its block in *out
        uint32_t pos_r;    // its region's R positions in pos_rs
        PosRuns pos_a;
    };
    std::vector<HostVar> hv;
    std::vector<PosRuns> pos_rs;
    std::vector<DevEffVar> vars;
    std::vector<uint32_t> words, nmask, image;
    int rc = TFBS_OK;

    auto flush = [&]() -> int {
        const size_t nv = hv.size();
        if (!nv) return TFBS_OK;
        const uint64_t nrec = nv * ns;
        // one image: the descriptors, then the words, then the N-mask words
        const size_t w0 = nv * (sizeof(DevEffVar) / 4), m0 = w0 + words.size();
        image.resize(m0 + nmask.size());
        memcpy(image.data(), vars.data(), nv * sizeof(DevEffVar));
        if (!words.empty()) memcpy(image.data() + w0, words.data(), 4 * words.size());
        if (!nmask.empty()) memcpy(image.data() + m0, nmask.data(), 4 * nmask.size());
        if ((rc = S.image.ensure_exact(image.size())) || (rc = S.recs.ensure_exact(nrec)) ||
            (rc = S.host.reserve(nrec * sizeof(DevEffRec))))
            return rc;
        S.ms[0] += now_ms() - t_prep;
        HIP_TRY(hipMemcpyAsync(S.image.p, image.data(), 4 * image.size(), hipMemcpyHostToDevice, stream));
        EffArgs A{};
        A.src = PairSrc{S.strands.p, S.weights.p, S.n_strands, nullptr, S.image.p + w0, S.image.p + m0};
        A.vars = reinterpret_cast<const DevEffVar *>(S.image.p);
        A.n_vars = (uint32_t)nv;
        A.rec_cap = nrec;
        A.recs = S.recs.p;
        HIP_TRY(hipEventRecord(S.ev[0], stream));
        hipLaunchKernelGGL(scan_effects_kernel, dim3((uint32_t)((nrec + kHitWaves - 1) / kHitWaves)), dim3(kHitBlock), 0,
                           stream, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(S.ev[1], stream));
        HIP_TRY(hipEventSynchronize(S.ev[1]));  // (the host part's clock starts when the kernel is done)
        const double t0 = now_ms();
        HIP_TRY(hipMemcpyAsync(S.host.p, S.recs.p, nrec * sizeof(DevEffRec), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        S.ms[1] += ms;
        const DevEffRec *q = reinterpret_cast<const DevEffRec *>(S.host.p);
        for (size_t k = 0; k < nv; k++) {
            const PosRuns &pr = pos_rs[hv[k].pos_r], &pa = hv[k].pos_a;
            for (uint32_t p = 0; p < ns; p++, q++) {
                tfbs_effect &o = (*out)[hv[k].out_at + p];
                const uint64_t L = P.pats[p].len;
                o.n_ref = q->n_ref;
                o.ref_score = q->ref_score;
                o.ref_window = q->ref_window;
                o.n_alt = q->n_alt;
                o.alt_score = q->alt_score;
                o.alt_window = q->alt_window;
                if (q->n_ref && q->ref_window < pr.n) o.ref_end = (o.ref_start = pos_at(pr, q->ref_window)) + L - 1;
                if (q->n_alt && q->alt_window < pa.n) o.alt_end = (o.alt_start = pos_at(pa, q->alt_window)) + L - 1;
            }
        }
        hv.clear();
        pos_rs.clear();
        vars.clear();
        words.clear();
        nmask.clear();
        S.ms[2] += now_ms() - t0;
        t_prep = now_ms();
        return TFBS_OK;
    };

    std::vector<uint8_t> nuc_r, nuc_a;
    std::vector<uint64_t> xr, xa;  // the two sequences' positions, expanded
    std::vector<uint32_t> wr, mr;  // R packed once per region
    Record rec;
    std::vector<const Record *> one(1, &rec), none;
    size_t at = base;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        const KeptRegion &K = B.kept[r];
        bool have_r = false, n_in_r = false;
        PosRuns pos_r;
        int32_t slot_r = -1;  // the region's R positions in the chunk's pos_rs
        for (size_t v = 0; v < K.vars.size(); v++, at += ns) {
            const KeptVariant &kv = K.vars[v];
            if (kv.status != TFBS_VAR_SCORED) continue;
            if (!have_r) {
                nuc_r.clear();
                pos_r = PosRuns();
                if ((rc = patch_runs(R.es, R.ee, none, K.ref.data(), R.es, K.ref.size(), nuc_r, pos_r))) return rc;
                xr.resize(pos_r.n);
                pos_r.expand(xr.data(), [](uint64_t p) { return p; });
                n_in_r = has_n(nuc_r);
                wr.resize(2 * (size_t)mask_words(pos_r.n));
                mr.resize(mask_words(pos_r.n));
                pack_seq(nuc_r, wr.data(), mr.data());
                have_r = true;
            }
            rec.pos = kv.pos;
            rec.ref = kv.ref;
            rec.alt = kv.alt;
            nuc_a.clear();
            HostVar h;
            if ((rc = patch_runs(R.es, R.ee, one, K.ref.data(), R.es, K.ref.size(), nuc_a, h.pos_a)))
                return fail(TFBS_E_STATE, "a scored record no longer patches alone");
            xa.resize(h.pos_a.n);
            h.pos_a.expand(xa.data(), [](uint64_t p) { return p; });
            const uint32_t nr = pos_r.n, na = h.pos_a.n, lim = std::min(nr, na);
            uint32_t a = 0, z = 0;
            while (a < lim && nuc_r[a] == nuc_a[a] && xr[a] == xa[a]) a++;
            while (z < lim - a && nuc_r[nr - 1 - z] == nuc_a[na - 1 - z] && xr[nr - 1 - z] == xa[na - 1 - z]) z++;
            const bool any_n = n_in_r || has_n(nuc_a);
            const size_t w_add = 2 * ((size_t)mask_words(nr) + mask_words(na)), m_add = any_n ? w_add / 2 : 0;
            const uint64_t add = 4 * (w_add + m_add) + sizeof(DevEffVar) + ns * sizeof(DevEffRec);
            const uint64_t used = 4 * (words.size() + nmask.size()) + hv.size() * (sizeof(DevEffVar) + ns * sizeof(DevEffRec));
            if (!hv.empty() && (used + add > budget || hv.size() >= max_vars || words.size() + w_add > (1ull << 31))) {
                if ((rc = flush())) return rc;
                slot_r = -1;
            }
            if (slot_r < 0) {
                slot_r = (int32_t)pos_rs.size();
                pos_rs.push_back(pos_r);
            }
            DevEffVar d{};
            d.word_off = (uint32_t)words.size();
            d.nmask_off = (uint32_t)nmask.size();
            d.len_r = nr;
            d.len_a = na;
            d.a = a;
            d.z = z;
            d.a_base = 32 * mask_words(nr);
            d.has_n = any_n ? 1u : 0u;
            words.resize(words.size() + w_add);
            uint32_t *w = words.data() + d.word_off, *m = nullptr;
            if (any_n) {
                nmask.resize(nmask.size() + m_add);
                m = nmask.data() + d.nmask_off;
                memcpy(m, mr.data(), 4 * mr.size());
            }
            memcpy(w, wr.data(), 4 * wr.size());
            pack_seq(nuc_a, w + wr.size(), m ? m + mr.size() : nullptr);
            vars.push_back(d);
            h.out_at = at;
            h.pos_r = (uint32_t)slot_r;
            hv.push_back(std::move(h));
        }
    }
    if ((rc = flush())) return rc;
    S.ms[0] += now_ms() - t_prep;
    return TFBS_OK;
}

}  // namespace tfbs
