// MI355X (gfx950) hit-list kernel: find_all_matches (main.rs:94-154) kept, not counted.
//
// For every distinct haplotype h of the asked regions, every strand p of the pattern set
// (creation order) and every window i with i + L <= len(h), the exact score -- a mono
// PWM's wrapping int32 column sum, a dinucleotide PWM's wrapping int32 pair sum, an N
// adding 0 -- is computed from the pattern set's own weights and compared with
// min_score.  Nothing of the count path is used: no plan, no lookup tables, no window
// lists, no diff runs, no reuse between haplotypes.  Brute force is the point: the list
// is a second opinion on the count path at any size.
//
//  * The pair a wave owns, the kernel's prologue, the walk over the pair's windows and the
//    scoring are hit_score.hpp's, as they are scan_best.hip's; so is the drivers' common
//    state, which uploads the tables that build_hit_tables makes here.
//  * Two passes run the same scoring code.  The count pass stores each pair's hits; an
//    exclusive u64 scan over the pairs, haplotype-major, turns them into offsets; the
//    fill pass places each chunk's hits behind the pair's offset with a ballot and a
//    popcount prefix.  The order (haplotype, pattern, window) comes out of the offsets:
//    no atomics, no fixed-capacity list, no sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hit_score.hpp"

namespace tfbs {
namespace {

struct HitsArgs {
    PairSrc src;
    const uint32_t *hap_ids;  // the chunk's haplotypes (batch indices)
    // pair p = chunk haplotype k * n_strands + strand.  The count pass stores the pair's
    // hits at off[p]; after the exclusive scan over the chunk's pairs + 1 values, off[p]
    // is the pair's first record and the last value the chunk's total
    uint64_t *off;
    uint32_t k0, k1;      // the haplotypes of the chunk this launch takes
    uint32_t n_chunk;     // haplotypes in the chunk (count pass: the total's slot is zeroed)
    // fill pass: record off[p] - rec_base of recs (rec_cap entries)
    uint64_t rec_base, rec_cap;
    DevHitRec *recs;
};

struct HitsPair {  // a record's fields besides the window and the score, and the threshold
    uint32_t hid, sidx;
    int32_t min_score;
};

// NCH 64-window chunks from window c0, in ascending order: scored together, counted or
// placed chunk by chunk.
template <bool FILL, int NCH>
__device__ __forceinline__ void hits_chunks(const HitsArgs &A, const PairScan &P, const HitsPair &Q, uint32_t c0,
                                            uint32_t lane, uint64_t &at) {
    uint32_t ii[NCH], s[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) ii[c] = scored_window(P, c0 + 64 * c + lane);
    SCORE_WINDOWS(NCH, P, ii, s);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t i = c0 + 64 * c + lane;
        const bool hit = i < P.nwin && (int32_t)s[c] > Q.min_score;
        const uint64_t mask = __ballot(hit);
        if (FILL && hit) {
            const uint32_t rank =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            const uint64_t r = at + rank;
            if (r < A.rec_cap) A.recs[r] = DevHitRec{Q.hid, Q.sidx, i, (int32_t)s[c]};
        }
        at += (uint32_t)__popcll(mask);
    }
}

// Grid: ceil((k1 - k0) * n_strands / kHitWaves) workgroups of kHitBlock threads.
template <bool FILL>
__global__ __launch_bounds__(kHitBlock) void scan_hits_kernel(HitsArgs A) {
    __shared__ int32_t s_rows[kHitWaves][kHitDiInts];
    const PairHead H = pair_head(A.src, A.k0, A.k1, s_rows);
    // before any load of the haplotype: the fill pass's time is the pairs without a hit returning at once
    if (!H.active) return;
    if (!FILL && H.pl == 0 && H.lane == 0) A.off[(uint64_t)A.n_chunk * A.src.n_strands] = 0;  // the total's slot
    if (FILL && A.off[H.p + 1] == A.off[H.p]) return;  // the count pass found no hit: nothing to place
    PAIR_OPEN(A.src, H, A.hap_ids, hid, hm, P);
    const HitsPair Q{hid, H.sidx, H.min_score};
    uint64_t at = FILL ? A.off[H.p] - A.rec_base : 0;  // records of the pair so far (fill: their place)
    WALK_CHUNKS(P.nwin, c0, (hits_chunks<FILL, NCH>(A, P, Q, c0, H.lane, at)));
    if (!FILL && H.lane == 0) A.off[H.p] = at;
}

// hap_off[k] = off[k * n_strands], k = 0 .. n_haps: the records before chunk haplotype k.
__global__ __launch_bounds__(256) void hits_hap_offsets_kernel(const uint64_t *__restrict__ off, uint32_t n_haps,
                                                                uint32_t n_strands, uint64_t *__restrict__ hap_off) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k <= n_haps) hap_off[k] = off[(uint64_t)k * n_strands];
}

}  // namespace

void build_hit_tables(const Patterns &P, HitTables *out) {
    out->strands.clear();
    out->weights.clear();
    for (const Pat &p : P.pats) {
        DevHitStrand s{};
        s.kind = (uint32_t)p.kind;
        s.min_score = p.min_score;
        s.w_off = (uint32_t)out->weights.size();
        if (p.kind == TFBS_KIND_PWM) {
            s.len = p.len;
            for (uint32_t j = 0; j < p.len; j++)
                for (int c = 0; c < 4; c++) out->weights.push_back(p.w5[5 * (size_t)j + c]);
        } else if (p.kind == TFBS_KIND_DIPWM) {
            s.len = p.len;
            out->weights.insert(out->weights.end(), p.w16.begin(), p.w16.end());
        } else {
            s.len = 0;  // TFBS_KIND_OTHER never matches
        }
        out->strands.push_back(s);
    }
}

struct HitsState : PairState {  // host: hap_off, then the records, copied back
    DevBuf<uint64_t> off, tmp, hap_off;
    DevBuf<DevHitRec> recs;
    double ms[4] = {0, 0, 0, 0};
};

void hits_state_destroy(HitsState *s) { delete s; }

void hits_last_ms(const HitsState *s, double out[4]) {
    for (int k = 0; k < 4; k++) out[k] = s ? s->ms[k] : 0.0;
}

namespace {

// Scratch of a chunk of nh haplotypes besides its records: the pairs' counters / offsets
// (u64: the scan works in place), the scan's tile sums, the haplotype list and offsets.
uint64_t chunk_fixed_bytes(uint64_t nh, uint64_t ns) {
    const uint64_t np = nh * ns + 1;
    return 8 * np + 8 * scan_tmp_words(np) + 4 * nh + 8 * (nh + 1);
}

}  // namespace

int hits_run(HitsState **state, int device, void *stream_, const Patterns &P, const ScanImage &img,
             const Batch &B, size_t r0, size_t r1, std::vector<tfbs_hit> *out, uint64_t *per_region) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, stream, 3, "hit tables")) return rc;
    HitsState &S = **state;
    for (double &m : S.ms) m = 0;
    if (per_region) std::fill(per_region, per_region + (r1 - r0), 0ull);
    const uint64_t ns = S.n_strands;
    // the distinct haplotypes of [r0, r1) in order (helper reference copies left out)
    std::vector<uint32_t> ids;
    for (size_t r = r0; r < r1; r++)
        for (uint32_t h = 0; h < B.rh[r].hap_count; h++) ids.push_back(B.rh[r].hap_begin + h);
    if (ids.empty() || ns == 0) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, "too many strands for the hit list kernel");
    const uint64_t budget = scratch_budget("TFBS_HITS_SCRATCH_MB", 256.0);  // read at the call

    HitsArgs A{};
    A.src = S.src(img);
    int rc;
    for (size_t start = 0; start < ids.size();) {
        // the chunk: as many haplotypes as the budget's counters allow, one at least
        uint64_t nh = std::min<uint64_t>(ids.size() - start, std::max<uint64_t>(1, kHitsMaxPairs / ns));
        nh = std::min(nh, std::max<uint64_t>(1, budget / (8 * ns + 12)));
        while (nh > 1 && chunk_fixed_bytes(nh, ns) > budget) nh -= std::max<uint64_t>(1, nh / 1024);
        const uint64_t fixed = chunk_fixed_bytes(nh, ns);
        const uint64_t np = nh * ns + 1;
        if ((rc = S.hap_ids.ensure_exact(nh)) || (rc = S.off.ensure_exact(np)) || (rc = S.tmp.ensure_exact(scan_tmp_words(np))) ||
            (rc = S.hap_off.ensure_exact(nh + 1)) || (rc = S.host.reserve(8 * (nh + 1))))
            return rc;
        HIP_TRY(hipMemcpyAsync(S.hap_ids.p, ids.data() + start, 4 * nh, hipMemcpyHostToDevice, stream));
        A.hap_ids = S.hap_ids.p;
        A.off = S.off.p;
        A.k0 = 0;
        A.k1 = A.n_chunk = (uint32_t)nh;
        HIP_TRY(hipEventRecord(S.ev[0], stream));
        hipLaunchKernelGGL(scan_hits_kernel<false>, dim3((uint32_t)((np - 1 + kHitWaves - 1) / kHitWaves)),
                           dim3(kHitBlock), 0, stream, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(S.ev[1], stream));
        if ((rc = exclusive_scan(S.off.p, np, S.tmp.p, stream))) return rc;
        hipLaunchKernelGGL(hits_hap_offsets_kernel, dim3((uint32_t)(nh / 256 + 1)), dim3(256), 0, stream, S.off.p,
                           (uint32_t)nh, (uint32_t)ns, S.hap_off.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(S.ev[2], stream));
        HIP_TRY(hipEventSynchronize(S.ev[2]));  // (the host part's clock starts when the kernels are done)
        double t0 = now_ms();
        HIP_TRY(hipMemcpyAsync(S.host.p, S.hap_off.p, 8 * (nh + 1), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        S.ms[0] += ms;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[1], S.ev[2]));
        S.ms[1] += ms;
        std::vector<uint64_t> hap_off(nh + 1);
        memcpy(hap_off.data(), S.host.p, 8 * (nh + 1));
        if (per_region) {
            for (uint64_t k = 0; k < nh; k++)
                per_region[B.haps[ids[start + k]].region - r0] += hap_off[k + 1] - hap_off[k];
            S.ms[3] += now_ms() - t0;
            start += nh;
            continue;
        }
        // the records, in runs of whole haplotypes that fit what the counters leave (one at least)
        const uint64_t room = budget > fixed ? (budget - fixed) / sizeof(DevHitRec) : 0;
        for (uint64_t k0 = 0; k0 < nh;) {
            uint64_t k1 = k0 + 1;
            while (k1 < nh && hap_off[k1 + 1] - hap_off[k0] <= room) k1++;
            const uint64_t nrec = hap_off[k1] - hap_off[k0];
            S.ms[3] += now_ms() - t0;
            if (nrec) {
                if ((rc = S.recs.ensure_exact(nrec)) || (rc = S.host.reserve(nrec * sizeof(DevHitRec)))) return rc;
                A.k0 = (uint32_t)k0;
                A.k1 = (uint32_t)k1;
                A.rec_base = hap_off[k0];
                A.rec_cap = nrec;
                A.recs = S.recs.p;
                HIP_TRY(hipEventRecord(S.ev[0], stream));
                hipLaunchKernelGGL(scan_hits_kernel<true>,
                                   dim3((uint32_t)(((k1 - k0) * ns + kHitWaves - 1) / kHitWaves)), dim3(kHitBlock), 0,
                                   stream, A);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(S.ev[1], stream));
                HIP_TRY(hipEventSynchronize(S.ev[1]));
                t0 = now_ms();
                HIP_TRY(hipMemcpyAsync(S.host.p, S.recs.p, nrec * sizeof(DevHitRec), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
                S.ms[2] += ms;
                const DevHitRec *rec = reinterpret_cast<const DevHitRec *>(S.host.p);
                const size_t base = out->size();
                out->resize(base + nrec);
                for (uint64_t x = 0; x < nrec; x++) {
                    const DevHitRec &q = rec[x];
                    const DevHap &hm = B.haps[q.hap];
                    const RegionH &R = B.rh[hm.region];
                    tfbs_hit &o = (*out)[base + x];
                    o.region = hm.region;
                    o.haplotype = q.hap - R.hap_begin;
                    o.pattern = q.pattern;
                    o.window = q.window;
                    site_range(B, P, R, hm, q.pattern, q.window, &o.start, &o.end);
                    o.score = q.score;
                    o.reserved = 0;
                }
            } else {
                t0 = now_ms();
            }
            k0 = k1;
        }
        S.ms[3] += now_ms() - t0;
        start += nh;
    }
    return TFBS_OK;
}

}  // namespace tfbs
