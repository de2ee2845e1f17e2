// The frame of the kernels that write one dense record per (distinct haplotype, pattern strand,
// inner range) -- scan_best.hip, scan_affinity.hip -- and of their drivers, on top of
// hit_score.hpp (the pair a wave owns, the prologue, the walk, the scoring, PairState).  A HIP
// header: only .hip sources include it.
//
//  * A region's ranges go in groups of kSweepRanges per sweep over the pair's windows: their
//    (s_rel, e_rel) pairs sit in scalar registers and a lane keeps the kind's state per range of
//    the group.  After the last chunk the kind folds the lanes and lane 0 writes one 16-byte
//    record with one vector store.
//  * The result is dense, so record (haplotype, strand, range) has a place known beforehand:
//    hap_off[haplotype] + strand * n_ranges + range.  No atomics, no count pass, no sort.
//  * The drivers run whole haplotypes in chunks under a scratch budget and expand a chunk's
//    records, copied back through the pinned buffer, into public ones.
//
// What a kernel does with a window's score is its *kind* K:
//    K::Rec                     the 16-byte device record
//    K::Lane                    a lane's state for one range of a sweep
//    K::Ctx                     what the kind needs beside the pair (wave-uniform)
//    K::init() -> Lane          a range's state before the first window
//    K::value(ctx, exists, s)   what a window of score s contributes: once per window
//    K::add(b, ov, i, v) -> Lane   b after window i of value v (ov: it exists and overlaps the range)
//    K::reduce(b) -> Rec        the butterfly over the lanes: every lane returns the record
// The lane states go in and out by value: with add() writing through a reference the built
// best kernel gains branches around each replacement (265 instructions).
#pragma once

#include <vector>

#include "hit_score.hpp"

namespace tfbs {

// Ranges of one sweep, chosen from the built kernels' registers (gfx950; DESIGN.md,
// "scan_best_kernel", "scan_affinity_kernel"): with 4 both take 68 VGPRs (7 waves per SIMD,
// nothing spilled; the hit kernel's count pass takes 46); the best kernel with 8 takes 81 (5
// waves, 43 SGPRs spilled), with 16 118 and 196 bytes of scratch per lane.  A region of the
// usual one to four ranges needs one sweep.
constexpr int kSweepRanges = 4;

struct SweepArgs {  // the head of both kernels' arguments; the records' pointer follows it
    PairSrc src;
    const int32_t *posrel;
    const DevRegion *regions;
    const int32_t *inner;
    const uint32_t *hap_ids;  // the chunk's haplotypes (batch indices)
    const uint64_t *hap_off;  // chunk haplotype k's first record: its n_strands x n_ranges follow
    uint32_t n_haps;
    uint64_t rec_cap;
};

// NCH 64-window chunks from window c0, in ascending order: scored together, then each existing
// window's value goes to the ranges of the sweep that range_overlaps(inner, match) gives it
// (range.rs:18-21: the match's start or its end lies inside the inner range).  pos: the
// windows' starts (null: window i starts at i).
template <typename K, int NCH, int NG>
__device__ __forceinline__ void sweep_chunks(const PairScan &P, const int32_t *pos, uint32_t c0, uint32_t lane,
                                             const typename K::Ctx &ctx, const int32_t (&rs)[NG],
                                             const int32_t (&re)[NG], typename K::Lane (&b)[NG]) {
    uint32_t ii[NCH], s[NCH];
    int32_t ms[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        ii[c] = scored_window(P, c0 + 64 * c + lane);
        ms[c] = pos ? pos[ii[c]] : (int32_t)ii[c];
    }
    SCORE_WINDOWS(NCH, P, ii, s);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t i = c0 + 64 * c + lane;
        const bool exists = i < P.nwin;
        const int32_t me = ms[c] + (int32_t)(P.L - 1);
        const auto v = K::value(ctx, exists, s[c]);
#pragma unroll
        for (int r = 0; r < NG; r++) {
            const bool ov = exists && ((rs[r] <= ms[c] && ms[c] <= re[r]) || (rs[r] <= me && me <= re[r]));
            b[r] = K::add(b[r], ov, i, v);
        }
    }
}

// One sweep over the pair's windows for ranges [first, first + ng) of `inner` (ng <= NG; the
// sweep is built for 1, 2 and kSweepRanges ranges, so a region of one range pays for one),
// then the reduction and the ng records from recs[rec].
template <typename K, int NG>
__device__ __forceinline__ void range_sweep(const SweepArgs &A, typename K::Rec *recs, const typename K::Ctx &ctx,
                                            const PairScan &P, const int32_t *pos, uint32_t lane, uint32_t first,
                                            uint32_t ng, uint64_t rec) {
    int32_t rs[NG], re[NG];
    typename K::Lane b[NG];
#pragma unroll
    for (int r = 0; r < NG; r++) {
        const bool have = (uint32_t)r < ng;  // (a range the group lacks overlaps nothing)
        const uint32_t at = 2 * (first + (have ? (uint32_t)r : 0u));
        rs[r] = __builtin_amdgcn_readfirstlane(have ? A.inner[at] : INT32_MAX);
        re[r] = __builtin_amdgcn_readfirstlane(have ? A.inner[at + 1] : INT32_MIN);
        b[r] = K::init();
    }
    WALK_CHUNKS(P.nwin, c0, (sweep_chunks<K, NCH, NG>(P, pos, c0, lane, ctx, rs, re, b)));
#pragma unroll
    for (int r = 0; r < NG; r++) {
        if ((uint32_t)r >= ng) break;  // (wave-uniform)
        const typename K::Rec out = K::reduce(b[r]);
        const uint64_t at = rec + (uint32_t)r;
        if (lane == 0 && at < A.rec_cap) recs[at] = out;
    }
}

// A kernel's body after PAIR_OPEN (nwin 0: every record is the empty one): the pair's records
// in sweeps of kSweepRanges ranges.  A macro for hit_score.hpp's reason: as a function both
// kernels build to other code (64 VGPRs, 8 waves per SIMD), which has not been timed; expanded
// in place they keep the registers and the occupancy they were measured with.
#define RANGE_SWEEPS(K, A, recs, ctx, H, hm, P)                                                              \
    do {                                                                                                     \
        const DevRegion rg = (A).regions[hm.region];                                                         \
        const uint32_t n_inner = __builtin_amdgcn_readfirstlane(rg.n_inner);                                 \
        const uint32_t inner_off = __builtin_amdgcn_readfirstlane(rg.inner_off);                             \
        const int32_t *pos = (hm.flags & HAP_HAS_POS) ? (A).posrel + hm.pos_off : nullptr;                   \
        const uint32_t lane = (H).lane;                                                                      \
        const uint64_t rec0 = (A).hap_off[(H).k] + (uint64_t)(H).sidx * n_inner;                             \
        for (uint32_t g0 = 0; g0 < n_inner; g0 += kSweepRanges) {                                            \
            const uint32_t ng = min((uint32_t)kSweepRanges, n_inner - g0);                                   \
            if (ng == 1) range_sweep<K, 1>(A, recs, ctx, P, pos, lane, inner_off + g0, ng, rec0 + g0);       \
            else if (ng == 2) range_sweep<K, 2>(A, recs, ctx, P, pos, lane, inner_off + g0, ng, rec0 + g0);  \
            else range_sweep<K, kSweepRanges>(A, recs, ctx, P, pos, lane, inner_off + g0, ng, rec0 + g0);    \
        }                                                                                                    \
    } while (0)

// ---- host: the drivers' state and the one chunk driver
template <typename Rec>
struct RangeState : PairState {  // a chunk's records' places and the records, copied back
    DevBuf<uint64_t> hap_off;
    DevBuf<Rec> recs;
    double ms[2] = {0, 0};  // the last run's kernel (HIP events), copy-back + host part (wall)
};

template <typename Rec>
void range_last_ms(const RangeState<Rec> *s, double out[2]) {
    for (int k = 0; k < 2; k++) out[k] = s ? s->ms[k] : 0.0;
}

// One chunk of whole haplotypes: their batch indices ids[0 .. nh) and their records' places
// (hap_off, nrec records in all) uploaded, `kernel` run on A -- the kind's own arguments set
// by the caller, A.head and A.recs here -- and waited for.  *kernel_ms += the kernel's time.
template <typename Rec, typename Args>
int range_launch_chunk(RangeState<Rec> &S, hipStream_t stream, const ScanImage &img, const uint32_t *ids,
                       const uint64_t *hap_off, size_t nh, uint64_t nrec, void (*kernel)(Args), Args A,
                       double *kernel_ms) {
    int rc;
    if ((rc = S.hap_ids.ensure_exact(nh)) || (rc = S.hap_off.ensure_exact(nh)) || (rc = S.recs.ensure_exact(nrec))) return rc;
    HIP_TRY(hipMemcpyAsync(S.hap_ids.p, ids, 4 * nh, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(S.hap_off.p, hap_off, 8 * nh, hipMemcpyHostToDevice, stream));
    A.head = SweepArgs{S.src(img), img.posrel, img.regions, img.inner, S.hap_ids.p, S.hap_off.p, (uint32_t)nh, nrec};
    A.recs = S.recs.p;
    HIP_TRY(hipEventRecord(S.ev[0], stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((nh * S.n_strands + kHitWaves - 1) / kHitWaves)), dim3(kHitBlock), 0,
                       stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.ev[1], stream));
    HIP_TRY(hipEventSynchronize(S.ev[1]));  // (the host part's clock starts when the kernel is done)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    *kernel_ms += ms;
    return TFBS_OK;
}

// The dense records of regions [r0, r1) of B appended to *out, sorted by (region, haplotype,
// strand, range).  region_hook(r, R), for a region with ranges, may refuse (non-zero); a failure
// past it reads "... the <label> kernel"; scratch_env names the chunks' budget in MiB (read at
// the call); A carries the kind's own arguments; expand(R, hm, haplotype in region, strand,
// range, record, o) fills the public record o of haplotype hm of region R, in place: the best
// records returned by value and assigned cost the host part some 6 %.  Synchronises `stream`.
template <typename Rec, typename Args, typename Pub, typename Hook, typename Expand>
int range_run(RangeState<Rec> &S, hipStream_t stream, const ScanImage &img, const Batch &B, size_t r0, size_t r1,
              const char *label, const char *scratch_env, void (*kernel)(Args), const Args &A, Hook region_hook,
              Expand expand, std::vector<Pub> *out) {
    S.ms[0] = S.ms[1] = 0;
    const uint64_t ns = S.n_strands;
    // the distinct haplotypes of [r0, r1) that have records, in order (helper reference copies
    // left out; a region without a non-empty inner range has none)
    std::vector<uint32_t> ids;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        // the public range index is the place in R.ranges: ascending (start, end), no repeats
        for (size_t k = 1; k < R.ranges.size(); k++)
            if (!(R.ranges[k - 1] < R.ranges[k])) return fail(TFBS_E_STATE, "inner ranges of a region not ascending");
        if (R.ranges.size() != B.regions[r].n_inner) return fail(TFBS_E_STATE, "inner ranges of a region not packed");
        if (R.ranges.empty()) continue;
        for (uint32_t h = 0; h < R.hap_count; h++) ids.push_back(R.hap_begin + h);
        if (int rc = region_hook(r, R)) return rc;
    }
    if (ids.empty() || ns == 0) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, std::string("too many strands for the ") + label + " kernel");
    const uint64_t budget = scratch_budget(scratch_env, 256.0);
    const uint64_t max_h = std::max<uint64_t>(1, kHitsMaxPairs / ns);
    auto recs_of = [&](uint32_t id) { return ns * (uint64_t)B.rh[B.haps[id].region].ranges.size(); };

    int rc;
    std::vector<uint64_t> hap_off;
    for (size_t start = 0; start < ids.size();) {
        // the chunk: whole haplotypes whose records fit the budget, one at least
        hap_off.clear();
        uint64_t nrec = 0;
        size_t nh = 0;
        while (start + nh < ids.size() && nh < max_h) {
            const uint64_t add = recs_of(ids[start + nh]);
            if (nh && (nrec + add) * sizeof(Rec) > budget) break;
            hap_off.push_back(nrec);
            nrec += add;
            nh++;
        }
        if ((rc = S.host.reserve(nrec * sizeof(Rec))) ||
            (rc = range_launch_chunk(S, stream, img, ids.data() + start, hap_off.data(), nh, nrec, kernel, A, &S.ms[0])))
            return rc;
        const double t0 = now_ms();
        HIP_TRY(hipMemcpyAsync(S.host.p, S.recs.p, nrec * sizeof(Rec), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const Rec *rec = reinterpret_cast<const Rec *>(S.host.p);
        size_t at = out->size();
        out->resize(at + nrec);
        for (size_t k = 0; k < nh; k++) {
            const uint32_t id = ids[start + k];
            const DevHap &hm = B.haps[id];
            const RegionH &R = B.rh[hm.region];
            const uint32_t nr = (uint32_t)R.ranges.size();
            const Rec *q = rec + hap_off[k];
            for (uint32_t p = 0; p < ns; p++)
                for (uint32_t x = 0; x < nr; x++, q++, at++) expand(R, hm, id - R.hap_begin, p, x, *q, (*out)[at]);
        }
        S.ms[1] += now_ms() - t0;
        start += nh;
    }
    return TFBS_OK;
}

}  // namespace tfbs
