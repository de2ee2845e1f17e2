// MI355X (gfx950) best-site kernel: per (distinct haplotype, pattern strand, inner range)
// the highest score among the windows whose match range overlaps the range, the lowest
// window attaining it and the number of such windows.  min_score plays no part.
//
// The pair a wave owns, the prologue, the walk over the pair's windows and the scoring are
// hit_score.hpp's, shared with scan_hits.hip, and so is the driver's base (PairState): brute
// force over every window of every distinct haplotype from the pattern set alone -- no plan,
// no lookup tables, no window lists, no reuse between haplotypes.  This file keeps what is
// done with a chunk's scores and the range sweeps.
//
//  * The region's ranges go in groups of kBestRanges per sweep over the windows: their
//    (s_rel, e_rel) pairs sit in scalar registers, and a lane keeps (score, window, count)
//    per range of the group.  A lane meets its windows in ascending order, so a strictly
//    greater score (or the first overlap) replaces its best: ties stay on the lowest window.
//  * After the last chunk a butterfly over the lanes takes the maximum of
//    (int64(score) << 32) | (0xFFFFFFFF - window) and the sum of the counts; lane 0 writes
//    one 16-byte record with one vector store.  A lane without a window in the range holds
//    (INT32_MIN, UINT32_MAX): the lowest key there is, below a genuine INT32_MIN at any window.
//  * The result is dense, so record (haplotype, strand, range) has a place known beforehand:
//    hap_off[haplotype] + strand * n_ranges + range.  No atomics, no count pass, no sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "hit_score.hpp"
#include "scores.hpp"

namespace tfbs {
namespace {

// Ranges of one sweep, chosen from the built kernel's registers (gfx950; DESIGN.md,
// "scan_best_kernel"): 4 ranges take 68 VGPRs (7 waves per SIMD, nothing spilled; the hit
// kernel's count pass takes 46), 8 take 81 (5 waves, 43 SGPRs spilled), 16 take 118 and 196
// bytes of scratch per lane.  A region of the usual one to four ranges needs one sweep.
constexpr int kBestRanges = 4;

struct BestArgs {
    PairSrc src;
    const int32_t *posrel;
    const DevRegion *regions;
    const int32_t *inner;
    const uint32_t *hap_ids;  // the chunk's haplotypes (batch indices)
    const uint64_t *hap_off;  // chunk haplotype k's first record: its n_strands x n_ranges follow
    uint32_t n_haps;
    uint64_t rec_cap;
    DevBestRec *recs;
};

template <int NG>
struct BestLane {  // a lane's running best and count per range of the sweep
    int32_t score[NG];
    uint32_t window[NG], n[NG];
};

// NCH 64-window chunks from window c0, in ascending order: scored together, then each
// existing window is tested against the sweep's NG ranges by range_overlaps(inner, match)
// (range.rs:18-21: the match's start or its end lies inside the inner range).  pos: the
// windows' starts (null: window i starts at i).
template <int NCH, int NG>
__device__ __forceinline__ void best_chunks(const PairScan &P, const int32_t *pos, uint32_t c0, uint32_t lane,
                                            const int32_t (&rs)[NG], const int32_t (&re)[NG], BestLane<NG> &b) {
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
        const int32_t me = ms[c] + (int32_t)(P.L - 1), sc = (int32_t)s[c];
#pragma unroll
        for (int r = 0; r < NG; r++) {
            const bool ov = exists && ((rs[r] <= ms[c] && ms[c] <= re[r]) || (rs[r] <= me && me <= re[r]));
            const bool better = ov && (b.n[r] == 0 || sc > b.score[r]);
            b.score[r] = better ? sc : b.score[r];
            b.window[r] = better ? i : b.window[r];
            b.n[r] += ov ? 1u : 0u;
        }
    }
}

// One sweep over the pair's windows for ranges [first, first + ng) of `inner` (ng <= NG; the
// sweep is built for 1, 2 and kBestRanges ranges, so a region of one range pays for one),
// then the reduction and the ng records from recs[rec].
template <int NG>
__device__ __forceinline__ void best_sweep(const BestArgs &A, const PairScan &P, const int32_t *pos, uint32_t lane,
                                           uint32_t first, uint32_t ng, uint64_t rec) {
    int32_t rs[NG], re[NG];
    BestLane<NG> b;
#pragma unroll
    for (int r = 0; r < NG; r++) {
        const bool have = (uint32_t)r < ng;  // (a range the group lacks overlaps nothing)
        const uint32_t at = 2 * (first + (have ? (uint32_t)r : 0u));
        rs[r] = __builtin_amdgcn_readfirstlane(have ? A.inner[at] : INT32_MAX);
        re[r] = __builtin_amdgcn_readfirstlane(have ? A.inner[at + 1] : INT32_MIN);
        b.score[r] = INT32_MIN;
        b.window[r] = UINT32_MAX;
        b.n[r] = 0;
    }
    WALK_CHUNKS(P.nwin, c0, (best_chunks<NCH, NG>(P, pos, c0, lane, rs, re, b)));
#pragma unroll
    for (int r = 0; r < NG; r++) {
        if ((uint32_t)r >= ng) break;  // (wave-uniform)
        long long key = (long long)(((unsigned long long)(uint32_t)b.score[r] << 32) | (0xFFFFFFFFu - b.window[r]));
        uint32_t n = b.n[r];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const long long o = __shfl_xor(key, m);
            key = o > key ? o : key;
            n += (uint32_t)__shfl_xor((int)n, m);
        }
        const uint64_t at = rec + (uint32_t)r;
        if (lane == 0 && at < A.rec_cap)
            A.recs[at] = DevBestRec{(int32_t)(key >> 32), 0xFFFFFFFFu - (uint32_t)key, n, 0u};
    }
}

// Grid: ceil(n_haps * n_strands / kHitWaves) workgroups of kHitBlock threads.
__global__ __launch_bounds__(kHitBlock) void scan_best_kernel(BestArgs A) {
    __shared__ int32_t s_rows[kHitWaves][kHitDiInts];
    const PairHead H = pair_head(A.src, 0, A.n_haps, s_rows);
    if (!H.active) return;
    PAIR_OPEN(A.src, H, A.hap_ids, hid, hm, P);  // (nwin 0: every record is the empty one)
    const DevRegion rg = A.regions[hm.region];
    const uint32_t n_inner = __builtin_amdgcn_readfirstlane(rg.n_inner);
    const uint32_t inner_off = __builtin_amdgcn_readfirstlane(rg.inner_off);
    const int32_t *pos = (hm.flags & HAP_HAS_POS) ? A.posrel + hm.pos_off : nullptr;
    const uint32_t lane = H.lane;
    const uint64_t rec0 = A.hap_off[H.k] + (uint64_t)H.sidx * n_inner;
    for (uint32_t g0 = 0; g0 < n_inner; g0 += kBestRanges) {
        const uint32_t ng = min((uint32_t)kBestRanges, n_inner - g0);
        if (ng == 1) best_sweep<1>(A, P, pos, lane, inner_off + g0, ng, rec0 + g0);
        else if (ng == 2) best_sweep<2>(A, P, pos, lane, inner_off + g0, ng, rec0 + g0);
        else best_sweep<kBestRanges>(A, P, pos, lane, inner_off + g0, ng, rec0 + g0);
    }
}

}  // namespace

struct BestState : PairState {  // host: a chunk's records, copied back
    DevBuf<uint64_t> hap_off;
    DevBuf<DevBestRec> recs;
    double ms[2] = {0, 0};
};

void best_state_destroy(BestState *s) { delete s; }

void best_last_ms(const BestState *s, double out[2]) {
    for (int k = 0; k < 2; k++) out[k] = s ? s->ms[k] : 0.0;
}

int best_prepare(BestState **state, int device, void *stream, const Patterns &P, uint32_t *n_strands) {
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, static_cast<hipStream_t>(stream), 2, "best-site tables")) return rc;
    *n_strands = (*state)->n_strands;
    return TFBS_OK;
}

int best_launch_chunk(BestState *state, void *stream_, const ScanImage &img, const uint32_t *ids,
                      const uint64_t *hap_off, size_t nh, uint64_t nrec, const uint64_t **d_hap_off,
                      const DevBestRec **recs, double *kernel_ms) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    BestState &S = *state;
    int rc;
    if ((rc = S.hap_ids.ensure_exact(nh)) || (rc = S.hap_off.ensure_exact(nh)) || (rc = S.recs.ensure_exact(nrec))) return rc;
    HIP_TRY(hipMemcpyAsync(S.hap_ids.p, ids, 4 * nh, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(S.hap_off.p, hap_off, 8 * nh, hipMemcpyHostToDevice, stream));
    BestArgs A{};
    A.src = S.src(img);
    A.posrel = img.posrel;
    A.regions = img.regions;
    A.inner = img.inner;
    A.hap_ids = S.hap_ids.p;
    A.hap_off = S.hap_off.p;
    A.n_haps = (uint32_t)nh;
    A.rec_cap = nrec;
    A.recs = S.recs.p;
    HIP_TRY(hipEventRecord(S.ev[0], stream));
    hipLaunchKernelGGL(scan_best_kernel, dim3((uint32_t)((nh * S.n_strands + kHitWaves - 1) / kHitWaves)),
                       dim3(kHitBlock), 0, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.ev[1], stream));
    HIP_TRY(hipEventSynchronize(S.ev[1]));  // (the host part's clock starts when the kernel is done)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    *kernel_ms += ms;
    *d_hap_off = S.hap_off.p;
    *recs = S.recs.p;
    return TFBS_OK;
}

int best_run(BestState **state, int device, void *stream_, const Patterns &P, const ScanImage &img, const Batch &B,
             size_t r0, size_t r1, std::vector<tfbs_best> *out) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    uint32_t n_strands = 0;
    if (int rc = best_prepare(state, device, stream_, P, &n_strands)) return rc;
    BestState &S = **state;
    S.ms[0] = S.ms[1] = 0;
    const uint64_t ns = n_strands;
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
    }
    if (ids.empty() || ns == 0) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, "too many strands for the best-site kernel");
    const uint64_t budget = scratch_budget("TFBS_BEST_SCRATCH_MB", 256.0);  // read at the call
    auto recs_of = [&](uint32_t id) { return ns * (uint64_t)B.rh[B.haps[id].region].ranges.size(); };

    int rc;
    std::vector<uint64_t> hap_off;
    for (size_t start = 0; start < ids.size();) {
        // the chunk: whole haplotypes whose records fit the budget, one at least
        hap_off.clear();
        uint64_t nrec = 0;
        size_t nh = 0;
        const uint64_t max_h = std::max<uint64_t>(1, kHitsMaxPairs / ns);
        while (start + nh < ids.size() && nh < max_h) {
            const uint64_t add = recs_of(ids[start + nh]);
            if (nh && (nrec + add) * sizeof(DevBestRec) > budget) break;
            hap_off.push_back(nrec);
            nrec += add;
            nh++;
        }
        const uint64_t *d_hap_off;
        const DevBestRec *d_recs;
        if ((rc = S.host.reserve(nrec * sizeof(DevBestRec))) ||
            (rc = best_launch_chunk(&S, stream_, img, ids.data() + start, hap_off.data(), nh, nrec, &d_hap_off, &d_recs,
                                    &S.ms[0])))
            return rc;
        const double t0 = now_ms();
        HIP_TRY(hipMemcpyAsync(S.host.p, S.recs.p, nrec * sizeof(DevBestRec), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const DevBestRec *rec = reinterpret_cast<const DevBestRec *>(S.host.p);
        size_t at = out->size();
        out->resize(at + nrec);
        for (size_t k = 0; k < nh; k++) {
            const uint32_t id = ids[start + k];
            const DevHap &hm = B.haps[id];
            const RegionH &R = B.rh[hm.region];
            const uint32_t nr = (uint32_t)R.ranges.size();
            const DevBestRec *q = rec + hap_off[k];
            for (uint32_t p = 0; p < ns; p++)
                for (uint32_t x = 0; x < nr; x++, q++, at++) {
                    tfbs_best &o = (*out)[at];
                    o.region = hm.region;
                    o.haplotype = id - R.hap_begin;
                    o.pattern = p;
                    o.range = x;
                    o.window = q->window;
                    o.n_windows = q->n_windows;
                    o.score = q->score;
                    o.reserved = 0;
                    o.start = o.end = 0;
                    if (q->n_windows) site_range(B, P, R, hm, p, q->window, &o.start, &o.end);
                }
        }
        S.ms[1] += now_ms() - t0;
        start += nh;
    }
    return TFBS_OK;
}

}  // namespace tfbs
