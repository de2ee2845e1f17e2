// MI355X (gfx950) best-site kernel: per (distinct haplotype, pattern strand, inner range)
// the highest score among the windows whose match range overlaps the range, the lowest
// window attaining it and the number of such windows.  min_score plays no part.
//
// The pair a wave owns, the prologue, the walk over the pair's windows and the scoring are
// hit_score.hpp's: brute force over every window of every distinct haplotype from the pattern
// set alone -- no plan, no lookup tables, no window lists, no reuse between haplotypes.  The
// range sweeps, the dense records' places and the chunk driver are range_sweep.hpp's, shared
// with scan_affinity.hip.  This file keeps the best-site kind: what is done with a window's
// score, and how a device record becomes a public one.
//
//  * A lane keeps (score, window, count) per range of the sweep.  It meets its windows in
//    ascending order, so a strictly greater score (or the first overlap) replaces its best:
//    ties stay on the lowest window.
//  * After the last chunk a butterfly over the lanes takes the maximum of
//    (int64(score) << 32) | (0xFFFFFFFF - window) and the sum of the counts.  A lane without a
//    window in the range holds (INT32_MIN, UINT32_MAX): the lowest key there is, below a
//    genuine INT32_MIN at any window.
#include <hip/hip_runtime.h>

#include <vector>

#include "range_sweep.hpp"
#include "scores.hpp"

namespace tfbs {
namespace {

struct BestKind {
    typedef DevBestRec Rec;
    struct Ctx {};
    struct Lane {  // a lane's running best and count for a range of the sweep
        int32_t score;
        uint32_t window, n;
    };
    static __device__ __forceinline__ Lane init() { return Lane{INT32_MIN, UINT32_MAX, 0}; }
    static __device__ __forceinline__ int32_t value(const Ctx &, bool, uint32_t s) { return (int32_t)s; }
    static __device__ __forceinline__ Lane add(Lane b, bool ov, uint32_t i, int32_t sc) {
        const bool better = ov && (b.n == 0 || sc > b.score);
        return Lane{better ? sc : b.score, better ? i : b.window, b.n + (ov ? 1u : 0u)};
    }
    static __device__ __forceinline__ Rec reduce(Lane b) {
        long long key = (long long)(((unsigned long long)(uint32_t)b.score << 32) | (0xFFFFFFFFu - b.window));
        uint32_t n = b.n;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const long long o = __shfl_xor(key, m);
            key = o > key ? o : key;
            n += (uint32_t)__shfl_xor((int)n, m);
        }
        return DevBestRec{(int32_t)(key >> 32), 0xFFFFFFFFu - (uint32_t)key, n, 0u};
    }
};

struct BestArgs {
    SweepArgs head;
    DevBestRec *recs;
};

// Grid: ceil(n_haps * n_strands / kHitWaves) workgroups of kHitBlock threads.
__global__ __launch_bounds__(kHitBlock) void scan_best_kernel(BestArgs A) {
    __shared__ int32_t s_rows[kHitWaves][kHitDiInts];
    const PairHead H = pair_head(A.head.src, 0, A.head.n_haps, s_rows);
    if (!H.active) return;
    PAIR_OPEN(A.head.src, H, A.head.hap_ids, hid, hm, P);
    const BestKind::Ctx ctx{};
    RANGE_SWEEPS(BestKind, A.head, A.recs, ctx, H, hm, P);
}

}  // namespace

struct BestState : RangeState<DevBestRec> {};

void best_state_destroy(BestState *s) { delete s; }

void best_last_ms(const BestState *s, double out[2]) { range_last_ms<DevBestRec>(s, out); }

int best_prepare(BestState **state, int device, void *stream, const Patterns &P, uint32_t *n_strands) {
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, static_cast<hipStream_t>(stream), 2, "best-site tables")) return rc;
    *n_strands = (*state)->n_strands;
    return TFBS_OK;
}

int best_launch_chunk(BestState *state, void *stream, const ScanImage &img, const uint32_t *ids,
                      const uint64_t *hap_off, size_t nh, uint64_t nrec, const uint64_t **d_hap_off,
                      const DevBestRec **recs, double *kernel_ms) {
    if (int rc = range_launch_chunk(*state, static_cast<hipStream_t>(stream), img, ids, hap_off, nh, nrec,
                                    scan_best_kernel, BestArgs{}, kernel_ms))
        return rc;
    *d_hap_off = state->hap_off.p;
    *recs = state->recs.p;
    return TFBS_OK;
}

int best_run(BestState **state, int device, void *stream, const Patterns &P, const ScanImage &img, const Batch &B,
             size_t r0, size_t r1, std::vector<tfbs_best> *out) {
    uint32_t n_strands = 0;
    if (int rc = best_prepare(state, device, stream, P, &n_strands)) return rc;
    return range_run(
        **state, static_cast<hipStream_t>(stream), img, B, r0, r1, "best-site", "TFBS_BEST_SCRATCH_MB", scan_best_kernel,
        BestArgs{}, [](size_t, const RegionH &) { return TFBS_OK; },
        [&](const RegionH &R, const DevHap &hm, uint32_t hap, uint32_t p, uint32_t x, const DevBestRec &q, tfbs_best &o) {
            o.region = hm.region;
            o.haplotype = hap;
            o.pattern = p;
            o.range = x;
            o.window = q.window;
            o.n_windows = q.n_windows;
            o.score = q.score;
            o.reserved = 0;
            o.start = o.end = 0;
            if (q.n_windows) site_range(B, P, R, hm, p, q.window, &o.start, &o.end);
        },
        out);
}

}  // namespace tfbs
