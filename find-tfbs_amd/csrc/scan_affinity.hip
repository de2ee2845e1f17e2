// MI355X (gfx950) binding-affinity kernel: per (distinct haplotype, pattern strand, inner range)
// the sum over the windows whose match range overlaps the range of the fixed-point weight
// a(top - score) = floor(2^40 * exp(-(top - score) / 1000)), the number of such windows and
// the number of them with a weight above 0 (include/tfbs_amd.h, "Binding affinity").
//
// The pair a wave owns, the prologue, the walk over the pair's windows and the scoring are
// hit_score.hpp's; the range sweeps, the dense records' places and the chunk driver are
// range_sweep.hpp's, shared with scan_best.hip.  This file keeps the affinity kind -- what is
// done with a window's score -- its tables, its one refusal and its public record:
//
//  * The two tables of a(d) (affinity_tables.hpp, 8 224 bytes) are staged in LDS once per
//    workgroup, ahead of the prologue's barrier; the strand's top comes through a scalar load.
//  * Per window d = top - score (below 2^32: the driver refuses a set whose sums can wrap), then
//    a(d) = umul64hi(T1[d % 1000], T2[d / 1000]) >> 22 for d <= kAffLast, once per window whatever
//    the ranges it overlaps.  Most windows of a real peak lie beyond kAffLast, so the two LDS
//    reads and the 64-bit multiply stand under a branch: a wave none of whose lanes needs them
//    skips them.
//  * A lane keeps (sum, windows, nonzero) per range of the sweep.  Integer adds only, so after
//    the last chunk a butterfly of adds over the lanes gives the same record in any order.  A
//    lane's sum stays below windows * 2^40 < 2^63 (the driver refuses a region of 2^23 bases).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "affinity_rows.hpp"
#include "affinity_tables.hpp"
#include "range_sweep.hpp"

namespace tfbs {
namespace {

constexpr uint32_t kAffTableLen = kAffT1Len + kAffT2Len;

typedef const __attribute__((address_space(4))) int32_t CTop;  // wave-uniform: a scalar load

struct AffKind {
    typedef DevAffRec Rec;
    struct Ctx {
        const uint64_t *t;  // the staged tables: T1 then T2
        int32_t top;        // the strand's pattern_id's reference score
    };
    struct Lane {  // a lane's running sum and counts for a range of the sweep
        uint64_t sum;
        uint32_t n, nz;
    };
    static __device__ __forceinline__ Lane init() { return Lane{0, 0, 0}; }
    // a(d) of the window; top >= score and top - score < 2^32 as integers, so the wrapping
    // difference is d
    static __device__ __forceinline__ uint64_t value(const Ctx &c, bool exists, uint32_t s) {
        const uint32_t d = exists ? (uint32_t)c.top - s : UINT32_MAX;
        uint64_t a = 0;
        if (d <= kAffLast) {
            const uint32_t q = d / 1000u;
            a = __umul64hi(c.t[d - 1000u * q], c.t[kAffT1Len + q]) >> 22;
        }
        return a;
    }
    static __device__ __forceinline__ Lane add(Lane b, bool ov, uint32_t, uint64_t a) {
        return Lane{b.sum + (ov ? a : 0ull), b.n + (ov ? 1u : 0u), b.nz + (ov && a ? 1u : 0u)};
    }
    static __device__ __forceinline__ Rec reduce(Lane b) {
        unsigned long long sum = b.sum;
        uint32_t n = b.n, nz = b.nz;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sum += (unsigned long long)__shfl_xor((long long)sum, m);
            n += (uint32_t)__shfl_xor((int)n, m);
            nz += (uint32_t)__shfl_xor((int)nz, m);
        }
        return DevAffRec{sum, n, nz};
    }
};

struct AffArgs {
    SweepArgs head;
    DevAffRec *recs;
    const uint64_t *tables;  // T1 then T2
    const int32_t *tops;     // per strand: its pattern_id's reference score
};

// Grid: ceil(n_haps * n_strands / kHitWaves) workgroups of kHitBlock threads.
__global__ __launch_bounds__(kHitBlock) void scan_affinity_kernel(AffArgs A) {
    __shared__ int32_t s_rows[kHitWaves][kHitDiInts];
    __shared__ uint64_t s_tab[kAffTableLen];
    for (uint32_t x = threadIdx.x; x < kAffTableLen; x += kHitBlock) s_tab[x] = A.tables[x];
    const PairHead H = pair_head(A.head.src, 0, A.head.n_haps, s_rows);  // (its barrier covers s_tab)
    if (!H.active) return;
    PAIR_OPEN(A.head.src, H, A.head.hap_ids, hid, hm, P);
    const AffKind::Ctx ctx{s_tab, ((CTop *)A.tops)[H.sidx]};
    RANGE_SWEEPS(AffKind, A.head, A.recs, ctx, H, hm, P);
}

}  // namespace

struct AffinityState : RangeState<DevAffRec> {  // and the tables and the tops
    DevBuf<uint64_t> tables;
    DevBuf<int32_t> tops;
    uint32_t max_strands = 0;  // the most strands one pattern_id has
    // PairState's upload, then the two tables and the tops (checked beforehand: affinity_run).
    int upload(const Patterns &P, hipStream_t stream, int n_events, const char *label) {
        std::vector<int32_t> t;
        if (int rc = affinity_tops(P, &t)) return rc;
        if (int rc = PairState::upload(P, stream, n_events, label)) return rc;
        std::vector<uint64_t> tab(kAffT1, kAffT1 + kAffT1Len);
        tab.insert(tab.end(), kAffT2, kAffT2 + kAffT2Len);
        t.resize(t.size() + 1);  // (never empty)
        int rc;
        if ((rc = tables.put(tab, stream)) || (rc = tops.put(t, stream))) return rc;
        HIP_TRY(hipStreamSynchronize(stream));  // (tab and t go out of scope)
        max_strands = affinity_max_strands(P);
        return TFBS_OK;
    }
};

void affinity_state_destroy(AffinityState *s) { delete s; }

void affinity_last_ms(const AffinityState *s, double out[2]) { range_last_ms<DevAffRec>(s, out); }

int affinity_prepare(AffinityState **state, int device, void *stream, const Patterns &P, uint32_t *n_strands) {
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, static_cast<hipStream_t>(stream), 2, "affinity tables")) return rc;
    *n_strands = (*state)->n_strands;
    return TFBS_OK;
}

int affinity_region_check(const AffinityState *state, const Batch &B, size_t r, const RegionH &R) {
    uint64_t longest = 0;
    for (uint32_t h = 0; h < R.hap_count; h++) longest = std::max<uint64_t>(longest, B.haps[R.hap_begin + h].len);
    if (longest * state->max_strands >= (1ull << 23))
        return fail(TFBS_E_ARG, "region " + std::to_string(r) + ": its longest haplotype times the most strands of "
                                    "one pattern_id reaches 2^23: an affinity sum could pass 2^63");
    return TFBS_OK;
}

namespace {

AffArgs aff_args(const AffinityState &S) {  // the kind's own arguments
    AffArgs A{};
    A.tables = S.tables.p;
    A.tops = S.tops.p;
    return A;
}

}  // namespace

int affinity_launch_chunk(AffinityState *state, void *stream, const ScanImage &img, const uint32_t *ids,
                          const uint64_t *hap_off, size_t nh, uint64_t nrec, const uint64_t **d_hap_off,
                          const DevAffRec **recs, double *kernel_ms) {
    if (int rc = range_launch_chunk(*state, static_cast<hipStream_t>(stream), img, ids, hap_off, nh, nrec,
                                    scan_affinity_kernel, aff_args(*state), kernel_ms))
        return rc;
    *d_hap_off = state->hap_off.p;
    *recs = state->recs.p;
    return TFBS_OK;
}

int affinity_run(AffinityState **state, int device, void *stream, const Patterns &P, const ScanImage &img,
                 const Batch &B, size_t r0, size_t r1, std::vector<tfbs_affinity> *out) {
    uint32_t n_strands = 0;
    if (int rc = affinity_prepare(state, device, stream, P, &n_strands)) return rc;
    AffinityState &S = **state;
    return range_run(
        S, static_cast<hipStream_t>(stream), img, B, r0, r1, "affinity", "TFBS_AFFINITY_SCRATCH_MB", scan_affinity_kernel,
        aff_args(S), [&](size_t r, const RegionH &R) { return affinity_region_check(&S, B, r, R); },
        [](const RegionH &, const DevHap &hm, uint32_t hap, uint32_t p, uint32_t x, const DevAffRec &q, tfbs_affinity &o) {
            o = tfbs_affinity{hm.region, hap, p, x, q.n_windows, q.n_nonzero, q.sum};
        },
        out);
}

}  // namespace tfbs
