// MI355X (gfx950) binding-affinity kernel: per (distinct haplotype, pattern strand, inner range)
// the sum over the windows whose match range overlaps the range of the fixed-point weight
// a(top - score) = floor(2^40 * exp(-(top - score) / 1000)), the number of such windows and
// the number of them with a weight above 0 (include/tfbs_amd.h, "Binding affinity").
//
// The frame is scan_best.hip's: the pair a wave owns, the prologue, the walk over the pair's
// windows and the scoring are hit_score.hpp's, the driver's base is PairState, the ranges go
// in sweeps of kAffRanges with their bounds in scalar registers, and a record's place is known
// beforehand (hap_off[haplotype] + strand * n_ranges + range): no atomics, no count pass, no
// sort.  What differs is what is done with a chunk's scores:
//
//  * The two tables of a(d) (affinity_tables.hpp, 8 224 bytes) are staged in LDS once per
//    workgroup, ahead of the prologue's barrier; the strand's top comes through a scalar load.
//  * Per window d = top - score (below 2^32: the driver refuses a set whose sums can wrap), then
//    a(d) = umul64hi(T1[d % 1000], T2[d / 1000]) >> 22 for d <= kAffLast.  Most windows of a real
//    peak lie beyond kAffLast, so the two LDS reads and the 64-bit multiply stand under a branch:
//    a wave none of whose lanes needs them skips them.
//  * A lane keeps (sum, windows, nonzero) per range of the sweep.  Integer adds only, so after
//    the last chunk a butterfly of adds over the lanes gives the same record in any order; lane
//    0 writes it with one 16-byte vector store.  A lane's sum stays below windows * 2^40 < 2^63
//    (the driver refuses a region of 2^23 bases).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "affinity_tables.hpp"
#include "hit_score.hpp"

namespace tfbs {
namespace {

// Ranges of one sweep.  The built kernel's registers (gfx950) are in DESIGN.md,
// "scan_affinity_kernel": a lane holds four registers per range against the best kernel's
// three, and 4 ranges stay at the best kernel's occupancy with nothing spilled.
constexpr int kAffRanges = 4;
constexpr uint32_t kAffTableLen = kAffT1Len + kAffT2Len;

typedef const __attribute__((address_space(4))) int32_t CTop;  // wave-uniform: a scalar load

struct AffArgs {
    PairSrc src;
    const int32_t *posrel;
    const DevRegion *regions;
    const int32_t *inner;
    const uint32_t *hap_ids;  // the chunk's haplotypes (batch indices)
    const uint64_t *hap_off;  // chunk haplotype k's first record: its n_strands x n_ranges follow
    const uint64_t *tables;   // T1 then T2
    const int32_t *tops;      // per strand: its pattern_id's reference score
    uint32_t n_haps;
    uint64_t rec_cap;
    DevAffRec *recs;
};

template <int NG>
struct AffLane {  // a lane's running sum and counts per range of the sweep
    uint64_t sum[NG];
    uint32_t n[NG], nz[NG];
};

// a(d) from the staged tables t (T1 then T2).
__device__ __forceinline__ uint64_t weight_of(const uint64_t *t, uint32_t d) {
    uint64_t a = 0;
    if (d <= kAffLast) {
        const uint32_t q = d / 1000u;
        a = __umul64hi(t[d - 1000u * q], t[kAffT1Len + q]) >> 22;
    }
    return a;
}

// NCH 64-window chunks from window c0: scored together, each existing window weighted once
// and added to the ranges of the sweep it overlaps (range_overlaps(inner, match), as
// best_chunks).  pos: the windows' starts (null: window i starts at i).
template <int NCH, int NG>
__device__ __forceinline__ void aff_chunks(const PairScan &P, const int32_t *pos, uint32_t c0, uint32_t lane,
                                           const uint64_t *t, int32_t top, const int32_t (&rs)[NG],
                                           const int32_t (&re)[NG], AffLane<NG> &b) {
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
        // top >= score and top - score < 2^32 as integers, so the wrapping difference is d
        const uint64_t a = weight_of(t, exists ? (uint32_t)top - s[c] : UINT32_MAX);
        const uint32_t nz = a ? 1u : 0u;
#pragma unroll
        for (int r = 0; r < NG; r++) {
            const bool ov = exists && ((rs[r] <= ms[c] && ms[c] <= re[r]) || (rs[r] <= me && me <= re[r]));
            b.sum[r] += ov ? a : 0ull;
            b.n[r] += ov ? 1u : 0u;
            b.nz[r] += ov ? nz : 0u;
        }
    }
}

// One sweep over the pair's windows for ranges [first, first + ng) of `inner` (ng <= NG; built
// for 1, 2 and kAffRanges ranges as the best sweep), then the reduction and the ng records
// from recs[rec].
template <int NG>
__device__ __forceinline__ void aff_sweep(const AffArgs &A, const PairScan &P, const int32_t *pos, uint32_t lane,
                                          const uint64_t *t, int32_t top, uint32_t first, uint32_t ng, uint64_t rec) {
    int32_t rs[NG], re[NG];
    AffLane<NG> b;
#pragma unroll
    for (int r = 0; r < NG; r++) {
        const bool have = (uint32_t)r < ng;  // (a range the group lacks overlaps nothing)
        const uint32_t at = 2 * (first + (have ? (uint32_t)r : 0u));
        rs[r] = __builtin_amdgcn_readfirstlane(have ? A.inner[at] : INT32_MAX);
        re[r] = __builtin_amdgcn_readfirstlane(have ? A.inner[at + 1] : INT32_MIN);
        b.sum[r] = 0;
        b.n[r] = b.nz[r] = 0;
    }
    WALK_CHUNKS(P.nwin, c0, (aff_chunks<NCH, NG>(P, pos, c0, lane, t, top, rs, re, b)));
#pragma unroll
    for (int r = 0; r < NG; r++) {
        if ((uint32_t)r >= ng) break;  // (wave-uniform)
        unsigned long long sum = b.sum[r];
        uint32_t n = b.n[r], nz = b.nz[r];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sum += (unsigned long long)__shfl_xor((long long)sum, m);
            n += (uint32_t)__shfl_xor((int)n, m);
            nz += (uint32_t)__shfl_xor((int)nz, m);
        }
        const uint64_t at = rec + (uint32_t)r;
        if (lane == 0 && at < A.rec_cap) A.recs[at] = DevAffRec{sum, n, nz};
    }
}

// Grid: ceil(n_haps * n_strands / kHitWaves) workgroups of kHitBlock threads.
__global__ __launch_bounds__(kHitBlock) void scan_affinity_kernel(AffArgs A) {
    __shared__ int32_t s_rows[kHitWaves][kHitDiInts];
    __shared__ uint64_t s_tab[kAffTableLen];
    for (uint32_t x = threadIdx.x; x < kAffTableLen; x += kHitBlock) s_tab[x] = A.tables[x];
    const PairHead H = pair_head(A.src, 0, A.n_haps, s_rows);  // (its barrier covers s_tab)
    if (!H.active) return;
    PAIR_OPEN(A.src, H, A.hap_ids, hid, hm, P);  // (nwin 0: every record is the empty one)
    const DevRegion rg = A.regions[hm.region];
    const uint32_t n_inner = __builtin_amdgcn_readfirstlane(rg.n_inner);
    const uint32_t inner_off = __builtin_amdgcn_readfirstlane(rg.inner_off);
    const int32_t *pos = (hm.flags & HAP_HAS_POS) ? A.posrel + hm.pos_off : nullptr;
    const uint32_t lane = H.lane;
    const int32_t top = ((CTop *)A.tops)[H.sidx];
    const uint64_t rec0 = A.hap_off[H.k] + (uint64_t)H.sidx * n_inner;
    for (uint32_t g0 = 0; g0 < n_inner; g0 += kAffRanges) {
        const uint32_t ng = min((uint32_t)kAffRanges, n_inner - g0);
        if (ng == 1) aff_sweep<1>(A, P, pos, lane, s_tab, top, inner_off + g0, ng, rec0 + g0);
        else if (ng == 2) aff_sweep<2>(A, P, pos, lane, s_tab, top, inner_off + g0, ng, rec0 + g0);
        else aff_sweep<kAffRanges>(A, P, pos, lane, s_tab, top, inner_off + g0, ng, rec0 + g0);
    }
}

}  // namespace

struct AffinityState : PairState {  // host: the tables, the tops and a chunk's records, copied back
    DevBuf<uint64_t> tables;
    DevBuf<int32_t> tops;
    uint32_t max_strands = 0;  // the most strands one pattern_id has
    DevBuf<uint64_t> hap_off;
    DevBuf<DevAffRec> recs;
    double ms[2] = {0, 0};
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

void affinity_last_ms(const AffinityState *s, double out[2]) {
    for (int k = 0; k < 2; k++) out[k] = s ? s->ms[k] : 0.0;
}

int affinity_run(AffinityState **state, int device, void *stream_, const Patterns &P, const ScanImage &img,
                 const Batch &B, size_t r0, size_t r1, std::vector<tfbs_affinity> *out) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, stream, 2, "affinity tables")) return rc;
    AffinityState &S = **state;
    S.ms[0] = S.ms[1] = 0;
    const uint64_t ns = S.n_strands;
    // the distinct haplotypes of [r0, r1) that have records, in order (as best_run)
    std::vector<uint32_t> ids;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        for (size_t k = 1; k < R.ranges.size(); k++)
            if (!(R.ranges[k - 1] < R.ranges[k])) return fail(TFBS_E_STATE, "inner ranges of a region not ascending");
        if (R.ranges.size() != B.regions[r].n_inner) return fail(TFBS_E_STATE, "inner ranges of a region not packed");
        if (R.ranges.empty()) continue;
        uint64_t longest = 0;
        for (uint32_t h = 0; h < R.hap_count; h++) {
            ids.push_back(R.hap_begin + h);
            longest = std::max<uint64_t>(longest, B.haps[R.hap_begin + h].len);
        }
        if (longest * S.max_strands >= (1ull << 23))
            return fail(TFBS_E_ARG, "region " + std::to_string(r) + ": its longest haplotype times the most strands of "
                                        "one pattern_id reaches 2^23: an affinity sum could pass 2^63");
    }
    if (ids.empty() || ns == 0) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, "too many strands for the affinity kernel");
    const uint64_t budget = scratch_budget("TFBS_AFFINITY_SCRATCH_MB", 256.0);  // read at the call
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
            if (nh && (nrec + add) * sizeof(DevAffRec) > budget) break;
            hap_off.push_back(nrec);
            nrec += add;
            nh++;
        }
        if ((rc = S.host.reserve(nrec * sizeof(DevAffRec))) || (rc = S.hap_ids.ensure_exact(nh)) ||
            (rc = S.hap_off.ensure_exact(nh)) || (rc = S.recs.ensure_exact(nrec)))
            return rc;
        HIP_TRY(hipMemcpyAsync(S.hap_ids.p, ids.data() + start, 4 * nh, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(S.hap_off.p, hap_off.data(), 8 * nh, hipMemcpyHostToDevice, stream));
        AffArgs A{};
        A.src = S.src(img);
        A.posrel = img.posrel;
        A.regions = img.regions;
        A.inner = img.inner;
        A.hap_ids = S.hap_ids.p;
        A.hap_off = S.hap_off.p;
        A.tables = S.tables.p;
        A.tops = S.tops.p;
        A.n_haps = (uint32_t)nh;
        A.rec_cap = nrec;
        A.recs = S.recs.p;
        HIP_TRY(hipEventRecord(S.ev[0], stream));
        hipLaunchKernelGGL(scan_affinity_kernel, dim3((uint32_t)((nh * ns + kHitWaves - 1) / kHitWaves)),
                           dim3(kHitBlock), 0, stream, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(S.ev[1], stream));
        HIP_TRY(hipEventSynchronize(S.ev[1]));  // (the host part's clock starts when the kernel is done)
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        S.ms[0] += ms;
        const double t0 = now_ms();
        HIP_TRY(hipMemcpyAsync(S.host.p, S.recs.p, nrec * sizeof(DevAffRec), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const DevAffRec *rec = reinterpret_cast<const DevAffRec *>(S.host.p);
        size_t at = out->size();
        out->resize(at + nrec);
        for (size_t k = 0; k < nh; k++) {
            const uint32_t id = ids[start + k];
            const DevHap &hm = B.haps[id];
            const RegionH &R = B.rh[hm.region];
            const uint32_t nr = (uint32_t)R.ranges.size();
            const DevAffRec *q = rec + hap_off[k];
            for (uint32_t p = 0; p < ns; p++)
                for (uint32_t x = 0; x < nr; x++, q++, at++)
                    (*out)[at] = tfbs_affinity{hm.region, id - R.hap_begin, p, x, q->n_windows, q->n_nonzero, q->sum};
        }
        S.ms[1] += now_ms() - t0;
        start += nh;
    }
    return TFBS_OK;
}

}  // namespace tfbs
