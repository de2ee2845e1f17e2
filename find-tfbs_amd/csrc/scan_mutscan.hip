// MI355X (gfx950) mutation-scan kernel: per (region, pattern strand, column c of the region's
// reference window R, base b != R[c]) the best score among the windows covering c on R and on
// R with column c set to b, the lowest window attaining each, and the record's kind under the
// strand's min_score (include/tfbs_amd.h, "Mutation scan"): the effect record of that SNV,
// for every SNV there is.
//
// A substitution changes one column, so the alt score of a window is its reference score plus
// one weight difference (two pair-weight differences for a dinucleotide strand): the whole
// scan costs about four hit scans, not 3 L of them.
//
//  * The pair a wave owns (pair_head_at), the scoring of a reference window (score_mono<1>,
//    score_dinuc<1>) and the drivers' base (PairState) are hit_score.hpp's; the host packing
//    (pack_seq.hpp) is shared with scan_effects.hip.  A pair is (chunk region, strand),
//    region-major.
//  * The wave walks R's columns in ascending 64-column chunks.  In chunk c0 lane l scores
//    reference window c0 + l once and stores it in the wave's ring of kMutRing scores in LDS:
//    the ring then holds windows c0 - 64 .. c0 + 63, which the columns c0 .. c0 + 63 reach
//    under a strand of up to kMutRingMax = 65 bases.  Lane l then owns column c = c0 + l and
//    loops j = 0 .. L - 1 (wave-uniform): window i = c - j, valid iff 0 <= i <= n - L, read
//    from the ring (consecutive lanes, consecutive dwords), gives the four scores
//    s - w[j][R[c]] + w[j][b] in wrapping uint32; b == R[c] is the reference side.  j
//    ascending is i descending, so replacing on >= leaves the lowest window on ties.  The
//    waves of a workgroup have different trip counts: no barrier inside the walk, the wave's
//    own LDS writes and reads are ordered by a wavefront-scope fence.
//  * A strand longer than the ring serves (mono only: a dinucleotide strand has at most 32
//    bases) takes the slow path: column by column, the lanes are the column's windows in
//    64-lane chunks, each rescored on R and shifted by its weight difference, and a butterfly
//    takes the best as scan_effects.hip does.  n min(L, n - L + 1) L column operations per pair.
//  * Two passes run the same code (scan_mutscan_kernel<FILL>).  A lane has up to three records
//    per chunk; three ballots and mbcnt give its rank, a running wave total the chunk's base.
//    The count pass stores one u64 per pair, exclusive_scan makes offsets, the fill pass
//    re-walks the pairs with a count.  Sorted by (region, pattern, column, alt base) without an
//    atomic, a fixed-capacity list or a sort.
//  * Lanes past the last column / window take column 0 / window 0 and are masked: reads stay
//    inside the sequence's pads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hit_score.hpp"
#include "pack_seq.hpp"

namespace tfbs {
namespace {

constexpr uint32_t kMutRing = 128;  // scores per wave: a chunk's 64 windows and the 64 before them
static_assert((kMutRing & (kMutRing - 1)) == 0 && kMutRingMax - 1 + 64 <= kMutRing, "the ring serves kMutRingMax");

struct MutArgs {
    PairSrc src;  // the tables; words / nmask: the chunk's packed image (haps unused)
    const DevMutRegion *regs;
    // pair p = chunk region k * n_strands + strand.  The count pass stores the pair's records at
    // off[p]; after the exclusive scan over the chunk's pairs + 1 values, off[p] is the pair's
    // first record and the last value the chunk's total
    uint64_t *off;
    uint64_t p0, n_pairs;  // the chunk's pairs this launch takes
    uint64_t n_chunk;      // pairs in the chunk (count pass: the total's slot is zeroed)
    uint32_t kinds;
    // fill pass: record off[p] - rec_base of recs (rec_cap entries)
    uint64_t rec_base, rec_cap;
    DevMutRec *recs;
};

template <typename T>
__device__ __forceinline__ T pick(const T (&a)[4], uint32_t i) {  // (selects: no indexed registers)
    return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3];
}

// The effects TSV's kind: 0 gain, 1 loss, 2 change, 3 same, 4 none.
__device__ __forceinline__ uint32_t mut_kind(int32_t ref, int32_t alt, int32_t min_score) {
    const bool pr = ref > min_score, pa = alt > min_score;
    return pa && !pr ? 0u : pr && !pa ? 1u : !pr ? 4u : ref != alt ? 2u : 3u;
}

// Orders the wave's own LDS accesses before the fence with those after it.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct MutPair {  // a record's fields besides the column's, and the threshold
    uint32_t k, sidx, kinds;
    int32_t min_score;
};

// A column's records: b ascending among the three bases other than r, each kept iff its kind
// is asked for.  e[t], kd[t], alt b[t]: slot t.
struct MutCol {
    bool e[3];
    uint32_t kd[3], b[3];
    int32_t ref_score;
    uint32_t ref_window;
};
__device__ __forceinline__ MutCol column_records(const MutPair &Q, bool col, uint32_t r, const int32_t (&sc)[4],
                                                 const uint32_t (&wi)[4]) {
    MutCol C;
    C.ref_score = pick(sc, r);
    C.ref_window = pick(wi, r);
#pragma unroll
    for (uint32_t t = 0; t < 3; t++) {
        C.b[t] = t + (t >= r ? 1u : 0u);
        C.kd[t] = mut_kind(C.ref_score, pick(sc, C.b[t]), Q.min_score);
        C.e[t] = col && ((Q.kinds >> C.kd[t]) & 1u);
    }
    return C;
}

__device__ __forceinline__ void store_record(const MutArgs &A, const MutPair &Q, uint64_t at, uint32_t c, uint32_t r,
                                             const MutCol &C, uint32_t t, int32_t alt_score, uint32_t alt_window) {
    if (at < A.rec_cap)
        A.recs[at] = DevMutRec{Q.k, Q.sidx, c, r | C.b[t] << 8 | C.kd[t] << 16, C.ref_score, C.ref_window, alt_score,
                               alt_window};
}

// The ring path: a strand of up to kMutRingMax bases.
template <bool FILL>
__device__ __forceinline__ void walk_ring(const MutArgs &A, const PairScan &P, const MutPair &Q, uint32_t n,
                                          uint32_t lane, int32_t *ring, uint64_t &at) {
    const uint32_t L = P.L;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        if (c0 < P.nwin) {  // (wave-uniform) the chunk's reference windows, each scored once
            const uint32_t i = c0 + lane;
            const uint32_t ii[1] = {scored_window(P, i)};
            uint32_t s[1];
            SCORE_WINDOWS(1, P, ii, s);
            ring[i & (kMutRing - 1)] = (int32_t)s[0];
        }
        wave_lds_fence();
        const uint32_t c = c0 + lane;
        const bool in = c < n;
        const uint32_t ce = in ? c : 0;  // (column 0 exists: reads stay inside the sequence)
        // the column's base r, its left neighbour p and its right neighbour q
        const uint32_t sh = ce ? 1u : 0u;
        uint32_t bits, nm;
        bases16(P.W, P.M, ce - sh, bits, nm);
        const uint32_t p = bits & 3u, r = (bits >> (2 * sh)) & 3u, q = (bits >> (2 * sh + 2)) & 3u;
        const bool p_n = !sh || (nm & 1u), q_n = ce + 1 >= n || ((nm >> (sh + 1)) & 1u);
        const bool col = in && !((nm >> sh) & 1u);  // an N column has no substitutions
        int32_t sc[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
        uint32_t wi[4] = {UINT32_MAX, UINT32_MAX, UINT32_MAX, UINT32_MAX};
        bool seen = false;
        for (uint32_t j = 0; j < L; j++) {  // (wave-uniform) window c - j has the column at its base j
            const uint32_t i = ce - j;
            const bool ok = col && j <= ce && i < P.nwin;
            const uint32_t s = (uint32_t)ring[i & (kMutRing - 1)];
            uint32_t a[4];
            if (P.di) {
                uint32_t d[4] = {0u, 0u, 0u, 0u};
                if (j >= 1) {  // the pair (p, column): row j - 1
                    const int32_t *row = P.rows + 16 * (j - 1) + 4 * p;
                    const int32_t x[4] = {row[0], row[1], row[2], row[3]};
                    const uint32_t xr = (uint32_t)pick(x, r);
#pragma unroll
                    for (int b = 0; b < 4; b++) d[b] += p_n ? 0u : (uint32_t)x[b] - xr;
                }
                if (j + 1 < L) {  // the pair (column, q): row j
                    const int32_t *row = P.rows + 16 * j + q;
                    const int32_t x[4] = {row[0], row[4], row[8], row[12]};
                    const uint32_t xr = (uint32_t)pick(x, r);
#pragma unroll
                    for (int b = 0; b < 4; b++) d[b] += q_n ? 0u : (uint32_t)x[b] - xr;
                }
#pragma unroll
                for (int b = 0; b < 4; b++) a[b] = s + d[b];
            } else {
                CInt4 &w = P.wq[j];
                const int32_t x[4] = {w.x, w.y, w.z, w.w};
                const uint32_t base = s - (uint32_t)pick(x, r);
#pragma unroll
                for (int b = 0; b < 4; b++) a[b] = base + (uint32_t)x[b];
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {  // i descends: >= leaves the lowest window on ties
                const bool better = ok && (int32_t)a[b] >= sc[b];
                sc[b] = better ? (int32_t)a[b] : sc[b];
                wi[b] = better ? i : wi[b];
            }
            seen |= ok;
        }
        wave_lds_fence();  // (the next chunk's scores overwrite slots read above)
        const MutCol C = column_records(Q, seen, r, sc, wi);
        uint32_t lower = 0, total = 0, own = 0;
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const uint64_t mask = __ballot(C.e[t]);
            lower = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, lower));
            total += (uint32_t)__popcll(mask);
        }
        if (FILL) {
#pragma unroll
            for (uint32_t t = 0; t < 3; t++) {
                if (C.e[t]) store_record(A, Q, at + lower + own, c, r, C, t, pick(sc, C.b[t]), pick(wi, C.b[t]));
                own += C.e[t] ? 1u : 0u;
            }
        }
        at += total;
    }
}

// The slow path: a mono strand longer than the ring serves.
template <bool FILL>
__device__ __forceinline__ void walk_slow(const MutArgs &A, const PairScan &P, const MutPair &Q, uint32_t n,
                                          uint32_t lane, const Col4 *wv, uint64_t &at) {
    const uint32_t L = P.L;
    for (uint32_t c = 0; c < n; c++) {  // (wave-uniform)
        uint32_t bits, nm;
        bases16(P.W, P.M, c, bits, nm);
        const uint32_t r = __builtin_amdgcn_readfirstlane(bits & 3u);
        if (__builtin_amdgcn_readfirstlane(nm & 1u)) continue;  // an N column has no substitutions
        const uint32_t lo = c + 1 > L ? c + 1 - L : 0, hi = min(c, n - L);  // the column's windows
        int32_t sc[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
        uint32_t wi[4] = {UINT32_MAX, UINT32_MAX, UINT32_MAX, UINT32_MAX};
        for (uint32_t t0 = lo; t0 <= hi; t0 += 64) {
            const uint32_t i = t0 + lane;
            const bool mine = i <= hi;
            const uint32_t ii[1] = {mine ? i : lo};
            uint32_t s[1];
            score_mono<1>(P.W, P.M, ii, L, P.wq, s);
            const Col4 w = wv[c - ii[0]];
            const int32_t x[4] = {w.x, w.y, w.z, w.w};
            const uint32_t base = s[0] - (uint32_t)pick(x, r);
#pragma unroll
            for (int b = 0; b < 4; b++) {  // a lane's windows ascend: > leaves the lowest on ties
                const int32_t a = (int32_t)(base + (uint32_t)x[b]);
                const bool better = mine && (wi[b] == UINT32_MAX || a > sc[b]);
                sc[b] = better ? a : sc[b];
                wi[b] = better ? ii[0] : wi[b];
            }
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {  // the best over the lanes, the lowest window on ties
            long long key = (long long)(((unsigned long long)(uint32_t)sc[b] << 32) | (0xFFFFFFFFu - wi[b]));
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const long long o = __shfl_xor(key, m);
                key = o > key ? o : key;
            }
            sc[b] = (int32_t)(key >> 32);
            wi[b] = 0xFFFFFFFFu - (uint32_t)key;
        }
        const MutCol C = column_records(Q, true, r, sc, wi);
        uint32_t own = 0;
#pragma unroll
        for (uint32_t t = 0; t < 3; t++) {
            if (FILL && C.e[t] && lane == t) store_record(A, Q, at + own, c, r, C, t, pick(sc, C.b[t]), pick(wi, C.b[t]));
            own += C.e[t] ? 1u : 0u;
        }
        at += own;
    }
}

// Grid: ceil(n_pairs / kHitWaves) workgroups of kHitBlock threads.
template <bool FILL>
__global__ __launch_bounds__(kHitBlock) void scan_mutscan_kernel(MutArgs A) {
    __shared__ __attribute__((aligned(16))) int32_t s_rows[kHitWaves][kHitDiInts];
    __shared__ int32_t s_ring[kHitWaves][kMutRing];
    const PairHead H = pair_head_at(A.src, A.p0, A.n_pairs, s_rows);
    if (!H.active) return;
    if (!FILL && H.pl == 0 && H.lane == 0) A.off[A.n_chunk] = 0;  // the total's slot
    if (FILL && A.off[H.p + 1] == A.off[H.p]) return;  // the count pass found no record: nothing to place
    const DevMutRegion d = A.regs[H.k];
    const uint32_t n = d.len;
    const bool scored = H.L != 0 && n >= H.L && (H.kind == TFBS_KIND_PWM || H.di);
    uint64_t at = FILL ? A.off[H.p] - A.rec_base : 0;  // records of the pair so far (fill: their place)
    if (scored) {
        const PairScan P{A.src.words + d.word_off, d.has_n ? A.src.nmask + d.nmask_off : nullptr,
                         (CInt4 *)(A.src.weights + H.w_off), H.rows, H.L, n - H.L + 1, H.di};
        const MutPair Q{H.k, H.sidx, A.kinds, H.min_score};
        if (H.L <= kMutRingMax)
            walk_ring<FILL>(A, P, Q, n, H.lane, s_ring[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)], at);
        else if (!H.di)
            walk_slow<FILL>(A, P, Q, n, H.lane, reinterpret_cast<const Col4 *>(A.src.weights + H.w_off), at);
    }
    if (!FILL && H.lane == 0) A.off[H.p] = at;
}

}  // namespace

struct MutscanState : PairState {  // host: a chunk's image, counters and records
    DevBuf<uint32_t> image;  // the chunk's descriptors, words and N-mask words: one upload
    DevBuf<uint64_t> off, tmp;
    DevBuf<DevMutRec> recs;
    double ms[4] = {0, 0, 0, 0};
};

void mutscan_state_destroy(MutscanState *s) { delete s; }

void mutscan_last_ms(const MutscanState *s, double out[4]) {
    for (int k = 0; k < 4; k++) out[k] = s ? s->ms[k] : 0.0;
}

int mutscan_run(MutscanState **state, int device, void *stream_, const Patterns &P, const Batch &B, size_t r0, size_t r1,
                uint32_t kinds, std::vector<tfbs_mutation> *out, uint64_t *total) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    *total = 0;
    if (!B.keep_variants) return fail(TFBS_E_STATE, "batch built without tfbs_batch_keep_variants");
    if (B.kept.size() != B.rh.size()) return fail(TFBS_E_STATE, "kept variants out of step with the regions");
    HIP_TRY(hipSetDevice(device));
    if (int rc = first_use(state, P, stream, 2, "mutation-scan tables")) return rc;
    MutscanState &S = **state;
    for (double &m : S.ms) m = 0;
    const uint64_t ns = S.n_strands;
    if (ns == 0 || r0 == r1) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, "too many strands for the mutation-scan kernel");
    const uint64_t budget = scratch_budget("TFBS_MUTSCAN_SCRATCH_MB", 256.0);  // read at the call
    const uint64_t max_regs = std::max<uint64_t>(1, kHitsMaxPairs / ns);
    double t_prep = now_ms();

    size_t first = r0;  // the chunk's first region
    std::vector<PosRuns> pos_rs;
    std::vector<DevMutRegion> regs;
    std::vector<uint32_t> words, nmask, image;
    std::vector<uint64_t> offs;
    int rc = TFBS_OK;

    // a chunk's scratch besides its records: the image, the pairs' counters / offsets (u64: the
    // scan works in place) and the scan's tile sums
    auto fixed_bytes = [&](uint64_t nreg, uint64_t nw, uint64_t nm) {
        const uint64_t np = nreg * ns + 1;
        return 4 * (nw + nm) + nreg * sizeof(DevMutRegion) + 8 * np + 8 * scan_tmp_words(np);
    };

    auto flush = [&]() -> int {
        const size_t nreg = regs.size();
        if (!nreg) return TFBS_OK;
        const uint64_t np = nreg * ns + 1;
        // one image: the descriptors, then the words, then the N-mask words
        const size_t w0 = nreg * (sizeof(DevMutRegion) / 4), m0 = w0 + words.size();
        image.resize(m0 + nmask.size());
        memcpy(image.data(), regs.data(), nreg * sizeof(DevMutRegion));
        if (!words.empty()) memcpy(image.data() + w0, words.data(), 4 * words.size());
        if (!nmask.empty()) memcpy(image.data() + m0, nmask.data(), 4 * nmask.size());
        if ((rc = S.image.ensure_exact(image.size())) || (rc = S.off.ensure_exact(np)) ||
            (rc = S.tmp.ensure_exact(scan_tmp_words(np))) || (rc = S.host.reserve(8 * np)))
            return rc;
        S.ms[0] += now_ms() - t_prep;
        HIP_TRY(hipMemcpyAsync(S.image.p, image.data(), 4 * image.size(), hipMemcpyHostToDevice, stream));
        MutArgs A{};
        A.src = PairSrc{S.strands.p, S.weights.p, S.n_strands, nullptr, S.image.p + w0, S.image.p + m0};
        A.regs = reinterpret_cast<const DevMutRegion *>(S.image.p);
        A.off = S.off.p;
        A.p0 = 0;
        A.n_pairs = A.n_chunk = np - 1;
        A.kinds = kinds;
        HIP_TRY(hipEventRecord(S.ev[0], stream));
        hipLaunchKernelGGL(scan_mutscan_kernel<false>, dim3((uint32_t)((np - 1 + kHitWaves - 1) / kHitWaves)),
                           dim3(kHitBlock), 0, stream, A);
        HIP_TRY(hipGetLastError());
        if ((rc = exclusive_scan(S.off.p, np, S.tmp.p, stream))) return rc;
        HIP_TRY(hipEventRecord(S.ev[1], stream));
        HIP_TRY(hipEventSynchronize(S.ev[1]));  // (the host part's clock starts when the kernels are done)
        double t0 = now_ms();
        HIP_TRY(hipMemcpyAsync(S.host.p, S.off.p, 8 * np, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        S.ms[1] += ms;
        offs.resize(np);
        memcpy(offs.data(), S.host.p, 8 * np);
        *total += offs[np - 1];
        // the records, in runs of whole pairs that fit what the image and the counters leave (one at least)
        const uint64_t fixed = fixed_bytes(nreg, words.size(), nmask.size());
        const uint64_t room = budget > fixed ? (budget - fixed) / sizeof(DevMutRec) : 0;
        for (uint64_t q0 = 0; out && q0 < np - 1;) {
            uint64_t q1 = q0 + 1;
            while (q1 < np - 1 && offs[q1 + 1] - offs[q0] <= room) q1++;
            const uint64_t nrec = offs[q1] - offs[q0];
            if (nrec) {
                S.ms[3] += now_ms() - t0;
                if ((rc = S.recs.ensure_exact(nrec)) || (rc = S.host.reserve(nrec * sizeof(DevMutRec)))) return rc;
                A.p0 = q0;
                A.n_pairs = q1 - q0;
                A.rec_base = offs[q0];
                A.rec_cap = nrec;
                A.recs = S.recs.p;
                HIP_TRY(hipEventRecord(S.ev[0], stream));
                hipLaunchKernelGGL(scan_mutscan_kernel<true>, dim3((uint32_t)((q1 - q0 + kHitWaves - 1) / kHitWaves)),
                                   dim3(kHitBlock), 0, stream, A);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(S.ev[1], stream));
                HIP_TRY(hipEventSynchronize(S.ev[1]));
                t0 = now_ms();
                HIP_TRY(hipMemcpyAsync(S.host.p, S.recs.p, nrec * sizeof(DevMutRec), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
                S.ms[2] += ms;
                const DevMutRec *q = reinterpret_cast<const DevMutRec *>(S.host.p);
                const size_t base = out->size();
                out->resize(base + nrec);
                for (uint64_t x = 0; x < nrec; x++, q++) {
                    if (q->region >= nreg || q->pattern >= ns || q->column >= regs[q->region].len)
                        return fail(TFBS_E_STATE, "mutation scan: a device record out of range");
                    const PosRuns &pr = pos_rs[q->region];
                    const uint32_t n = regs[q->region].len, L = P.pats[q->pattern].len, c = q->column;
                    tfbs_mutation &o = (*out)[base + x];
                    o.region = (uint32_t)(first + q->region);
                    o.column = c;
                    o.pattern = q->pattern;
                    o.ref = (uint8_t)(q->rak & 0xFF);
                    o.alt = (uint8_t)((q->rak >> 8) & 0xFF);
                    o.kind = (uint8_t)((q->rak >> 16) & 0xFF);
                    o.reserved = 0;
                    o.pos = pos_at(pr, c);
                    o.n_windows = std::min(c, n - L) - (c + 1 > L ? c + 1 - L : 0) + 1;
                    o.ref_score = q->ref_score;
                    o.ref_window = q->ref_window;
                    o.alt_score = q->alt_score;
                    o.alt_window = q->alt_window;
                    o.reserved1 = 0;
                    o.ref_end = (o.ref_start = pos_at(pr, std::min(q->ref_window, n - 1))) + L - 1;
                    o.alt_end = (o.alt_start = pos_at(pr, std::min(q->alt_window, n - 1))) + L - 1;
                }
            }
            q0 = q1;
        }
        S.ms[3] += now_ms() - t0;
        first += nreg;
        pos_rs.clear();
        regs.clear();
        words.clear();
        nmask.clear();
        t_prep = now_ms();
        return TFBS_OK;
    };

    std::vector<uint8_t> nuc;
    const std::vector<const Record *> none;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        const KeptRegion &K = B.kept[r];
        nuc.clear();
        PosRuns pos;
        if ((rc = patch_runs(R.es, R.ee, none, K.ref.data(), R.es, K.ref.size(), nuc, pos))) return rc;
        const uint32_t n = pos.n;
        const bool any_n = has_n(nuc);
        const size_t w_add = 2 * (size_t)mask_words(n), m_add = any_n ? mask_words(n) : 0;
        if (!regs.empty() && (fixed_bytes(regs.size() + 1, words.size() + w_add, nmask.size() + m_add) > budget ||
                              regs.size() >= max_regs || words.size() + w_add > (1ull << 31))) {
            if ((rc = flush())) return rc;
        }
        DevMutRegion d{};
        d.word_off = (uint32_t)words.size();
        d.nmask_off = (uint32_t)nmask.size();
        d.len = n;
        d.has_n = any_n ? 1u : 0u;
        words.resize(words.size() + w_add);
        if (any_n) nmask.resize(nmask.size() + m_add);
        pack_seq(nuc, words.data() + d.word_off, any_n ? nmask.data() + d.nmask_off : nullptr);
        regs.push_back(d);
        pos_rs.push_back(std::move(pos));
    }
    if ((rc = flush())) return rc;
    S.ms[0] += now_ms() - t_prep;
    return TFBS_OK;
}

}  // namespace tfbs
