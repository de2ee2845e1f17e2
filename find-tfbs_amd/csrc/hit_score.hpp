// What the brute-force kernels (scan_hits.hip, scan_best.hip, scan_affinity.hip), the variant-effect kernel
// (scan_effects.hip: pair_head, the scoring, the drivers' base), the mutation-scan kernel
// (scan_mutscan.hip: pair_head_at, the scoring of one window, the drivers' base) and their drivers share.  A HIP
// header: only .hip sources include it.  What scan_best.hip and scan_affinity.hip share beyond it -- the
// range sweeps, the dense records' places, the chunk driver -- is range_sweep.hpp's, on top of this one.
//  * Device: the exact scoring code (bases16, score_mono, score_dinuc), the kernels' prologue
//    in two steps (pair_head, PAIR_OPEN), what a wave knows of its pair (PairScan) and the walk
//    over the pair's windows (WALK_CHUNKS, scored_window, SCORE_WINDOWS).  A kernel keeps what
//    it does with a chunk's scores.
//  * Host: the drivers' common state (PairState, first_use), the scratch budget.
//
// A wave owns one (haplotype, strand) pair; its lanes are 64 consecutive windows and it walks
// the 64-window chunks in ascending order.  A lane takes the bases of its window 16 at a time:
// two packed words and two N-mask words funnel-shifted to the window's phase.  It has up to
// four 64-window chunks' windows in flight: their words are loaded together and a column's
// weights are fetched once.  The strand is wave-uniform: a mono column's four weights come
// through one scalar load and three selects, a dinucleotide strand's rows (at most 31 x 16
// ints) sit in the wave's LDS slice, where the 16 entries of a row lie on 16 banks (lanes on
// one entry broadcast).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <string>

#include "hip_util.hpp"
#include "hits.hpp"
#include "scan.hpp"

namespace tfbs {

constexpr uint32_t kHitWaves = 4;                       // waves (pairs) per workgroup
constexpr uint32_t kHitBlock = 64 * kHitWaves;
constexpr int kHitChunks = 4;                           // 64-window chunks a lane has in flight
constexpr uint32_t kHitDiInts = (kDiMaxLen - 1) * 16;   // a dinucleotide strand's rows
constexpr uint64_t kHitsMaxPairs = 1ull << 30;          // pairs per launch: the grid stays below 2^31

typedef const __attribute__((address_space(4))) DevHitStrand CStrand;  // wave-uniform: scalar loads
struct alignas(16) Col4 {  // one mono column: [A,C,G,T]
    int32_t x, y, z, w;
};
typedef const __attribute__((address_space(4))) Col4 CInt4;

// The 16 bases from base q of a haplotype (2 bits each, base q lowest) and their N bits.
__device__ __forceinline__ void bases16(const uint32_t *W, const uint32_t *M, uint32_t q, uint32_t &bits,
                                        uint32_t &nm) {
    const uint32_t wi = q >> 4;
    bits = __builtin_amdgcn_alignbit(W[wi + 1], W[wi], 2 * (q & 15));
    nm = M ? __builtin_amdgcn_alignbit(M[(q >> 5) + 1], M[q >> 5], q & 31) : 0u;
}

// Wrapping column sums of the windows at bases i[0 .. NCH) (one per 64-window chunk in
// flight: their words are loaded together, a column's weights once); an N column adds 0.
template <int NCH>
__device__ __forceinline__ void score_mono(const uint32_t *W, const uint32_t *M, const uint32_t (&i)[NCH], uint32_t L,
                                           CInt4 *wq, uint32_t (&s)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; c++) s[c] = 0;
    for (uint32_t g = 0; g < L; g += 16) {  // (wave-uniform trip counts)
        uint32_t bits[NCH], nm[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) bases16(W, M, i[c] + g, bits[c], nm[c]);
        const uint32_t cnt = min(16u, L - g);
        for (uint32_t t = 0; t < cnt; t++) {
            CInt4 &w = wq[g + t];
            const int32_t wa = w.x, wc = w.y, wg = w.z, wt = w.w;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint32_t b = bits[c] & 3u;
                const int32_t v = b == 0 ? wa : b == 1 ? wc : b == 2 ? wg : wt;
                s[c] += (nm[c] & 1u) ? 0u : (uint32_t)v;
                bits[c] >>= 2;
                nm[c] >>= 1;
            }
        }
    }
}

// Wrapping pair sums of the windows at bases i[0 .. NCH) (L <= 32 bases); a pair holding an
// N adds 0.
template <int NCH>
__device__ __forceinline__ void score_dinuc(const uint32_t *W, const uint32_t *M, const uint32_t (&i)[NCH],
                                            uint32_t L, const int32_t *rows, uint32_t (&s)[NCH]) {
    uint32_t prev[NCH], prevn[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) s[c] = 0, prev[c] = 0, prevn[c] = 1;  // (no pair ends on the first base)
    for (uint32_t g = 0; g < L; g += 16) {
        uint32_t bits[NCH], nm[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) bases16(W, M, i[c] + g, bits[c], nm[c]);
        const uint32_t cnt = min(16u, L - g);
        for (uint32_t t = 0; t < cnt; t++) {
            const uint32_t j = g + t;  // the pair (base j - 1, base j) is row j - 1
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint32_t b = bits[c] & 3u, n = nm[c] & 1u;
                const int32_t v = j ? rows[16 * (j - 1) + 4 * prev[c] + b] : 0;
                s[c] += (n | prevn[c]) ? 0u : (uint32_t)v;
                prev[c] = b;
                prevn[c] = n;
                bits[c] >>= 2;
                nm[c] >>= 1;
            }
        }
    }
}

// A dinucleotide strand's rows into a wave's LDS slice (L <= kDiMaxLen: check_dipwm_length).
__device__ __forceinline__ void stage_dinuc_rows(int32_t *slice, const int32_t *weights, uint32_t w_off, uint32_t L,
                                                 uint32_t lane) {
    const uint32_t n = min((L - 1) * 16, kHitDiInts);
    for (uint32_t x = lane; x < n; x += 64) slice[x] = weights[w_off + x];
}

struct PairSrc {  // the tables and the batch image: the head of both kernels' arguments
    const DevHitStrand *strands;
    const int32_t *weights;
    uint32_t n_strands;
    const DevHap *haps;
    const uint32_t *words;
    const uint32_t *nmask;
};

struct PairHead {  // the prologue's first step (wave-uniform but lane)
    uint32_t lane;
    uint64_t pl, p;    // the wave's pair: of the launch, of the chunk
    bool active;       // the launch has a pair pl
    uint32_t k, sidx;  // p = chunk haplotype k * n_strands + strand sidx
    uint32_t kind, L, w_off;
    int32_t min_score;
    bool di;
    const int32_t *rows;  // the wave's LDS slice: a dinucleotide strand's rows
};

struct PairScan {  // what a wave knows of its pair to score it (wave-uniform)
    const uint32_t *W, *M;
    CInt4 *wq;
    const int32_t *rows;
    uint32_t L, nwin;
    bool di;
};

// The prologue up to and including the workgroup's barrier.  The launch takes the pairs of
// chunk haplotypes [k0, k1) (pairs are haplotype-major: the first is k0 * n_strands); the wave
// takes pair blockIdx.x * kHitWaves + wave of them, loads its strand through scalar loads and
// stages a dinucleotide strand's rows.  An inactive wave (the last workgroup's tail) takes the
// last pair, so that every wave of the workgroup reaches the barrier.  pair_head_at is the same
// for the chunk's pairs [p0, p0 + n_pairs), which need not be whole haplotypes (scan_mutscan.hip's
// fill pass).  The two share their body as a macro, for the reason given below.
#define PAIR_HEAD_BODY(T, N_PAIRS, P0, s_rows)                                                                  \
    const uint32_t lane = threadIdx.x & 63;                                                                     \
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                     \
    const uint64_t n_pairs = (N_PAIRS);                                                                         \
    const uint64_t pl = (uint64_t)blockIdx.x * kHitWaves + wave;                                                \
    const bool active = pl < n_pairs;                                                                           \
    const uint64_t p = (P0) + (active ? pl : n_pairs - 1);                                                      \
    const uint32_t k = (uint32_t)(p / (T).n_strands);                                                           \
    const uint32_t sidx = (uint32_t)(p - (uint64_t)k * (T).n_strands);                                          \
    CStrand &S = ((CStrand *)(T).strands)[sidx];                                                                \
    const uint32_t kind = S.kind, L = S.len, w_off = S.w_off;                                                   \
    const int32_t min_score = S.min_score;                                                                      \
    const bool di = kind == TFBS_KIND_DIPWM;                                                                    \
    if (di) stage_dinuc_rows((s_rows)[wave], (T).weights, w_off, L, lane); /* (L <= kDiMaxLen: check_dipwm_length) */ \
    __syncthreads();                                                                                            \
    return PairHead{lane, pl, p, active, k, sidx, kind, L, w_off, min_score, di, (s_rows)[wave]}
__device__ __forceinline__ PairHead pair_head(const PairSrc &T, uint32_t k0, uint32_t k1,
                                              int32_t (&s_rows)[kHitWaves][kHitDiInts]) {
    PAIR_HEAD_BODY(T, (uint64_t)(k1 - k0) * T.n_strands, (uint64_t)k0 * T.n_strands, s_rows);
}
__device__ __forceinline__ PairHead pair_head_at(const PairSrc &T, uint64_t p0, uint64_t np,
                                                 int32_t (&s_rows)[kHitWaves][kHitDiInts]) {
    PAIR_HEAD_BODY(T, np, p0, s_rows);
}

// The three pieces below are macros, not functions: a function is simplified on its own
// before it is inlined, and with any of them as one the built kernels differ from those of
// the code written out in each kernel (registers, occupancy, the branches around a chunk's
// second half).  Expanded in place they are that code.
//
// The prologue's second step, for a wave that goes on: declares the pair's haplotype (batch
// index `hid`, descriptor `hm`) and `const PairScan P` (and, on the way, `scored` and `nwin`).
// nwin 0: nothing to score.
#define PAIR_OPEN(T, H, hap_ids, hid, hm, P)                                                        \
    const uint32_t hid = (hap_ids)[(H).k];                                                          \
    const DevHap hm = (T).haps[hid];                                                                \
    const bool scored = (H).L != 0 && hm.len >= (H).L && ((H).kind == TFBS_KIND_PWM || (H).di);     \
    const uint32_t nwin = scored ? hm.len - (H).L + 1 : 0;                                          \
    const PairScan P {                                                                              \
        (T).words + hm.word_off, (hm.flags & HAP_HAS_N) ? (T).nmask + hm.nmask_off : nullptr,       \
            (CInt4 *)((T).weights + (H).w_off), (H).rows, (H).L, nwin, (H).di                       \
    }

// The walk over a pair's windows: BODY, a statement that uses the constant NCH, for NCH
// 64-window chunks from window c0, ascending.  A 3-chunk tail scores one chunk of window 0.
#define WALK_CHUNKS(nwin, c0, BODY)                                      \
    for (uint32_t c0 = 0; c0 < (nwin); c0 += 64 * kHitChunks) {          \
        const uint32_t nch = ((nwin) - c0 + 63) / 64;                    \
        if (nch >= 3) {                                                  \
            constexpr int NCH = kHitChunks;                              \
            BODY;                                                        \
        } else if (nch == 2) {                                           \
            constexpr int NCH = 2;                                       \
            BODY;                                                        \
        } else {                                                         \
            constexpr int NCH = 1;                                       \
            BODY;                                                        \
        }                                                                \
    }

// The chunk scorer: the scores s[] of the windows at bases ii[0 .. NCH) of pair P.
#define SCORE_WINDOWS(NCH, P, ii, s)                                             \
    do {                                                                         \
        if ((P).di) score_dinuc<NCH>((P).W, (P).M, ii, (P).L, (P).rows, s);      \
        else score_mono<NCH>((P).W, (P).M, ii, (P).L, (P).wq, s);                \
    } while (0)

// The window a lane scores in place of window i.
__device__ __forceinline__ uint32_t scored_window(const PairScan &P, uint32_t i) {
    return i < P.nwin ? i : 0;  // (window 0 exists: reads stay inside the haplotype's pads)
}

// What the drivers keep on a ctx: the pattern set's tables on the device (build_hit_tables),
// the chunk's haplotype list, the pinned buffer of the copy-back and the events.
struct PairState {
    DevBuf<DevHitStrand> strands;
    DevBuf<int32_t> weights;
    uint32_t n_strands = 0;
    DevBuf<uint32_t> hap_ids;
    PinnedBytes host;
    Event ev[3];
    // The tables uploaded and n_events events created; a failure reads "<label>: ...".
    int upload(const Patterns &P, hipStream_t stream, int n_events, const char *label) {
        HitTables T;
        build_hit_tables(P, &T);
        n_strands = (uint32_t)T.strands.size();
        int rc;
        if ((rc = strands.ensure_exact(T.strands.size())) || (rc = weights.ensure_exact(T.weights.size() + 4))) return rc;
        hipError_t e = hipSuccess;
        if (!T.strands.empty())
            e = hipMemcpyAsync(strands.p, T.strands.data(), T.strands.size() * sizeof(DevHitStrand),
                               hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && !T.weights.empty())
            e = hipMemcpyAsync(weights.p, T.weights.data(), T.weights.size() * 4, hipMemcpyHostToDevice, stream);
        for (int k = 0; k < n_events; k++)
            if (e == hipSuccess) e = ev[k].create();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);  // (T goes out of scope)
        return e == hipSuccess ? TFBS_OK : fail(TFBS_E_HIP, std::string(label) + ": " + hipGetErrorString(e));
    }
    PairSrc src(const ScanImage &img) const {
        return PairSrc{strands.p, weights.p, n_strands, img.haps, img.words, img.nmask};
    }
};

// A driver's state (a PairState and its own buffers) on its first call: made, its tables
// uploaded; a failure deletes it and leaves *state null, so the next call tries again.
template <typename S>
int first_use(S **state, const Patterns &P, hipStream_t stream, int n_events, const char *label) {
    if (*state) return TFBS_OK;
    S *s = new S();
    if (int rc = s->upload(P, stream, n_events, label)) {
        delete s;
        return rc;
    }
    *state = s;
    return TFBS_OK;
}

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace tfbs
