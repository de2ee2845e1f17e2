// Matrix-core scan (gfx950 v_mfma_scale_f32_32x32x64_f8f6f4, FP6 x FP4) for
// strands with L <= 32 (mfma.cpp).
//
// matches (pattern.rs:141-171) scores every window i of a haplotype with
// sum_j w[j][nuc(i + j)] (N = 0, pattern.rs:119-135).  For 32 windows x a set of
// strands that is a GEMM: the strands' weights times the windows' one-hot bases
// (all zero for N).  The kernel runs it on FP6 digits q <= 0 of an upper bound
// (score <= C + s Q, mfma.cpp) with the one-hot in FP4, at the matrix cores'
// FP4/FP6 rate.  U = 8 Q > T0 is necessary for a hit; those candidate windows are
// rescored exactly from the strand's integer weights.
//
//  * Two strands per GEMM row: the K chunk of 64 holds 8 columns of strand 2n (K
//    block 0) and of strand 2n + 1 (K block 1); A = the digits (scale 2^3: digits x 8
//    = integers; block 1 2^14: the field one up), B = the window's one-hot in both
//    blocks, and the accumulator starts at 2^23 + (1023 - T0) (1 + 2^11).  Every
//    output is an integer in [2^23, 2^24) (exact in f32) whose mantissa holds V = U +
//    1023 - T0 of strand 2n in bits 0-10 and of strand 2n + 1 in bits 11-21, each in
//    [0, 2048) (mfma.cpp clips the digits so); U > T0 iff the field's top bit (10 or
//    21) is set.  One OR tree over a lane's 16 outputs (v_or3 + v_bitop3) tests 32
//    (window, strand) pairs.
//  * One kernel family, scan_mfma_all_kernel<STAGED, UNIT>, one launch per scan: a
//    workgroup (8 waves) takes one haplotype group, or a unit of up to kMMaxUnit
//    consecutive groups, and stages the one-hot table, the haplotype descriptors and
//    (STAGED) packed words in LDS once, then every super tile (tiles of 64 strands of
//    one depth class) in turn.  Every digit fragment is one conflict-free
//    ds_read_b128 + ds_read_b64 per lane and feeds two window tiles.
//  * Window tiles come from the group's window list (build_window_lists): 32
//    listed windows of any of the group's haplotypes per tile, lane l & 31 its
//    own (haplotype, window), so reference-window reuse leaves no holes.
//  * C layout: lane l holds column l & 31 -- the window of its own list entry --
//    and strand pairs (r & 3) + 8 (r >> 2) + 4 (l >> 5), r < 16.  A firing lane
//    (a candidate among its 32 strands) queues a self-contained record (its
//    fields' top bits, its window's list entry, the strand tile) in LDS; the wave
//    decodes its records in batches into (haplotype, strand, window) candidates
//    (drain_queue: no global load); when the wave has scanned
//    it rescores those exactly, one per lane (pattern.rs:125-151), applies the
//    inner-range overlap test (range.rs:18-21 as main.rs:503 uses it) and appends
//    one (haplotype, key) pair per hit and overlapped range to its part of the
//    group's hit list (no count matrix, no atomics: the key assembly,
//    key_kernels.hip, counts them per region); a full wave list spills to a
//    launch-wide list rescored after the scan.
//  * After the scan: the overflow candidates' rescoring and the spill records'
//    bucketing by region (post_scan_kernel, or fused into the scan's last
//    workgroup).  The window lists are built in window_lists.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "scan.hpp"

namespace tfbs {
namespace {


typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kMBlock = 512;          // 8 waves (two per SIMD) share one super tile image
static_assert(kMBlock / 64 == kMBlockWaves, "hit list parts per workgroup");
constexpr int kMOnehotBytes = 2048;   // LDS: one-hot table (4-mer -> 4 x 16 bits of FP4), image, words
constexpr uint32_t kMChunkBytes = 1536;  // one K chunk's B fragments of a 64-strand tile (dwords 0-3 | 4-5)
constexpr uint32_t kMStagedMax = 80 * 1024;  // LDS per workgroup at 2 workgroups per CU (160 KiB)
constexpr uint32_t kTestMask = (1u << (kMFieldBits - 1)) | (1u << (2 * kMFieldBits - 1));  // the fields' top bits
constexpr uint32_t kQueueBits = 0x20200404u;  // those bits after queue_tile's byte permute (outputs 2j, 2j + 1)
// e8m0 scales: the digits x 8 (K block 0), x 2^(3 + 11) (block 1: the field one up); the one-hot x 1
constexpr int kScaleD0 = 130, kScaleD1 = 130 + kMFieldBits, kScaleOnehot = 127;

// A lane's haplotype (the group's descriptors are staged in LDS, s_hd).
struct LaneHap {
    uint32_t word_off, len, flags, nmask_off;
};

// The packed words (and N-mask words) a lane needs for its window i (read one
// pair of tiles ahead of use).
struct WinWords {
    uint32_t w[3], m[2];
};

__device__ __forceinline__ void load_window(const ScanArgs &A, const uint32_t *words, const LaneHap &hm, uint32_t i,
                                            WinWords &ww) {
    const uint32_t ic = min(i, hm.len);  // reads stay inside the +3 word pad
    const uint32_t *w = words + hm.word_off + (ic >> 4);
    ww.w[0] = w[0];
    ww.w[1] = w[1];
    ww.w[2] = w[2];
    if (hm.flags & HAP_HAS_N) {
        const uint32_t *m = A.nmask + hm.nmask_off + (ic >> 5);
        ww.m[0] = m[0];
        ww.m[1] = m[1];
    } else {
        ww.m[0] = ww.m[1] = 0;
    }
}

// A fragments of the lane's window i: chunk kc = columns 8 kc .. + 7 as FP4
// one-hot nibbles (1.0 at the base's position, 16 bits per column; the same in
// both lane halves, which the A scales tell apart), two 4-mer table reads; N
// bases zeroed in haplotypes that have them.
template <int NK>
__device__ __forceinline__ void build_onehot(const LaneHap &hm, uint32_t i, const WinWords &ww, const char *s_onehot,
                                             v4i (&a)[NK]) {
    const uint32_t ic = min(i, hm.len);
    const uint32_t sh = 2 * (ic & 15);
    const uint32_t img_lo = __builtin_amdgcn_alignbit(ww.w[1], ww.w[0], sh);  // bases i .. i+15
    const uint32_t img_hi = __builtin_amdgcn_alignbit(ww.w[2], ww.w[1], sh);  // bases i+16 .. i+31
    const uint2 *tab = reinterpret_cast<const uint2 *>(s_onehot);
#pragma unroll
    for (int kc = 0; kc < NK; kc++) {
        const uint32_t img = kc < 2 ? img_lo : img_hi;
        const uint32_t b0 = 16 * (kc & 1);
        const uint2 x = tab[__builtin_amdgcn_ubfe(img, b0, 8)], y = tab[__builtin_amdgcn_ubfe(img, b0 + 8, 8)];
        a[kc] = v4i{(int)x.x, (int)x.y, (int)y.x, (int)y.y};
    }
    // Bases past the haplotype end need no mask: they only reach windows with
    // i + L > len (rejected when the candidate is rescored) or columns >= L
    // (zero digits).
    if (hm.flags & HAP_HAS_N) {  // N scores 0 (pattern.rs:119-135): clear its one-hot
        const uint32_t vm = ~__builtin_amdgcn_alignbit(ww.m[1], ww.m[0], ic & 31);
#pragma unroll
        for (int kc = 0; kc < NK; kc++)
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const uint32_t keep = ((vm >> (8 * kc + 2 * d)) & 1u ? 0xFFFFu : 0u) |
                                      ((vm >> (8 * kc + 2 * d + 1)) & 1u ? 0xFFFF0000u : 0u);
                a[kc][d] &= keep;
            }
    }
}

// B fragments of one strand tile: chunk kc's 32 FP6 digits per lane (192
// bits) as dwords 0-3 (at kc * 1536 + lane * 16) and dwords 4-5 (at kc * 1536 +
// 1024 + lane * 8), mfma_tile_bytes per tile: conflict-free reads.
struct BFrag {
    v4i b;
    int2 c;
};

template <int D>
__device__ __forceinline__ void load_frags(const char *tile, uint32_t lane, BFrag (&f)[D]) {
#pragma unroll
    for (int kc = 0; kc < D; kc++) {
        // no ds_read2 merging across chunks: merged pairs need v_mov copies
        // into the MFMA operand tuples
        if (kc) asm volatile("" ::: "memory");
        f[kc].b = *reinterpret_cast<const v4i *>(tile + kc * 1536 + lane * 16);
        f[kc].c = *reinterpret_cast<const int2 *>(tile + kc * 1536 + 1024 + lane * 8);
    }
}

// One chunk: FP6 digits (A: rows = the tile's 32 strand pairs) x FP4 one-hot (B:
// columns = the tile's 32 windows), f32 accumulate; sa: the lane's A scale (digits x 8,
// x 2^14 for the pair's second strand, K block 1), B scale 1.  (A and B have the same
// lane layout -- lane l: row / column l & 31, K block l >> 5 -- so the image and the
// one-hot serve either operand; with the windows as columns a lane's 16 outputs are 16
// strand pairs of ONE window, the window of its own list entry.)
__device__ __forceinline__ v16f mfma_chunk(const v4i &a, const BFrag &f, const v16f &acc, int sa) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{f.b[0], f.b[1], f.b[2], f.b[3], f.c.x, f.c.y, 0, 0},
                                                           v8i{a[0], a[1], a[2], a[3], 0, 0, 0, 0}, acc,
                                                           2 /* A: FP6 e2m3 */, 4 /* B: FP4 e2m1 */, 0, sa, 0,
                                                           kScaleOnehot);
}

// Candidate handling.  A firing lane (its window passed the coarse test for some
// strand of the tile; ~40 % of the rounds have one) appends one record to its wave's
// LDS queue (queue_tile): the fields' top bits of its 16 outputs (8 v_perm + 4
// v_bitop3, 16 bytes), its own list entry (the window) and the tile's first
// global strand | the lane.  The wave decodes its records in batches, one record per
// lane (drain_queue, no global load), into (strand | haplotype in group << 24,
// window) candidates: the first kWaveCands in LDS (s_cand), then the wave's region of
// the global list (A.cands), then the launch-wide overflow list (cand_over_kernel /
// post_scan_kernel).  A tile whose records do not fit drains the queue first and its
// round is scored again (no accumulator live across a drain).  The wave rescores its
// candidates after the scan (rescore_list).
constexpr uint32_t kMQueue = 64;      // records per wave (>= one tile's 64 firing lanes)
constexpr uint32_t kWaveCands = kMWaveCands;  // LDS candidates per wave (C3: 66 mean; the rest in the global list)
__shared__ uint4 s_qdata[kMBlock / 64][kMQueue];
__shared__ uint2 s_qmeta[kMBlock / 64][kMQueue];
__shared__ uint2 s_cand[kMBlock / 64][kWaveCands];
__shared__ uint32_t s_hnext;  // the workgroup's next pair of window tiles (scan_super)
__shared__ uint4 s_hd[kMMaxHapsPerBlock];   // the group's haplotypes: LaneHap
__shared__ uint4 s_hd2[kMMaxHapsPerBlock];  // and (region, pos_off, drun_off, n_druns) for the rescoring
extern __shared__ __attribute__((aligned(16))) int32_t s_mdyn[];  // one-hot table | image | words
// The unit kernel's resident descriptors (scan_pool): s_hd / s_hd2 of every haplotype of
// the unit, haplotype h0 + t of the unit at t.
__shared__ uint4 s_hdu[kMMaxUnit * kMMaxHapsPerBlock];
__shared__ uint4 s_hd2u[kMMaxUnit * kMMaxHapsPerBlock];  // (the rescoring's half: rescore_list<true>)


// What the firing path of a round needs: the group's window list (wl, nw
// entries) for the drain, the first global tile and haplotype of the workgroup.
struct GroupCtx {
    const uint32_t *wl;
    const uint16_t *wl16;  // a narrow group's list (16-bit entries), else null
    uint32_t nw, tile0, h0, slot;
    uint32_t ub;  // the group's place in its unit (unit_place)
    __device__ __forceinline__ uint32_t at(uint32_t q) const { return wl16 ? (uint32_t)wl16[q] : wl[q]; }
};

// Where a wave lists its candidates past the LDS list: ccap entries at clist (a unit's
// groups share the wave's list: the groups' regions of A.cands taken as one).
struct WaveCands {
    uint32_t ccap;
    uint2 *clist;
};
// A group's place in its unit, one word: the group's first haplotype counted from the
// unit's first (a candidate's haplotype = that + its index in the group) | the unit's
// groups << 16.  One group per workgroup: unit_place(0, 1).
__device__ __forceinline__ uint32_t unit_place(uint32_t bias, uint32_t ngu) { return bias | (ngu << 16); }

// What the rescoring reads of a haplotype: DevHap's fields, from the scan
// workgroup's LDS descriptors (s_hd, s_hd2) or from a DevHap.
struct CandHap {
    uint32_t word_off, len, flags, nmask_off, region, pos_off, drun_off, n_druns;
    __device__ __forceinline__ static CandHap of(const DevHap &h) {
        return CandHap{h.word_off, h.len, h.flags, h.nmask_off, h.region, h.pos_off, h.drun_off, h.n_druns};
    }
    __device__ __forceinline__ static CandHap of(const uint4 &a, const uint4 &b) {
        return CandHap{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    }
};

// Appends a record to the spill list (rare: hits past a wave's list, reference
// hits past a region's list, inner ranges past 32).
__device__ __forceinline__ void spill_record(const ScanArgs &A, uint32_t head, uint32_t x, uint32_t y) {
    const uint32_t o = atomicAdd(A.over, 1u);
    if (o < A.spill_cap) {
        A.spill[3 * (size_t)o] = head;
        A.spill[3 * (size_t)o + 1] = x;
        A.spill[3 * (size_t)o + 2] = y;
    }
}

// Shared windows (ScanArgs::share): f(s) for every sharer s of donor `hap`'s window i
// in depth class c (one thread walks the donor's entries: the rare paths; the wave
// lists' expansion is wave-cooperative, rescore_list).
template <class F>
__device__ __forceinline__ void for_sharers(const ScanArgs &A, uint32_t c, uint32_t hap, uint32_t i, F &&f) {
    const uint64_t *so = A.share_off[c];
    if (!so) return;
    const uint64_t e1 = so[hap + 1];
    for (uint64_t e = so[hap]; e < e1; e++) {
        const uint2 s = A.share[c][e];
        if (i >= (s.y & 0xFFFFu) && i < (s.y >> 16)) f(s.x);
    }
}
__device__ __forceinline__ uint32_t strand_class(const ScanArgs &A, uint32_t g) {  // 0: depth 1-2, 1: depth 3-4
    return A.mmeta[(size_t)(g >> 6) * kGMetaInts + kGDepth] > 2 ? 1u : 0u;
}

// What the rescoring loads before it knows that it needs it: the first diff runs of a
// HAP_DEDUP haplotype with round A (3.4 runs per haplotype on average at C3, at most 16,
// profiles/r16 Part 0: four cover most haplotypes whole) and the first inner ranges of
// the region with round B (C3's regions have one, the test regions up to 40).
constexpr uint32_t kRunsUpFront = 4;
constexpr uint32_t kInnerUpFront = 2;

// A rescored candidate: the hit's inner ranges k < 32 (mask bit k; key = key0 + k), to
// be listed by the caller, and for a donor's hit (shared windows) its depth class sc and
// its sn sharer entries share[sc][se ..].
struct CandHit {
    uint32_t mask, key0, sc, sn;
    uint64_t se;
};

// The loads of one round have arrived (one wait per round) and stay where they were
// issued: without a use here the compiler sinks a load into the branch that needs it,
// behind that branch's own chain of loads.
__device__ __forceinline__ void arrived(uint32_t &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void arrived(int32_t &x) { asm volatile("" : "+v"(x)); }

// Exact rescoring of one candidate: window i of haplotype hp (hits index hap)
// for the strand g = global tile * 64 + strand in tile: the exact score (one weight per
// column of the strand's blocks of 8, zero-padded, N columns masked out), strict against
// the strand's minimum (pattern.rs:125-151).  A HAP_DEDUP haplotype's
// window read because it meets a diff run within the class span, but whose strand
// columns [i, i + L) meet none, is the reference's window for that strand: not
// listed (the key assembly adds the reference's hit, tfbs_internal.hpp).  Returns the hit's
// inner ranges k < 32 to be listed by the caller;
// ranges past 32 go to the spill list here.  A hit of the region's reference
// haplotype is also listed for the reuse of its window by the HAP_DEDUP
// haplotypes; a helper reference haplotype (past the region's distinct
// haplotypes) has no counts of its own.
// Every load is issued as soon as its address is known, in two rounds behind the
// descriptor's, each awaited once: round A (addresses from the candidate and hp) the
// strand fields, the tile's depth, the region, the position, the N mask, the packed
// words and the first kRunsUpFront diff runs; round B the weights, the first
// kInnerUpFront inner ranges and, for a possible donor, its share offsets (speculative:
// in range for every haplotype of the launch).  The tests follow in the order of
// pattern.rs; only what lies past the batches (runs 5-16, ranges 3-32) is loaded later,
// by a lane that is still undecided.
__device__ __forceinline__ CandHit score_candidate(const ScanArgs &A, const uint32_t *words, const CandHap &hp,
                                                   uint32_t hap, uint32_t g, uint32_t i) {
    CandHit R{0, 0, 0, 0, 0};
    const int32_t *meta = A.mmeta + (size_t)(g >> 6) * kGMetaInts;
    const uint32_t sn = g & 63u;
    const bool dedup = (hp.flags & HAP_DEDUP) && A.dedup;
    const bool donor = (hp.flags & HAP_DEDUP) && (A.share_off[0] || A.share_off[1]);  // its sharers hit too
    // round A
    int4 sf = *reinterpret_cast<const int4 *>(meta + kGStrandInts * sn);  // min, woff, len, slot
    int32_t depth = meta[kGDepth];
    const DevRegion *rgp = A.regions + hp.region;
    uint32_t inner_off = rgp->inner_off, n_inner = rgp->n_inner, hap_begin = rgp->hap_begin, hap_count = rgp->hap_count;
    const uint32_t ic = min(i, max(hp.len, 1u) - 1);  // i + L > len: no hit (below), reads stay in range
    int32_t p = (int32_t)i;
    if (hp.flags & HAP_HAS_POS) p = A.posrel[hp.pos_off + ic];
    uint32_t m0 = 0, m1 = 0;
    if (hp.flags & HAP_HAS_N) {
        const uint32_t *m = A.nmask + hp.nmask_off + (ic >> 5);
        m0 = m[0];
        m1 = m[1];
    }
    const uint32_t *w = words + hp.word_off + (ic >> 4);
    uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    uint32_t ra[kRunsUpFront], rb[kRunsUpFront];  // (no run: [~0, 0] meets no window)
    const uint32_t n_runs = dedup ? hp.n_druns : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kRunsUpFront; j++) {
        ra[j] = 0xFFFFFFFFu;
        rb[j] = 0;
        if (j < n_runs) {
            ra[j] = A.druns[2 * (size_t)(hp.drun_off + j)];
            rb[j] = A.druns[2 * (size_t)(hp.drun_off + j) + 1];
        }
    }
    arrived(sf.x), arrived(sf.y), arrived(sf.z), arrived(sf.w), arrived(depth);
    arrived(inner_off), arrived(n_inner), arrived(hap_begin), arrived(hap_count);
    arrived(p), arrived(m0), arrived(m1), arrived(w0), arrived(w1), arrived(w2);
#pragma unroll
    for (uint32_t j = 0; j < kRunsUpFront; j++) arrived(ra[j]), arrived(rb[j]);
    // round B
    const uint32_t L = (uint32_t)sf.z;
    const uint32_t sh = 2 * (ic & 15);
    const uint32_t img[2] = {__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh)};
    const int32_t *wt = A.mweights + sf.y;
    int32_t v[32];
#pragma unroll
    for (uint32_t jb = 0; jb < 32; jb += 8) {
        if (jb < L) {  // a lane loads only its strand's blocks
#pragma unroll
            for (uint32_t j = jb; j < jb + 8; j++) v[j] = wt[4 * j + ((img[j >> 4] >> (2 * (j & 15))) & 3u)];
        } else {
#pragma unroll
            for (uint32_t j = jb; j < jb + 8; j++) v[j] = 0;
        }
    }
    const int32_t *inner = A.inner + 2 * (size_t)inner_off;
    const uint32_t nk = min(n_inner, 32u);
    int32_t rs[kInnerUpFront], re[kInnerUpFront];
#pragma unroll
    for (uint32_t k = 0; k < kInnerUpFront; k++) {
        rs[k] = re[k] = 0;
        if (k < nk) {
            rs[k] = inner[2 * k];
            re[k] = inner[2 * k + 1];
        }
    }
    R.sc = depth > 2 ? 1u : 0u;  // (strand_class)
    const uint64_t *so = A.share_off[R.sc];
    uint32_t e0l = 0, e0h = 0, e1l = 0, e1h = 0;
    if (donor && so) {
        const uint64_t e0 = so[hap], e1 = so[hap + 1];
        e0l = (uint32_t)e0, e0h = (uint32_t)(e0 >> 32), e1l = (uint32_t)e1, e1h = (uint32_t)(e1 >> 32);
    }
#pragma unroll
    for (uint32_t j = 0; j < 32; j++) arrived(v[j]);
#pragma unroll
    for (uint32_t k = 0; k < kInnerUpFront; k++) arrived(rs[k]), arrived(re[k]);
    arrived(e0l), arrived(e0h), arrived(e1l), arrived(e1h);
    // the tests
    if (i + L > hp.len) return R;                       // past the end (pattern.rs:147-150)
    const uint32_t live = ~__builtin_amdgcn_alignbit(m1, m0, ic & 31);  // bit j: base i + j is not N
    const uint32_t keep = live & (L >= 32 ? ~0u : (1u << L) - 1);      // columns < L that are not N
    int32_t sc = 0;
#pragma unroll
    for (uint32_t j = 0; j < 32; j++) sc += v[j] & -(int32_t)((keep >> j) & 1u);  // N scores 0
    if (!(sc > sf.x)) return R;                         // strict (pattern.rs:151)
    if (dedup) {  // columns [i, i + L) the reference's: its hit (key assembly)
        bool dirty = false;
#pragma unroll
        for (uint32_t j = 0; j < kRunsUpFront; j++) dirty = dirty || run_meets(ra[j], rb[j], i, L);
        for (uint32_t k = hp.drun_off + kRunsUpFront; k < hp.drun_off + hp.n_druns && !dirty; k++)
            dirty = run_meets(A.druns[2 * (size_t)k], A.druns[2 * (size_t)k + 1], i, L);
        if (!dirty) return R;
    }
    if (A.hits && i / 64 < A.hits_wpp) {
        auto mark = [&](uint32_t x) {
            atomicOr(A.hits + ((size_t)x * A.n_patterns_total + (uint32_t)meta[kGOrig + sn]) * A.hits_wpp + i / 64,
                     1ull << (i & 63));
        };
        mark(hap);
        if (donor) for_sharers(A, R.sc, hap, i, mark);
    }
    if ((hp.flags & HAP_REF) && A.dedup) {  // for the HAP_DEDUP haplotypes' unscanned windows
        const uint32_t at = atomicAdd(A.ref_count + hp.region, 1u);
        if (at < kRefPerRegion) {
            A.ref_hits[2 * ((size_t)hp.region * kRefPerRegion + at)] = g;
            A.ref_hits[2 * ((size_t)hp.region * kRefPerRegion + at) + 1] = i;
        } else {
            spill_record(A, hp.region | 0x80000000u, g, i);
        }
    }
    if (hap >= hap_begin + hap_count) return R;  // a helper reference haplotype: no keys
    const uint32_t off0 = (uint32_t)sf.w * n_inner;
    // range.rs:18-21 as main.rs:503 uses it
    auto overlaps = [&](int32_t s, int32_t en) {
        const uint32_t span = (uint32_t)(en - s);
        return (uint32_t)(p - s) <= span || (uint32_t)(p + (int32_t)L - 1 - s) <= span;
    };
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t k = 0; k < kInnerUpFront; k++)
        if (k < nk && overlaps(rs[k], re[k])) mask |= 1u << k;
    for (uint32_t k = kInnerUpFront; k < nk; k++) {
        const int2 r = *reinterpret_cast<const int2 *>(inner + 2 * k);
        if (overlaps(r.x, r.y)) mask |= 1u << k;
    }
    for (uint32_t k = 32; k < n_inner; k++) {           // ranges past 32 (rare)
        if (overlaps(inner[2 * k], inner[2 * k + 1])) {
            spill_record(A, hp.region, A.hap_base + hap, off0 + k);
            if (donor)
                for_sharers(A, R.sc, hap, i,
                            [&](uint32_t x) { spill_record(A, hp.region, A.hap_base + x, off0 + k); });
        }
    }
    R.key0 = off0;
    R.mask = mask;
    if (mask) {  // the donor's entries, for the caller's expansion
        R.se = (uint64_t)e0l | ((uint64_t)e0h << 32);
        R.sn = (uint32_t)(((uint64_t)e1l | ((uint64_t)e1h << 32)) - R.se);
    }
    return R;
}

// The candidate lists' room per wave (A.cand_cap per workgroup; the hit lists':
// A.hit_cap, rescore_list): the LDS list's (at most kWaveCands) followed by the wave's
// region of the global list (TFBS_CAND_CAP makes all of them small in the spill tests).
__device__ __forceinline__ uint32_t wave_cand_cap(const ScanArgs &A) { return A.cand_cap / (kMBlock / 64); }
// slot: the workgroup's place in the per-group lists (region_base + its first
// haplotype group in the launch = that group's index in the batch).  The wave's
// global list in a unit of ngu groups whose first slot is `slot`: the groups' regions
// are consecutive, each wave takes ngu x its share of one (ngu = 1: one workgroup's
// region in eight parts).
__device__ __forceinline__ WaveCands unit_cands(const ScanArgs &A, uint32_t slot, uint32_t ngu, uint32_t wave) {
    const uint32_t ccap = ngu * wave_cand_cap(A);
    return WaveCands{ccap, reinterpret_cast<uint2 *>(A.cands) + (size_t)slot * A.cand_cap + (size_t)wave * ccap};
}

#ifdef TFBS_SCAN_PROF
// per wave of the workgroup's (unit's) first slot: [0] s_memtime at the kernel's start,
// [1] after the staging barrier, [2] after the scan loops, [3] cycles waited at the super
// tiles' barriers (TFBS_ROUND_PROF, else 0), [4] after the rescoring, [5] / [6]
// s_memrealtime (100 MHz, one clock for the chip) at the start and the end, [7] pairs
// scored | candidates << 32; [8, 16) TFBS_ROUND_PROF's split, or without it the
// rescoring's (rescore_list): [8] cycles from a pass's start to its candidates scored
// and its donors' entry ranges known, summed over the passes, [9] cycles in the
// expansion's rounds, [10] donor hits, [11] the entries they span (T), [13] passes, [14]
// cycles in the hits' own appends (with the entries' prefix and the first round's fetch
// issued in front of them); [12] stays 0: tools/scan_prof.py tells the builds apart by it
#define SCAN_STAMP(k, v) \
    do { if (A.prof && lane == 0) A.prof[((size_t)slot * kMBlockWaves + wave) * kScanProfWords + (k)] = (v); } while (0)
#else
#define SCAN_STAMP(k, v) do { } while (0)
#endif
#if defined(TFBS_SCAN_PROF) && !defined(TFBS_ROUND_PROF)
#define RESCORE_T() ({ __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                       __builtin_amdgcn_sched_barrier(0); t_; })
#define RESCORE_PROF(...) __VA_ARGS__
#else
#define RESCORE_PROF(...)
#endif

// The wave's listed candidates, one per lane (after its scan: no accumulator
// is live, and the other waves keep the matrix cores busy); each hit's
// (haplotype, key) pairs are appended to the wave's part of its group's hit
// list (ballot prefix: no atomics), the excess spilled.
// UNIT: the candidates of a unit of ngu groups (first haplotype h0, first slot `slot`),
// rescored once -- the descriptors from the unit's resident copies (s_hdu, s_hd2u), the
// words from global memory (words = A.words) --; a hit goes to the wave list of its
// haplotype's group (slot + the group in the unit), the ballot prefix taken over that
// group's lanes, one count per group (hnv: lane u holds group u's).  candn likewise: a
// group's are its candidates in the lists; those past the lists (cn - n) are counted at
// the unit's first slot.
// A pass (64 candidates) is: the scores (score_candidate: the descriptor from LDS, then
// two rounds of loads); the hits' own pairs, per group; the expansion of the donors'
// hits to their sharers (shared windows) over the pass's flattened entry space -- the
// donor lanes' entry counts sn in a wave prefix, total T, and in each round of 64 lane j
// owns entry t0 + j: it finds the donor lane whose range holds it, takes that lane's
// hit by shuffle, loads the one share entry and tests the hit's window against it; the
// covering entries append the hit's pairs for their sharers to the list of the DONOR's
// group, by the same ballot prefix, one key bit per ballot.  One load round per 64
// entries of however many donors, ceil(T / 64) rounds a pass, and a round's load is issued a
// round ahead: the first before the hits' own pairs are listed, the next before this
// round's pairs are appended.  The donor of an entry:
// the donors whose ranges start inside the round write their lane at the start's place
// in a 64-word table (the wave's queue LDS, empty once the scan is over: s_qdata is only
// touched by its own wave's queue_tile / drain_queue, and by the fused post-scan behind a
// barrier); a lane's donor is the last start at or before it, or the donor that the
// round before ended in.
template <bool UNIT>
__device__ __forceinline__ void rescore_list(const ScanArgs &A, const uint32_t *words, uint32_t h0, uint32_t slot,
                                             uint32_t ngu, uint32_t wave, uint32_t lane, uint32_t cn) {
    const uint32_t cap = A.hit_cap / (kMBlock / 64);  // the hit list's room per wave
    const WaveCands W = unit_cands(A, slot, ngu, wave);
    const uint32_t lcap = min(W.ccap, kWaveCands), n = min(cn, lcap + W.ccap);
    const uint2 *glist = W.clist;
    // the round's range starts (64 words); volatile: lanes read what OTHER lanes of the wave wrote, which the
    // compiler would otherwise replace by the lane's own store (the wave's LDS accesses are executed in order)
    volatile uint32_t *s_start = reinterpret_cast<volatile uint32_t *>(&s_qdata[wave][0]);
    uint32_t hnv = 0, cnv = lane == 0 ? cn - n : 0u;
    RESCORE_PROF(unsigned long long p_score = 0, p_exp = 0, p_own = 0, p_don = 0, p_T = 0, p_pass = 0;)
    auto list_of = [&](uint32_t u) {
        return reinterpret_cast<uint2 *>(A.hitl) + (size_t)(slot + u) * A.hit_cap + (size_t)wave * cap;
    };
    // the pairs (x, key0 + bit) of every set bit of m, behind the list's hn entries (uniform)
    auto append = [&](uint2 *out, uint32_t &hn, uint32_t m, uint32_t x, uint32_t key0, uint32_t region) {
        uint64_t act;
        while ((act = __ballot(m != 0)) != 0) {
            if (m) {
                const uint32_t at = hn + __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0));
                const uint32_t key = key0 + __builtin_ctz(m);
                m &= m - 1;
                if (at < cap) out[at] = make_uint2(A.hap_base + x, key);
                else spill_record(A, region, A.hap_base + x, key);
            }
            hn += (uint32_t)__popcll(act);
        }
    };
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
        RESCORE_PROF(const unsigned long long tp0 = RESCORE_T();)
        const uint32_t k = k0 + lane;
        CandHit R{0, 0, 0, 0, 0};
        uint32_t hap = h0, win = 0, gi = 0, region = 0;
        if (k < n) {
            const uint2 c = k < lcap ? s_cand[wave][k] : glist[k - lcap];
            const uint32_t hl = c.x >> 24;  // the haplotype in the group (unit)
            hap = h0 + hl;
            win = c.y;
            const CandHap hp = UNIT ? CandHap::of(s_hdu[hl], s_hd2u[hl]) : CandHap::of(s_hd[hl], s_hd2[hl]);
            if (UNIT)  // its group in the unit (no division: its reciprocal would live across the scan)
                for (uint32_t u = 1; u < kMMaxUnit; u++) gi += hl >= u * A.haps_per_block ? 1u : 0u;
            region = hp.region;
            R = score_candidate(A, words, hp, hap, c.x & 0xFFFFFFu, win);
        }
        const uint32_t sn = R.sn;
#if defined(TFBS_SCAN_PROF) && !defined(TFBS_ROUND_PROF)
        {   // (the scores and the donors' ranges awaited: the ballots' operands)
            const uint64_t don = __ballot(sn != 0), hit = __ballot(R.mask != 0);
            asm volatile("" ::"s"(don), "s"(hit));
            p_score += RESCORE_T() - tp0;
            p_don += (uint32_t)__popcll(don);
            p_pass++;
        }
        const unsigned long long tu0 = RESCORE_T();
#endif
        // the expansion: the donor lanes' entries [se, se + sn) laid end to end, entry t of
        // the pass = entry t - excl of the lane whose [excl, excl + sn) holds t
        uint32_t incl = sn;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= o) incl += t;
        }
        const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63), excl = incl - sn;
        const uint64_t ebase = R.se - excl;  // + t: the lane's entry t (mod 2^64)
        const uint32_t meta = R.sc | (gi << 1);
        uint32_t carry = 0;  // the donor lane that the round before ended in
        // round t0's entry of this lane (its load issued) and the hit it belongs to
        struct Entry {
            uint2 s;
            uint32_t meta, win, key0, mask, region;
        };
        auto fetch = [&](uint32_t t0) {
            const uint32_t t = t0 + lane;
            s_start[lane] = 0xFFFFFFFFu;
            if (sn != 0 && excl - t0 < 64u) s_start[excl - t0] = lane;
            const uint32_t sv = s_start[lane];
            const uint64_t starts = __ballot(sv != 0xFFFFFFFFu);
            const uint64_t below = starts & ((2ull << lane) - 1);  // the starts at or before this lane
            const uint32_t from = (uint32_t)__shfl((int)sv, below ? 63 - __builtin_clzll(below) : 0);
            const uint32_t src = below ? from : carry;
            carry = (uint32_t)__builtin_amdgcn_readlane((int)src, 63);
            const uint64_t d_e = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)ebase, (int)src) |
                                  ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(ebase >> 32), (int)src) << 32)) + t;
            Entry E;
            E.meta = (uint32_t)__shfl((int)meta, (int)src);
            E.win = (uint32_t)__shfl((int)win, (int)src);
            E.key0 = (uint32_t)__shfl((int)R.key0, (int)src);
            E.mask = (uint32_t)__shfl((int)R.mask, (int)src);
            E.region = (uint32_t)__shfl((int)region, (int)src);
            E.s = make_uint2(0, 0);
            if (t < T) E.s = A.share[E.meta & 1u][d_e];
            return E;
        };
        Entry cur{make_uint2(0, 0), 0, 0, 0, 0, 0};
        if (T) cur = fetch(0);  // (in flight while the hits' own pairs are listed)
        for (uint32_t u = 0; u < ngu; u++) {  // the lanes of group u (wave-uniform loop)
            const bool in = !UNIT || gi == u;
            uint32_t hn = (uint32_t)__builtin_amdgcn_readlane((int)hnv, (int)u);  // wave-uniform
            const uint32_t listed = (uint32_t)__popcll(__ballot(k < n && in));  // (by the whole wave)
            if (lane == u) cnv += listed;
            append(list_of(u), hn, in ? R.mask : 0u, hap, R.key0, region);
            if (lane == u) hnv = hn;
        }
        RESCORE_PROF(const unsigned long long tu1 = RESCORE_T(); p_own += tu1 - tu0;)
        for (uint32_t t0 = 0; t0 < T; t0 += 64) {
            Entry nx = cur;
            if (t0 + 64 < T) nx = fetch(t0 + 64);  // the next round's entries, in flight behind this round's
            const bool mine = cur.win >= (cur.s.y & 0xFFFFu) && cur.win < (cur.s.y >> 16);  // (no entry: [0, 0))
            for (uint32_t u = 0; u < ngu; u++) {  // the entries of group u's donors
                uint32_t hn = (uint32_t)__builtin_amdgcn_readlane((int)hnv, (int)u);
                append(list_of(u), hn, mine && (!UNIT || (cur.meta >> 1) == u) ? cur.mask : 0u, cur.s.x, cur.key0,
                       cur.region);
                if (lane == u) hnv = hn;
            }
            cur = nx;
        }
        RESCORE_PROF(p_exp += RESCORE_T() - tu1; p_T += T;)
    }
    RESCORE_PROF(SCAN_STAMP(8, p_score); SCAN_STAMP(9, p_exp); SCAN_STAMP(10, p_don); SCAN_STAMP(11, p_T);
                 SCAN_STAMP(13, p_pass); SCAN_STAMP(14, p_own);)
    if (lane < ngu) {  // every slot of the unit, also a group's without a window
        A.hitn[(size_t)(slot + lane) * kMBlockWaves + wave] = min(hnv, cap);
        // (the list counters: per-wave stores summed on the host -- one atomic per wave on a
        // shared counter serialises at L2, ~10 ns each, and doubled the C3 step)
        A.candn[(size_t)(slot + lane) * kMBlockWaves + wave] = cnv;
    }
}

// Coarse test of one tile: OR of the lane's 16 outputs, the fields' top bits
// (7 v_or3 + v_bitop3); x != 0 iff the lane has a candidate.  Both tiles of a
// pair are tested in the MFMAs' basic block (tools/isa_lint.py checks the wait
// states).
__device__ __forceinline__ uint32_t coarse_test(const v16f &acc) {
    uint32_t u[16];
#pragma unroll
    for (int r = 0; r < 16; r++) u[r] = __float_as_uint(acc[r]);
    const uint32_t x = (u[0] | u[1] | u[2]) | (u[3] | u[4] | u[5]) | (u[6] | u[7] | u[8]) | (u[9] | u[10] | u[11]) |
                       (u[12] | u[13] | u[14]) | u[15];
    return x & kTestMask;
}

// The same tile's candidates decoded at once when the queue is full (rare): the
// lane's mask as drain_queue builds it, each candidate listed as drain_queue lists it.
__device__ __forceinline__ uint32_t record_mask(const uint32_t (&dd)[4]) {
    // dword k (queue_tile): the first strand's top bits of outputs 4k, 4k+1, 4k+2,
    // 4k+3 at 2, 10, 3, 11, the second's at 21, 29, 22, 30.  m bit b: strand b >> 4,
    // output 4 (b >> 1 & 3) + 2 (b & 1) + (b >> 3 & 1)
    uint32_t lo = (dd[0] >> 2) & 0x303u, hi = (dd[0] >> 21) & 0x303u;
#pragma unroll
    for (int k = 1; k < 4; k++) {
        lo |= (dd[k] << (2 * k - 2)) & (0x303u << (2 * k));
        hi |= (dd[k] >> (21 - 2 * k)) & (0x303u << (2 * k));
    }
    return lo | (hi << 16);
}
// bytes 1, 1', 2, 2' of outputs 2j, 2j + 1: top bits at 2, 10, 21, 29; dword k keeps
// those of j = 2k and, one bit up, of j = 2k + 1
__device__ __forceinline__ void record_bits(const v16f &acc, uint32_t (&x)[4]) {
    uint32_t d[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
        d[j] = __builtin_amdgcn_perm(__float_as_uint(acc[2 * j + 1]), __float_as_uint(acc[2 * j]), 0x06020501u);
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] = __builtin_amdgcn_bitop3_b32(d[2 * k], d[2 * k + 1] << 1, kQueueBits, 0xe4);  // M ? d[2k] : d[2k+1] << 1
}
// Lists the candidates of mask m (bit b: strand b >> 4 of output r(b)) of a record
// whose tile's first global strand | lane is gl and whose window entry is ent; one
// per lane per pass.
__device__ __forceinline__ void list_mask(const ScanArgs &A, const GroupCtx &G, uint32_t wave, uint32_t m, uint32_t gl,
                                          uint32_t ent, uint32_t &cn) {
    const WaveCands W = unit_cands(A, G.slot, G.ub >> 16, wave);  // (G.slot: the unit's first)
    const uint32_t lcap = min(W.ccap, kWaveCands), cap = lcap + W.ccap;
    uint2 *glist = W.clist;
    const uint32_t hl = ent & (kMMaxHapsPerBlock - 1), i = ent >> 6;
    const uint32_t gbase = (gl & ~63u) + 8 * ((gl >> 5) & 1u);  // the tile's first strand; lanes 32-63: pairs + 4
    uint64_t act;
    while ((act = __ballot(m != 0)) != 0) {
        if (m) {
            const uint32_t b = __builtin_ctz(m);
            m &= m - 1;
            const uint32_t r = 4 * ((b >> 1) & 3u) + 2 * (b & 1u) + ((b >> 3) & 1u);
            const uint32_t g = gbase + 2 * ((r & 3u) + 8 * (r >> 2)) + (b >> 4);
            const uint32_t slot = cn + __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0));
            const uint2 c = make_uint2(g | (((G.ub & 0xFFFFu) + hl) << 24), i);
            if (slot < lcap) {
                s_cand[wave][slot] = c;
            } else if (slot < cap) {
                glist[slot - lcap] = c;
            } else {  // rescored after the scan (cand_over_kernel / post_scan_kernel)
                const uint32_t o = atomicAdd(A.over + 1, 1u);
                if (o < A.cand_over_cap) {
                    A.cand_over[3 * (size_t)o] = A.hap_base + G.h0 + hl;  // batch index
                    A.cand_over[3 * (size_t)o + 1] = g;
                    A.cand_over[3 * (size_t)o + 2] = i;
                }
            }
        }
        cn += (uint32_t)__popcll(act);
    }
}

// Decodes the wave's first n queue records, one per lane per pass: the record's
// candidate bits (both strands of its 16 outputs) gathered into one mask, each
// candidate listed (one per lane per round; cn: the wave's count, uniform).
__device__ __forceinline__ void drain_queue(const ScanArgs &A, const GroupCtx &G, uint32_t n, uint32_t wave,
                                            uint32_t lane, uint32_t &cn) {
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
        const uint32_t e = e0 + lane;
        uint32_t m = 0, ent = 0, gl = 0;
        if (e < n) {
            const uint4 d = s_qdata[wave][e];
            const uint2 q = s_qmeta[wave][e];
            ent = q.x;
            gl = q.y;
            const uint32_t dd[4] = {d.x, d.y, d.z, d.w};
            m = record_mask(dd);
        }
        list_mask(A, G, wave, m, gl, ent, cn);
    }
}

// A firing tile (x: the lane's coarse test; q: the lane's list position, rows past
// the list's nw entries being the last tile's padding; the queue has room for the
// tile's records): each firing lane queues one record -- bytes 1-2 of its outputs
// (the fields' top bits), its list entry (window row lane & 31 of window tile
// `which`, went) and g0 | lane (g0: the strand tile's first global strand) --;
// qn (uniform) counts the wave's records.
__device__ __forceinline__ void queue_tile(const ScanArgs &A, const GroupCtx &G, const v16f &acc, bool mine, uint64_t f,
                                           uint32_t g0, uint32_t went, uint32_t which, uint32_t lane, uint32_t wave,
                                           uint32_t &qn, uint32_t &cn) {
    const uint32_t nf = (uint32_t)__popcll(f);
    uint32_t ent = 0, x[4] = {0, 0, 0, 0};
    if (mine) {
        ent = went;  // the lane's own entry of tile `which` (lanes l and l + 32 load the same)
        record_bits(acc, x);
    }
    if (__builtin_expect(qn + nf > kMQueue, 0)) {  // the queue is full (dense hits): decoded first
        drain_queue(A, G, qn, wave, lane, cn);
        qn = 0;
    }
    if (mine) {
        const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(f >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)f, qn));
        s_qdata[wave][at] = uint4{x[0], x[1], x[2], x[3]};
        s_qmeta[wave][at] = make_uint2(ent, g0 | lane);
    }
    qn += nf;
}

// One round's chains with chunk 0's B fragment already loaded (f0: read during the
// round before, so the round's first MFMAs do not wait for LDS); chunks 1.. are read
// before the first MFMA is issued.  a1 / c1: the pair's second window tile (TWO).
template <int D, int NK, bool TWO>
__device__ __forceinline__ void round_scores(const char *tile, uint32_t lane, const BFrag &f0, const v4i (&a0)[NK],
                                             const v4i (&a1)[NK], const v16f &cb, int sa, v16f &c0, v16f &c1) {
    if (D >= 3) {
        // depth 3-4 (the class whose A fragments take 32 VGPRs): chunk kc + 1's
        // fragment read as chunk kc's MFMAs issue, a scheduling barrier between the
        // chunks -- two fragments live instead of D (no scratch spill)
        BFrag cur = f0;
        c0 = cb;
        if (TWO) c1 = cb;
#pragma unroll
        for (int kc = 0; kc < D; kc++) {
            BFrag nx;
            if (kc + 1 < D) {
                nx.b = *reinterpret_cast<const v4i *>(tile + (kc + 1) * 1536 + lane * 16);
                nx.c = *reinterpret_cast<const int2 *>(tile + (kc + 1) * 1536 + 1024 + lane * 8);
            }
            c0 = mfma_chunk(a0[kc], cur, c0, sa);
            if (TWO) c1 = mfma_chunk(a1[kc], cur, c1, sa);
            __builtin_amdgcn_sched_barrier(0);
            if (kc + 1 < D) cur = nx;
        }
        return;
    }
    BFrag f[D];
    f[0] = f0;
#pragma unroll
    for (int kc = 1; kc < D; kc++) {
        f[kc].b = *reinterpret_cast<const v4i *>(tile + kc * 1536 + lane * 16);
        f[kc].c = *reinterpret_cast<const int2 *>(tile + kc * 1536 + 1024 + lane * 8);
    }
    c0 = cb;
    if (TWO) c1 = cb;
#pragma unroll
    for (int kc = 0; kc < D; kc++) {
        c0 = mfma_chunk(a0[kc], f[kc], c0, sa);
        if (TWO) c1 = mfma_chunk(a1[kc], f[kc], c1, sa);
    }
}
__device__ __forceinline__ void load_frag0(const char *tile, uint32_t lane, BFrag &f) {
    f.b = *reinterpret_cast<const v4i *>(tile + lane * 16);
    f.c = *reinterpret_cast<const int2 *>(tile + 1024 + lane * 8);
}

#ifdef TFBS_ROUND_PROF
// Per-round clock split (profiling builds only, TFBS_SCAN_PROF words 8-15): per wave,
// shader cycles from a two-tile round's top to its first MFMA's issue (the chunk-0 B
// fragment and the matrix pipe), first to last MFMA issued, last MFMA to the test's
// decision, the firing path; rounds, fired rounds; the super tiles' restaging; the
// pairs' own work (next pair, list entries, A fragments); [8] (stamp word 3) the wave's
// wait at the super tiles' two barriers (every super tile).  s_memtime between
// scheduling barriers: the stamps order the round but add their own latency.
__shared__ unsigned long long s_rprof[kMBlock / 64][9];
#define RPROF_T() ({ __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                     __builtin_amdgcn_sched_barrier(0); t_; })
#define RPROF_ADD(wave, k, v) do { if ((threadIdx.x & 63) == 0) s_rprof[wave][k] += (v); } while (0)
#endif

// The strand tiles of depth D, [tb, te) (images from `img`), x window tiles ta (A
// fragments a0) and, if TWO, ta + 1 (a1) of the group's list: per strand tile one
// round (D chunks x the window tiles), the coarse test of both tiles with one vector
// compare, the firing path (queue_tile) only when some lane fired.  A pointer loop (3
// scalar instructions per round); the next round's chunk-0 B fragment is read
// unconditionally (past the last tile: the image area is padded by kMChunkBytes, the
// value unused).
template <int D, int NK, bool TWO>
__device__ __forceinline__ void scan_segment(const ScanArgs &A, const char *img, uint32_t tb, uint32_t te,
                                             const GroupCtx &G, uint32_t lane, uint32_t wave, const v4i (&a0)[NK],
                                             const v4i (&a1)[NK], uint32_t ta, uint32_t e0, uint32_t e1, const v16f &cb,
                                             int sa, uint32_t &qn, uint32_t &cn) {
    constexpr uint32_t kTB = mfma_tile_bytes(D);
    const char *tile = img;
    const char *const end = img + (te - tb) * kTB;
    uint32_t g0 = (G.tile0 + tb) * kMStrands;  // the tile's first global strand
    const uint32_t q0 = kMWindows * ta + (lane & 31);  // the lane's list positions (tile a; tile b: + 32)
    BFrag pf;
    load_frag0(img, lane, pf);
#ifdef TFBS_ROUND_PROF
    unsigned long long pb = 0, pm = 0, pt = 0, pfi = 0, nr = 0, nf = 0;
#endif
    do {
#ifdef TFBS_ROUND_PROF
        const unsigned long long t0 = RPROF_T();
        BFrag f[D];
        f[0] = pf;
#pragma unroll
        for (int kc = 1; kc < D; kc++) {
            f[kc].b = *reinterpret_cast<const v4i *>(tile + kc * 1536 + lane * 16);
            f[kc].c = *reinterpret_cast<const int2 *>(tile + kc * 1536 + 1024 + lane * 8);
        }
        v16f c0 = mfma_chunk(a0[0], f[0], cb, sa), c1;
        const unsigned long long t1 = RPROF_T();
        if (TWO) c1 = mfma_chunk(a1[0], f[0], cb, sa);
#pragma unroll
        for (int kc = 1; kc < D; kc++) {
            c0 = mfma_chunk(a0[kc], f[kc], c0, sa);
            if (TWO) c1 = mfma_chunk(a1[kc], f[kc], c1, sa);
        }
        const unsigned long long t2 = RPROF_T();
#else
        v16f c0, c1;
        round_scores<D, NK, TWO>(tile, lane, pf, a0, a1, cb, sa, c0, c1);
#endif
        load_frag0(tile + kTB, lane, pf);
        const uint32_t x0 = coarse_test(c0), x1 = TWO ? coarse_test(c1) : 0u;
        const bool fired = __ballot((x0 | x1) != 0) != 0;
#ifdef TFBS_ROUND_PROF
        const unsigned long long t3 = RPROF_T();
#endif
        if (__builtin_expect(fired, 0)) {
#ifdef TFBS_ROUND_PROF
            nf++;
#endif
            // cold: queue the firing lanes' records (padding rows left out), or list
            // a tile's candidates at once when the queue is full
            const bool m0 = x0 != 0 && q0 < G.nw, m1 = TWO && x1 != 0 && q0 + kMWindows < G.nw;
            const uint64_t f0 = __ballot(m0), f1 = __ballot(m1);
            if (f0) queue_tile(A, G, c0, m0, f0, g0, e0, 0, lane, wave, qn, cn);
            if (TWO && f1) queue_tile(A, G, c1, m1, f1, g0, e1, 1, lane, wave, qn, cn);
        }
#ifdef TFBS_ROUND_PROF
        const unsigned long long t4 = RPROF_T();
        pb += t1 - t0;
        pm += t2 - t1;
        pt += t3 - t2;
        pfi += t4 - t3;
        nr++;
#endif
        tile += kTB;
        g0 += kMStrands;
    } while (tile != end);
#ifdef TFBS_ROUND_PROF
    if (TWO) {
        RPROF_ADD(wave, 0, pb);
        RPROF_ADD(wave, 1, pm);
        RPROF_ADD(wave, 2, pt);
        RPROF_ADD(wave, 3, pfi);
        RPROF_ADD(wave, 4, nr);
        RPROF_ADD(wave, 5, nf);
    }
#endif
}

// One step: every strand tile of the super tile (depth segments 1..NK, byte
// d - 1 of seg = the end of depth d) x the window tiles ta and, if TWO, ta + 1.
template <int NK, bool TWO>
__device__ __forceinline__ void scan_step(const ScanArgs &A, const char *s_img, uint32_t seg, const GroupCtx &G,
                                          uint32_t lane, uint32_t wave, const v4i (&a0)[NK], const v4i (&a1)[NK],
                                          uint32_t ta, uint32_t e0, uint32_t e1, const v16f &cb, int sa, uint32_t &qn,
                                          uint32_t &cn) {
    uint32_t tb = NK > 2 ? (seg >> 8) & 255u : 0;  // class 4 starts at depth 3 (no tile of depth 1-2)
    const char *img = s_img;
#define TFBS_SEGMENT(D)                                                                                          \
    if (D <= NK && D + 1 >= NK) { /* a class holds depths NK - 1 and NK (mfma_depth_class) */                  \
        const uint32_t te = (seg >> (8 * (D - 1))) & 255u;                                                     \
        if (te > tb)                                                                                             \
            scan_segment<(D <= NK ? D : 1), NK, TWO>(A, img, tb, te, G, lane, wave, a0, a1, ta, e0, e1, cb, sa, qn, cn); \
        img += (te - tb) * mfma_tile_bytes(D);                                                                   \
        tb = te;                                                                                                 \
    }
    TFBS_SEGMENT(1)
    TFBS_SEGMENT(2)
    TFBS_SEGMENT(3)
    TFBS_SEGMENT(4)
#undef TFBS_SEGMENT
}

// The A fragments of list entry we (window << 6 | haplotype in the group): the
// lane's haplotype from the LDS descriptors, its window's words, the one-hot.
template <int NK>
__device__ __forceinline__ void entry_onehot(const ScanArgs &A, const uint32_t *words, uint32_t we, const char *tab,
                                             v4i (&a)[NK]) {
    const uint4 d = s_hd[we & (kMMaxHapsPerBlock - 1)];
    const LaneHap hm{d.x, d.y, d.z, d.w};
    const uint32_t i = we >> 6;
    WinWords ww;
    load_window(A, words, hm, i, ww);
    build_onehot<NK>(hm, i, ww, tab, a);
}

// The unit kernel's pair pool (scan_pool).  A unit's descriptors stay in the LDS for the
// whole workgroup (s_hdu: haplotype h0 + t of the unit at t, so a group's entry is found
// at its bias + the entry's six haplotype bits), and s_pool holds, per depth class, one
// word of four per group of the unit: x = the pairs of
// window tiles of the groups up to and including it (a group without a window in the
// class, or past the unit's last, adds none: x of the last entry is the pool's size),
// y = the entries of its list | narrow << 31, (z, w) = the list's first entry in
// wlist / wlist16.
__shared__ uint4 s_pool[2][kMMaxUnit];
static_assert(kMMaxUnit * kMMaxHapsPerBlock <= kMBlock, "one thread per descriptor of a unit");
constexpr uint32_t kPoolNarrow = 1u << 31;

__device__ __forceinline__ uint32_t pool_pairs(uint32_t nw) { return ((nw + kMWindows - 1) / kMWindows + 1) / 2; }

// Written once by the workgroup's first wave, before the first super tile's barriers
// (hg0 / h0: the unit's first group / haplotype; lane 4 c + g: class c, group g; a class
// without a super tile has no list and an empty pool).
__device__ __forceinline__ void pool_fill(const ScanArgs &A, uint32_t hg0, uint32_t h0, uint32_t ngu, uint32_t lane) {
    uint32_t has = 0;
    for (uint32_t si = 0; si < A.n_msupers; si++) has |= A.msupers[si].nk > 2 ? 2u : 1u;
    const uint32_t gi = lane & (kMMaxUnit - 1), c = (lane / kMMaxUnit) & 1u;
    const uint64_t *off = c ? A.wlist_off[1] : A.wlist_off[0];
    uint32_t nw = 0, narrow = 0;
    uint64_t e0 = 0;
    if (lane < 2 * kMMaxUnit && gi < ngu && ((has >> c) & 1u) && off) {
        const uint32_t gh0 = h0 + gi * A.haps_per_block, gh1 = min(gh0 + A.haps_per_block, A.n_haps);
        e0 = off[gh0];
        nw = (uint32_t)(off[gh1] - e0);
        narrow = (A.gnarrow && A.gnarrow[hg0 + gi]) ? kPoolNarrow : 0u;
    }
    const uint32_t np = pool_pairs(nw);
    uint32_t end = 0;
    for (uint32_t j = 0; j < kMMaxUnit; j++) {  // (by the whole wave)
        const uint32_t v = (uint32_t)__shfl((int)np, (int)(lane - gi + j));
        end += j <= gi ? v : 0u;
    }
    if (lane < 2 * kMMaxUnit) s_pool[c][gi] = make_uint4(end, nw | narrow, (uint32_t)e0, (uint32_t)(e0 >> 32));
}

// entry_onehot for a group of a unit: hd its resident descriptors, the words from the
// unit's LDS copy or global memory (two copies of the loads, no flat access).
template <int NK>
__device__ __forceinline__ void pool_onehot(const ScanArgs &A, const uint32_t *lwords, bool in_lds, const uint4 *hd,
                                            uint32_t we, const char *tab, v4i (&a)[NK]) {
    const uint4 d = hd[we & (kMMaxHapsPerBlock - 1)];
    const LaneHap hm{d.x, d.y, d.z, d.w};
    const uint32_t i = we >> 6;
    WinWords ww;
    if (in_lds) load_window(A, lwords, hm, i, ww);
    else load_window(A, A.words, hm, i, ww);
    build_onehot<NK>(hm, i, ww, tab, a);
}

// One super tile's window pairs over the lists of ALL the unit's groups for the tile's
// depth class: the waves draw pair p of the pool from s_hnext, find its group by three
// uniform compares with the running pair counts and score that group's pair p - the
// group's first -- two consecutive tiles of one group's list, cut as scan_loop cuts
// them.  No barrier inside a super tile: a group's descriptors are resident, its words
// come from the unit's LDS copy (lwords, the unit's first nlds groups) or from global
// memory (the base uniform in the wave, chosen per pair).  A queue record is labelled
// with the group of the pair that drains it, so the wave drains its queue whenever its
// next pair belongs to another group (wave-local), and after its last pair.
template <int NK>
__device__ __forceinline__ uint32_t scan_pool(const ScanArgs &A, const DevMSuper &S, const char *s_img,
                                              const uint32_t *lwords, uint32_t nlds, uint32_t h0, uint32_t slot,
                                              uint32_t ngu, uint32_t lane, uint32_t wave, uint32_t &qn, uint32_t &cn) {
    constexpr int c = NK > 2;
    const uint32_t hpb = A.haps_per_block;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pool[c][kMMaxUnit - 1].x);
    const float a0f = __uint_as_float(S.acc0);
    v16f cb = {a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f};
    asm volatile("" : "+v"(cb));  // kept in VGPRs: every round's MFMAs read it (no per-round copies)
    const int sa = lane < 32 ? kScaleD0 : kScaleD1;
    const char *tab = s_img - kMOnehotBytes;
    auto next_pair = [&]() {
        uint32_t p = 0;
        if (lane == 0) p = atomicAdd(&s_hnext, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane(p);
    };
    // pair p's group (gi) and list (G), all wave-uniform; returns the pair's index in the list
    auto place = [&](uint32_t p, GroupCtx &G, uint32_t &gi) {
        gi = 0;
        for (uint32_t u = 0; u + 1 < kMMaxUnit; u++)
            gi += p >= (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pool[c][u].x) ? 1u : 0u;
        const uint4 t = s_pool[c][gi];
        const uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x);
        const uint32_t y = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.y);
        const uint64_t e0 = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)t.z) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)t.w) << 32);
        G.wl = A.wlist[c] + e0;
        G.wl16 = (y & kPoolNarrow) ? A.wlist16[c] + e0 : nullptr;
        G.nw = y & ~kPoolNarrow;
        G.tile0 = S.tile0;
        G.h0 = h0 + gi * hpb;
        G.slot = slot;
        G.ub = unit_place(gi * hpb, ngu);
        return p - (end - pool_pairs(G.nw));
    };
    // lane l scores window row l & 31 of each tile
    auto entries = [&](const GroupCtx &G, uint32_t q, uint32_t &ea, uint32_t &eb) {
        const uint32_t r = kMWindows * 2 * q + (lane & 31);
        ea = G.at(min(r, G.nw - 1));
        eb = G.at(min(r + kMWindows, G.nw - 1));
    };
    uint32_t p = next_pair(), ea = 0, eb = 0, n_pairs = 0;
    if (p < total) {
        GroupCtx G;
        uint32_t gi;
        const uint32_t q = place(p, G, gi);
        entries(G, q, ea, eb);
    }
    while (p < total) {
        n_pairs++;
#ifdef TFBS_ROUND_PROF
        const unsigned long long tp0 = RPROF_T();
#endif
        GroupCtx G;
        uint32_t gi;
        const uint32_t q = place(p, G, gi);
        const uint32_t pn = next_pair();
        const bool two = 2 * q + 1 < (G.nw + kMWindows - 1) / kMWindows;
        v4i a0[NK], a1[NK];
        const bool in_lds = gi < nlds;
        const uint4 *hd = s_hdu + gi * hpb;
        pool_onehot<NK>(A, lwords, in_lds, hd, ea, tab, a0);
        pool_onehot<NK>(A, lwords, in_lds, hd, eb, tab, a1);  // (a copy of the last window when !two: unused)
        const uint32_t e0 = ea, e1 = eb;  // (the firing path's entries: the lane's own)
        uint32_t gn = gi;
        if (pn < total) {  // the next pair's entries, maybe another group's: in flight while this pair is scored
            GroupCtx Gn;
            const uint32_t qnx = place(pn, Gn, gn);
            entries(Gn, qnx, ea, eb);
        }
#ifdef TFBS_ROUND_PROF
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (as scan_loop: the A fragments awaited here)
        const unsigned long long tp1 = RPROF_T();
        RPROF_ADD(wave, 7, tp1 - tp0);
#endif
        if (two) scan_step<NK, true>(A, s_img, S.seg, G, lane, wave, a0, a1, 2 * q, e0, e1, cb, sa, qn, cn);
        else scan_step<NK, false>(A, s_img, S.seg, G, lane, wave, a0, a1, 2 * q, e0, e1, cb, sa, qn, cn);
        if (pn >= total || gn != gi) {  // the queue's records are this group's: decoded before another's join them
            drain_queue(A, G, qn, wave, lane, cn);
            qn = 0;
        }
        p = pn;
    }
    return n_pairs;
}

// words: the packed haplotype words, indexed by DevHap::word_off (an LDS copy
// of this workgroup's haplotypes, biased by their first word, or global memory).
// The group's window list (the windows of its haplotypes the class reads) is
// cut into tiles of 32 windows (the last one padded with its last window),
// handed to the waves two at a time from an LDS counter -- the waves finish
// together however the windows fall -- and the next pair's list entries are
// loaded while the current pair is scored.
// One super tile's window pairs over the group's list of its depth class, then the
// wave's last queue records decoded (qn, cn: the wave's queued records and listed
// candidates, carried over super tiles).  Returns the pairs this wave scored.
template <int NK>
__device__ __forceinline__ uint32_t scan_loop(const ScanArgs &A, const DevMSuper &S, const char *s_img,
                                              const uint32_t *words, uint32_t hg, uint32_t slot, uint32_t ub, uint32_t lane,
                                              uint32_t wave, uint32_t &qn, uint32_t &cn) {
    const uint32_t h0 = hg * A.haps_per_block;
    const uint32_t h1 = min(h0 + A.haps_per_block, A.n_haps);
    const uint64_t e0 = A.wlist_off[NK > 2][h0];
    GroupCtx G;
    G.wl = A.wlist[NK > 2] + e0;
    G.wl16 = (A.gnarrow && A.gnarrow[hg]) ? A.wlist16[NK > 2] + e0 : nullptr;
    G.nw = (uint32_t)(A.wlist_off[NK > 2][h1] - e0);
    G.tile0 = S.tile0;
    G.h0 = h0;
    G.slot = slot;
    G.ub = ub;
    const uint32_t ntile = (G.nw + kMWindows - 1) / kMWindows, npair = (ntile + 1) / 2;
    const float a0f = __uint_as_float(S.acc0);
    v16f cb = {a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f, a0f};
    asm volatile("" : "+v"(cb));  // kept in VGPRs: every round's MFMAs read it (no per-round copies)
    const int sa = lane < 32 ? kScaleD0 : kScaleD1;
    const char *tab = s_img - kMOnehotBytes;
    auto next_pair = [&]() {
        uint32_t p = 0;
        if (lane == 0) p = atomicAdd(&s_hnext, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane(p);
    };
    // lane l scores window row l & 31 of each tile
    auto entries = [&](uint32_t p, uint32_t &ea, uint32_t &eb) {
        const uint32_t q = kMWindows * 2 * p + (lane & 31);
        ea = G.at(min(q, G.nw - 1));
        eb = G.at(min(q + kMWindows, G.nw - 1));
    };
    uint32_t p = next_pair(), ea = 0, eb = 0, n_pairs = 0;
    if (p < npair) entries(p, ea, eb);
    while (p < npair) {
        n_pairs++;
#ifdef TFBS_ROUND_PROF
        const unsigned long long tp0 = RPROF_T();
#endif
        const uint32_t pn = next_pair();
        const bool two = 2 * p + 1 < ntile;
        v4i a0[NK], a1[NK];
        entry_onehot<NK>(A, words, ea, tab, a0);
        entry_onehot<NK>(A, words, eb, tab, a1);  // (a copy of the last window when !two: unused)
        const uint32_t e0 = ea, e1 = eb;          // (the firing path's entries: the lane's own)
        if (pn < npair) entries(pn, ea, eb);      // in flight while this pair is scored
#ifdef TFBS_ROUND_PROF
        // the A fragments awaited here (their LDS reads), so that the pair's first
        // round does not carry them
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long tp1 = RPROF_T();
        RPROF_ADD(wave, 7, tp1 - tp0);
#endif
        if (two) scan_step<NK, true>(A, s_img, S.seg, G, lane, wave, a0, a1, 2 * p, e0, e1, cb, sa, qn, cn);
        else scan_step<NK, false>(A, s_img, S.seg, G, lane, wave, a0, a1, 2 * p, e0, e1, cb, sa, qn, cn);
        p = pn;
    }
    drain_queue(A, G, qn, wave, lane, cn);  // (the records are self-contained: a drain per super tile)
    qn = 0;
    return n_pairs;
}

// LDS staging of a workgroup (a plain copy loop: batching all loads before the
// stores was slower, 2.84 -> 3.10 ms per C3 step).
__device__ __forceinline__ void stage_image(const ScanArgs &A, const DevMSuper &S, uint4 *dst) {
    const uint4 *src = reinterpret_cast<const uint4 *>(A.mimage + S.img_off / 4);
    const uint32_t n16 = S.img_bytes / 16;
    for (uint32_t i = threadIdx.x; i < n16; i += kMBlock) dst[kMOnehotBytes / 16 + i] = src[i];
}

// The one-hot table (4-mer code -> 64 bits, column t (16 bits) holds FP4 1.0 (0x2)
// in the nibble of its base): once per workgroup.
__device__ __forceinline__ void stage_onehot(int32_t *smem) {
    uint2 *tab = reinterpret_cast<uint2 *>(smem);
    for (uint32_t k = threadIdx.x; k < 256; k += kMBlock) {
        uint32_t h[4];
        for (int t = 0; t < 4; t++) h[t] = 2u << (4 * ((k >> (2 * t)) & 3));
        tab[k] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    }
}

// A group's descriptors and (STAGED) its packed words after the image budget; returns
// the words' base for DevHap::word_off (the kernels of one group per workgroup).
template <bool STAGED>
__device__ __forceinline__ const uint32_t *stage_group(const ScanArgs &A, int32_t *smem, uint32_t h0, uint32_t hn) {
    if (threadIdx.x < hn) {  // (32 of DevHap's 48 bytes; s_hd2: the rescoring's half)
        s_hd[threadIdx.x] = A.hd[h0 + threadIdx.x];
        s_hd2[threadIdx.x] = A.hd2[h0 + threadIdx.x];
    }
    if (!STAGED) return A.words;
    const uint4 f = A.hd[h0], l = A.hd[h0 + hn - 1];
    const uint32_t wbeg = f.x;
    const uint32_t wend = l.x + (l.y + 15) / 16 + 3;
    uint32_t *s_words = reinterpret_cast<uint32_t *>(smem) + (kMOnehotBytes + A.mimg_max + kMChunkBytes) / 4;
    for (uint32_t i = threadIdx.x; i < wend - wbeg; i += kMBlock) s_words[i] = A.words[wbeg + i];
    return s_words - wbeg;
}

// A unit's packed words, once per workgroup: its haplotypes are consecutive, so the words
// of its first ng groups (hn: the unit's haplotypes) are one range, from the first's
// word_off to the last's end as stage_group takes a group's, copied after the image
// budget when it fits the room the host reserved (A.unit_lds_words); *nlds = ng then,
// else 0 (every group of the unit reads global memory).  Returns the LDS base for
// DevHap::word_off.
__device__ __forceinline__ const uint32_t *stage_unit_words(const ScanArgs &A, int32_t *smem, uint32_t h0, uint32_t hn,
                                                            uint32_t ng, uint32_t *nlds) {
    uint32_t *s_words = reinterpret_cast<uint32_t *>(smem) + (kMOnehotBytes + A.mimg_max + kMChunkBytes) / 4;
    *nlds = 0;
    if (ng == 0) return s_words;
    const uint4 f = A.hd[h0], l = A.hd[h0 + min(ng * A.haps_per_block, hn) - 1];
    const uint32_t wbeg = f.x;
    const uint32_t wend = l.x + (l.y + 15) / 16 + 3;
    if (wend < wbeg || wend - wbeg > A.unit_lds_words) return s_words;
    for (uint32_t i = threadIdx.x; i < wend - wbeg; i += kMBlock) s_words[i] = A.words[wbeg + i];
    *nlds = ng;
    return s_words - wbeg;
}

}  // namespace
// post_scan_kernel's work by one workgroup of NT threads (defined below); s_sum: NT + 1
// words of LDS
template <uint32_t NT>
__device__ void post_one_block(const ScanArgs &A, uint32_t tid, uint32_t n_regions, uint32_t *__restrict__ bcnt,
                               uint32_t *__restrict__ boff, uint32_t *__restrict__ sorted,
                               uint32_t *__restrict__ report, uint32_t *__restrict__ need_wide, uint32_t *s_sum);
namespace {

// One workgroup per haplotype group for EVERY super tile (the depth classes in
// turn): the group's words, descriptors and one-hot table are staged once, each
// super tile's image in turn (a barrier on either side), and the wave rescores its
// candidates of all of them once at the end -- the per-workgroup costs (staging,
// the rescoring's dependent loads) are paid once per group, not once per super
// tile.  Grid: one workgroup per group (unit), 4 waves per SIMD (two workgroups per
// CU).  LDS: one-hot table | the largest image | (STAGED) words.
// UNIT: the workgroup's haplotypes are a unit of A.unit consecutive groups (the
// last unit may be short).  The one-hot table, the unit's descriptors (s_hdu) and, where
// the host gave them room (STAGED, A.unit_lds groups), the packed words of the unit's
// first groups are staged once per workgroup, each super tile's image once per unit; inside
// a super tile the waves draw the window pairs of all the unit's groups from one pool
// (scan_pool), with no barrier but the two around the image's staging.  The wave's
// candidates of all groups and super tiles share one list and are rescored once
// (rescore_list<true>); every group keeps its own slot for the hit lists and counts.
// !UNIT is the kernel of one group per workgroup.
template <bool STAGED, bool UNIT>
__global__ __launch_bounds__(kMBlock, 4) void scan_mfma_all_kernel(ScanArgs A) {
#ifdef TFBS_SCAN_PROF
    const unsigned long long t_start = __builtin_amdgcn_s_memtime(), r_start = __builtin_amdgcn_s_memrealtime();
#endif
    int32_t *smem = s_mdyn;
    const uint32_t hpb = A.haps_per_block;
    const uint32_t un = A.gorder ? A.gorder[blockIdx.x] : blockIdx.x;  // (its lists and stamps at its first slot)
    const uint32_t hg0 = UNIT ? un * A.unit : un;
    const uint32_t ngu = UNIT ? min(A.unit, (A.n_haps + hpb - 1) / hpb - hg0) : 1u;  // the unit's groups
    const uint32_t slot = A.region_base + hg0;
    const uint32_t h0 = hg0 * hpb;
    stage_onehot(smem);
    const uint32_t *words = nullptr;
    uint32_t nlds = 0;  // UNIT: the unit's first groups whose words are in the LDS
    if (!UNIT) {
        words = stage_group<STAGED>(A, smem, h0, min(h0 + hpb, A.n_haps) - h0);
    } else {
        const uint32_t hn = min(h0 + ngu * hpb, A.n_haps) - h0;
        if (threadIdx.x < hn) {
            s_hdu[threadIdx.x] = A.hd[h0 + threadIdx.x];
            s_hd2u[threadIdx.x] = A.hd2[h0 + threadIdx.x];
        }
        if (STAGED) words = stage_unit_words(A, smem, h0, hn, min(A.unit_lds, ngu), &nlds);
        if (threadIdx.x < 64) pool_fill(A, hg0, h0, ngu, threadIdx.x);
    }
    const char *s_img = reinterpret_cast<const char *>(smem) + kMOnehotBytes;
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t qn = 0, cn = 0, n_pairs = 0;
#ifdef TFBS_ROUND_PROF
    if (threadIdx.x < kMBlockWaves * 9) (&s_rprof[0][0])[threadIdx.x] = 0;
#endif
    for (uint32_t si = 0; si < A.n_msupers; si++) {
        const DevMSuper S = A.msupers[si];
#ifdef TFBS_ROUND_PROF
        const unsigned long long ts0 = RPROF_T();
#endif
        __syncthreads();  // the previous image's readers (and the pool's) are done
#ifdef TFBS_ROUND_PROF
        const unsigned long long ts1 = RPROF_T();
#endif
        stage_image(A, S, reinterpret_cast<uint4 *>(smem));
        if (threadIdx.x == 0) s_hnext = 0;
#ifdef TFBS_ROUND_PROF
        const unsigned long long ts2 = RPROF_T();
#endif
        __syncthreads();
#ifdef TFBS_ROUND_PROF
        {
            const unsigned long long ts3 = RPROF_T();
            if (si) RPROF_ADD(wave, 6, ts3 - ts0);
            RPROF_ADD(wave, 8, (ts1 - ts0) + (ts3 - ts2));  // the wave's wait at the super tile's barriers
        }
#endif
#ifdef TFBS_SCAN_PROF
        if (si == 0) {
            SCAN_STAMP(0, t_start);
            SCAN_STAMP(5, r_start);
            SCAN_STAMP(1, __builtin_amdgcn_s_memtime());
        }
#endif
        if (UNIT)
            n_pairs += S.nk > 2 ? scan_pool<4>(A, S, s_img, words, nlds, h0, slot, ngu, lane, wave, qn, cn)
                                : scan_pool<2>(A, S, s_img, words, nlds, h0, slot, ngu, lane, wave, qn, cn);
        else
            n_pairs += S.nk > 2 ? scan_loop<4>(A, S, s_img, words, hg0, slot, unit_place(0, 1), lane, wave, qn, cn)
                                : scan_loop<2>(A, S, s_img, words, hg0, slot, unit_place(0, 1), lane, wave, qn, cn);
    }
    (void)n_pairs;
    SCAN_STAMP(2, __builtin_amdgcn_s_memtime());
    if (UNIT) rescore_list<true>(A, A.words, h0, slot, ngu, wave, lane, cn);
    else rescore_list<false>(A, words, h0, slot, 1, wave, lane, cn);
    SCAN_STAMP(4, __builtin_amdgcn_s_memtime());
    SCAN_STAMP(6, __builtin_amdgcn_s_memrealtime());
    SCAN_STAMP(7, (unsigned long long)n_pairs | ((unsigned long long)cn << 32));
#ifdef TFBS_ROUND_PROF
    for (int k = 0; k < 8; k++) SCAN_STAMP(8 + k, s_rprof[wave][k]);
    SCAN_STAMP(3, s_rprof[wave][8]);  // the wait at the super tiles' barriers
#endif
    if (A.post_done) {  // fused post-scan: the last workgroup to finish does it
        __syncthreads();  // every wave's lists and spill records are written
        uint32_t *s_t = reinterpret_cast<uint32_t *>(&s_qdata[0][0]);  // (the queues are empty now)
        if (threadIdx.x == 0) {
            __threadfence();  // (release: this workgroup's records)
            s_t[0] = atomicAdd(A.post_done, 1u) == gridDim.x - 1 ? 1u : 0u;
        }
        __syncthreads();
        if (s_t[0]) {
            __threadfence();  // (acquire: every workgroup's records)
            post_one_block<kMBlock>(A, threadIdx.x, A.post_regions, A.post_bcnt, A.post_boff, A.post_sorted,
                                    A.post_report, A.post_need_wide, s_t + 4);
        }
    }
}

// Candidates past the waves' lists (drain_queue), one per thread; their
// hits go to the spill list.
__global__ __launch_bounds__(256) void cand_over_kernel(ScanArgs A) {
    const uint32_t n = min(A.over[1], A.cand_over_cap);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const uint32_t hap = A.cand_over[3 * (size_t)k], g = A.cand_over[3 * (size_t)k + 1];
        const DevHap hp = A.haps[hap];
        const uint32_t i = A.cand_over[3 * (size_t)k + 2];
        const CandHit R = score_candidate(A, A.words, CandHap::of(hp), hap, g, i);
        const uint32_t m0 = R.mask, key0 = R.key0;
        for (uint32_t m = m0; m; m &= m - 1) spill_record(A, hp.region, hap, key0 + __builtin_ctz(m));
        if (m0 && (hp.flags & HAP_DEDUP))  // shared windows: the sharers' pairs
            for_sharers(A, strand_class(A, g), hap, i, [&](uint32_t x) {
                for (uint32_t m = m0; m; m &= m - 1) spill_record(A, hp.region, A.hap_base + x, key0 + __builtin_ctz(m));
            });
    }
}

typedef void (*MfmaKernel)(ScanArgs);
MfmaKernel mfma_all_variant(bool staged, bool unit) {
    if (unit) return staged ? scan_mfma_all_kernel<true, true> : scan_mfma_all_kernel<false, true>;
    return staged ? scan_mfma_all_kernel<true, false> : scan_mfma_all_kernel<false, false>;
}

}  // namespace

// The scan's post-processing in one launch: every workgroup rescores its share of
// the overflow candidates (cand_over_kernel's work, when `cand`), then the last
// workgroup to finish -- the one whose ticket on *done (zeroed before) is the
// grid's last -- buckets the spill records by region on its own (post_buckets: region
// r's records end up at [boff[r], boff[r] + bcnt[r]) of sorted, boff[r] written only
// where bcnt[r] != 0; bcnt: 2 (n_regions + 1) words zeroed before, the counts and the
// scatter's fill counters): spills are rare, and no records (the usual case) costs
// one counter read.
constexpr uint32_t kPostBlock = 256;

// (spill_hist_wide_kernel's, more than kPostSerial records)
// boff[0 .. n_regions]: the exclusive prefix of the bucket counts (one workgroup of
// kPostBlock threads) -- each thread a run of consecutive buckets, one block scan of
// the runs' sums (not one per 256 buckets: 10 000 regions took 40 scans of 16
// barriers); the counts are zeroed for the scatter's fill counters
template <uint32_t NT = kPostBlock>
__device__ void spill_bucket_offsets(uint32_t tid, uint32_t n_regions, uint32_t *__restrict__ bcnt,
                                     uint32_t *__restrict__ boff, uint32_t *s_sum) {
    const uint32_t per = (n_regions + NT) / NT;  // ceil((n_regions + 1) / NT)
    const uint32_t i0 = min(tid * per, n_regions + 1), i1 = min(i0 + per, n_regions + 1);
    uint32_t mine = 0;
    for (uint32_t i = i0; i < i1; i++) mine += i < n_regions ? bcnt[i] : 0u;
    s_sum[tid] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < NT; o <<= 1) {
        const uint32_t t = tid >= o ? s_sum[tid - o] : 0u;
        __syncthreads();
        s_sum[tid] += t;
        __syncthreads();
    }
    uint32_t at = s_sum[tid] - mine;
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t v = i < n_regions ? bcnt[i] : 0u;
        boff[i] = at;
        at += v;
        if (i < n_regions) bcnt[i] = 0;
    }
}

// report (optional): the final overflow counters copied there by the last workgroup (the
// assembly's check, when its leftover pass -- which copies them otherwise -- is not
// launched); need_wide (optional: the wide kernels are not launched): set when the
// records are too many for the last workgroup, so that the host reruns the assembly
// with them.
// The overflow candidates' rescoring, block blk of nblk (NT threads): the hits' spill
// records get their slots one atomic per wave (C5: ~120 000 records through one
// counter, one atomic each, took ~1 ms); the loop is wave-uniform for the wave sum.
template <uint32_t NT>
__device__ void post_candidates(const ScanArgs &A, uint32_t tid, uint32_t blk, uint32_t nblk) {
    const uint32_t n = min(A.over[1], A.cand_over_cap), lane = tid & 63;
    for (uint32_t k0 = blk * NT; k0 < n; k0 += nblk * NT) {
        const uint32_t k = k0 + tid;
        uint32_t m = 0, key0 = 0, region = 0, hap = 0, sc = 0, si = 0, ns = 0;  // ns: sharers of the hit's window
        if (k < n) {
            hap = A.cand_over[3 * (size_t)k];
            const uint32_t g = A.cand_over[3 * (size_t)k + 1];
            const DevHap hp = A.haps[hap];
            region = hp.region;
            si = A.cand_over[3 * (size_t)k + 2];
            const CandHit R = score_candidate(A, A.words, CandHap::of(hp), hap, g, si);
            m = R.mask;
            key0 = R.key0;
            if (m && (hp.flags & HAP_DEDUP)) {
                sc = strand_class(A, g);
                for_sharers(A, sc, hap, si, [&](uint32_t) { ns++; });
            }
        }
        const uint32_t c = (uint32_t)__builtin_popcount(m) * (1 + ns);
        uint32_t inc = c;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= o) inc += t;
        }
        const uint32_t total = (uint32_t)__shfl((int)inc, 63);
        uint32_t base = 0;
        if (lane == 0 && total) base = atomicAdd(A.over, total);
        uint32_t at = (uint32_t)__shfl((int)base, 0) + inc - c;
        auto put = [&](uint32_t x) {
            for (uint32_t mm = m; mm; mm &= mm - 1, at++)
                if (at < A.spill_cap) {
                    A.spill[3 * (size_t)at] = region;
                    A.spill[3 * (size_t)at + 1] = x;
                    A.spill[3 * (size_t)at + 2] = key0 + __builtin_ctz(mm);
                }
        };
        if (m) put(hap);
        if (ns) for_sharers(A, sc, hap, si, [&](uint32_t x) { put(A.hap_base + x); });
    }
}

// The last workgroup's part (every workgroup's spill records visible): the overflow
// counters to report, then the records bucketed by region when they are few.
template <uint32_t NT>
__device__ void post_buckets(const ScanArgs &A, uint32_t tid, uint32_t n_regions, uint32_t *__restrict__ bcnt,
                             uint32_t *__restrict__ boff, uint32_t *__restrict__ sorted,
                             uint32_t *__restrict__ report, uint32_t *__restrict__ need_wide, uint32_t *s_sum) {
    if (report && tid < 2) report[tid] = __atomic_load_n(A.over + tid, __ATOMIC_RELAXED);
    const uint32_t n = min(__atomic_load_n(A.over, __ATOMIC_RELAXED), A.spill_cap);
    if (n == 0) return;  // no records: the readers skip the buckets (AsmArgs::spill_count)
    if (n > kPostSerial) {  // spill_hist_wide_kernel + spill_scatter_wide_kernel's
        if (need_wide && tid == 0) *need_wide = 1u;
        return;
    }
    // No pass over the regions: the record that finds its region's count at 0 is the
    // region's leader (bit k of lead: this thread's k-th record) and, the counts final,
    // takes the region's slots from a cursor in LDS -- the buckets lie in sorted in the
    // leaders' order.  The fill counters are a second zeroed array, so that bcnt keeps
    // the counts for the readers (AsmArgs::spill_cnt).
    static_assert(kPostSerial <= 32 * NT, "a thread's records: one bit each");
    uint32_t *bfill = bcnt + n_regions + 1;
    if (tid == 0) s_sum[0] = 0;
    uint32_t lead = 0;
    for (uint32_t e = tid, k = 0; e < n; e += NT, k++)
        if (atomicAdd(&bcnt[A.spill[3 * (size_t)e] & 0x7FFFFFFFu], 1u) == 0) lead |= 1u << k;
    __threadfence();  // (the counters' atomics seen by every thread of the block)
    __syncthreads();
    for (; lead; lead &= lead - 1) {
        const uint32_t r = A.spill[3 * (size_t)(tid + (uint32_t)__builtin_ctz(lead) * NT)] & 0x7FFFFFFFu;
        boff[r] = atomicAdd(&s_sum[0], __atomic_load_n(&bcnt[r], __ATOMIC_RELAXED));
    }
    __threadfence();  // (boff's stores seen by every thread of the block)
    __syncthreads();
    for (uint32_t e = tid; e < n; e += NT) {
        const uint32_t r = A.spill[3 * (size_t)e] & 0x7FFFFFFFu;
        const uint32_t at = boff[r] + atomicAdd(&bfill[r], 1u);
        sorted[3 * (size_t)at] = A.spill[3 * (size_t)e];
        sorted[3 * (size_t)at + 1] = A.spill[3 * (size_t)e + 1];
        sorted[3 * (size_t)at + 2] = A.spill[3 * (size_t)e + 2];
    }
}

template <uint32_t NT>
__device__ void post_one_block(const ScanArgs &A, uint32_t tid, uint32_t n_regions, uint32_t *__restrict__ bcnt,
                               uint32_t *__restrict__ boff, uint32_t *__restrict__ sorted,
                               uint32_t *__restrict__ report, uint32_t *__restrict__ need_wide, uint32_t *s_sum) {
    post_candidates<NT>(A, tid, 0, 1);
    __threadfence();  // (its spill records, for the whole block)
    __syncthreads();
    post_buckets<NT>(A, tid, n_regions, bcnt, boff, sorted, report, need_wide, s_sum);
}
// (the scan kernel's tail, instantiated above this definition)
template __device__ void post_one_block<kMBlock>(const ScanArgs &, uint32_t, uint32_t, uint32_t *, uint32_t *,
                                                 uint32_t *, uint32_t *, uint32_t *, uint32_t *);

__global__ __launch_bounds__(kPostBlock) void post_scan_kernel(ScanArgs A, uint32_t cand, uint32_t *done,
                                                              uint32_t n_regions, uint32_t *__restrict__ bcnt,
                                                              uint32_t *__restrict__ boff,
                                                              uint32_t *__restrict__ sorted,
                                                              uint32_t *__restrict__ report,
                                                              uint32_t *__restrict__ need_wide) {
    __shared__ uint32_t s_last, s_sum[kPostBlock];
    const uint32_t tid = threadIdx.x;
    if (cand) post_candidates<kPostBlock>(A, tid, blockIdx.x, gridDim.x);
    __syncthreads();
    if (tid == 0) {
        __threadfence();  // (release: this workgroup's spill records)
        s_last = atomicAdd(done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();  // (acquire: every workgroup's records)
    post_buckets<kPostBlock>(A, tid, n_regions, bcnt, boff, sorted, report, need_wide, s_sum);
}

// More than kPostSerial spill records: their bucket counts over the whole grid, then
// the last workgroup (finish ticket) the offsets; the scatter below, also over the
// grid (C5's ~120 000 records took ~1 ms in post_scan_kernel's last workgroup).
__global__ __launch_bounds__(kPostBlock) void spill_hist_wide_kernel(ScanArgs A, uint32_t *done, uint32_t n_regions,
                                                                     uint32_t *__restrict__ bcnt,
                                                                     uint32_t *__restrict__ boff) {
    __shared__ uint32_t s_last, s_sum[kPostBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = min(A.over[0], A.spill_cap);
    if (n <= kPostSerial) return;  // (uniform: post_scan_kernel bucketed them)
    for (uint32_t e = blockIdx.x * kPostBlock + tid; e < n; e += gridDim.x * kPostBlock)
        atomicAdd(&bcnt[A.spill[3 * (size_t)e] & 0x7FFFFFFFu], 1u);
    __syncthreads();
    if (tid == 0) {
        __threadfence();  // (release: this workgroup's counts)
        s_last = atomicAdd(done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();  // (acquire: every workgroup's counts)
    spill_bucket_offsets(tid, n_regions, bcnt, boff, s_sum);
}

__global__ __launch_bounds__(256) void spill_scatter_wide_kernel(ScanArgs A, const uint32_t *__restrict__ boff,
                                                                 uint32_t *__restrict__ bcnt,
                                                                 uint32_t *__restrict__ sorted) {
    const uint32_t n = min(A.over[0], A.spill_cap);
    if (n <= kPostSerial) return;  // (post_scan_kernel scattered them)
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const uint32_t r = A.spill[3 * (size_t)e] & 0x7FFFFFFFu;
        const uint32_t at = boff[r] + atomicAdd(&bcnt[r], 1u);
        sorted[3 * (size_t)at] = A.spill[3 * (size_t)e];
        sorted[3 * (size_t)at + 1] = A.spill[3 * (size_t)e + 1];
        sorted[3 * (size_t)at + 2] = A.spill[3 * (size_t)e + 2];
    }
}

int launch_post_fused(const ScanArgs &a, bool cand, uint32_t *done, uint32_t n_regions, uint32_t *bcnt, uint32_t *boff,
                      uint32_t *sorted, hipStream_t stream, bool wide, uint32_t *report, uint32_t *need_wide,
                      uint32_t cand_grid) {
    // (256 workgroups: 1 024 cost C2 14 us in dispatch and finish tickets and did not
    // speed up C5's rescoring; the wide scatter's 128 exit at once when there is nothing
    // for them -- and are left out when the batch's last assembly did not need them)
    hipLaunchKernelGGL(post_scan_kernel, dim3(cand ? cand_grid : 1), dim3(kPostBlock), 0, stream, a, cand ? 1u : 0u, done,
                       n_regions, bcnt, boff, sorted, report, wide ? nullptr : need_wide);
    if (wide) {
        hipLaunchKernelGGL(spill_hist_wide_kernel, dim3(128), dim3(kPostBlock), 0, stream, a, done + 1, n_regions, bcnt,
                           boff);
        hipLaunchKernelGGL(spill_scatter_wide_kernel, dim3(128), dim3(256), 0, stream, a, boff, bcnt, sorted);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("post_scan_kernel launch: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_post_scan(const ScanArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(cand_over_kernel, dim3(256), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("cand_over_kernel launch: ") + hipGetErrorString(e));
    return 1;
}

size_t mfma_lds_fixed() { return kMOnehotBytes; }

int launch_mfma_all(const ScanArgs &a0, const DevMSuper *supers, uint32_t n_supers, uint32_t group_words,
                    uint32_t n_haps, hipStream_t stream) {
    if (n_haps == 0 || n_supers == 0) return 0;
    const uint32_t hpb = a0.haps_per_block;
    const DevMSuper &last = supers[n_supers - 1];
    if ((uint64_t)(last.tile0 + last.tile_count) * kMStrands > (1u << 24) || hpb > kMMaxHapsPerBlock)
        return fail(TFBS_E_ARG, "matrix-core scan: more than 2^24 strands or 64 haplotypes per workgroup");
    const uint32_t n_hg = (n_haps + hpb - 1) / hpb;
    // slack kept in the budget (a retired 2 KiB array) so that the staging decisions below are unchanged
    constexpr size_t kMLdsSlack = 2048;
    const size_t static_lds =
        sizeof(s_qdata) + sizeof(s_qmeta) + sizeof(s_cand) + kMLdsSlack + sizeof(s_hnext) + sizeof(s_hd) + sizeof(s_hd2);
    size_t img_bytes = 0;
    for (uint32_t k = 0; k < n_supers; k++) img_bytes = std::max<size_t>(img_bytes, supers[k].img_bytes);
    const size_t base = kMOnehotBytes + img_bytes + kMChunkBytes;  // (the padding: scan_segment's B prefetch)
    const size_t staged_bytes = base + ((size_t)group_words * 4 + 15) / 16 * 16;
    bool staged = staged_bytes + static_lds <= kMStagedMax;
    // a unit of G groups per workgroup (ScanArgs::unit); G = 1: the kernel of one group
    const uint32_t G = std::min(std::max(a0.unit, 1u), kMMaxUnit);
    // A unit's words (ScanArgs::unit_words): k consecutive groups span at most k x
    // group_words, so that many of a unit's first groups have LDS words as fit beside the
    // largest image and the unit kernel's static LDS (the resident descriptors and the
    // pool instead of s_hd) under kMStagedMax (TFBS_SCAN_UNIT_WORDS=lds); the others' --
    // and all of a unit the room does not hold -- are read from global memory, as every
    // unit's are with "global" or unset.
    uint32_t unit_lds = 0;
    size_t unit_bytes = base;
    if (G > 1) {
        const size_t static_unit = static_lds - sizeof(s_hd) - sizeof(s_hd2) + sizeof(s_hdu) + sizeof(s_hd2u) + sizeof(s_pool) + 64;
        const size_t gw = std::max<size_t>(((size_t)group_words * 4 + 15) / 16 * 16, 16);
        const size_t room = kMStagedMax > base + static_unit ? kMStagedMax - base - static_unit : 0;
        // (the host's choice is global words: measured as fast as the LDS copy or faster for every G
        // at C3 and C2, DESIGN.md "Units"; the LDS copy only when forced)
        if (a0.unit_words == 1) unit_lds = (uint32_t)std::min<size_t>(G, room / gw);
        unit_bytes = base + unit_lds * gw;
        staged = unit_lds > 0;
    }
    const size_t lds = G > 1 ? unit_bytes : staged ? staged_bytes : base;
    const MfmaKernel kern = mfma_all_variant(staged, G > 1);
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024)
        e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("MFMA LDS attribute: ") + hipGetErrorString(e));
    int launches = 0;
    for (uint64_t g0 = 0; g0 < n_hg; g0 += kMLaunchGroups) {
        const uint32_t ng = (uint32_t)std::min<uint64_t>(kMLaunchGroups, n_hg - g0);
        const uint32_t h0 = (uint32_t)(g0 * hpb);
        ScanArgs a = a0;
        a.unit = G;
        a.unit_lds = unit_lds;
        a.unit_lds_words = (uint32_t)((unit_bytes - base) / 4);
        a.haps = a0.haps + h0;
        a.hd = a0.hd + h0;
        a.hd2 = a0.hd2 + h0;
        a.hap_base = a0.hap_base + h0;
        for (int c = 0; c < 2; c++) a.wlist_off[c] = a0.wlist_off[c] ? a0.wlist_off[c] + h0 : nullptr;
        a.gnarrow = a0.gnarrow ? a0.gnarrow + g0 : nullptr;
        a.n_haps = std::min<uint32_t>(n_haps - h0, ng * hpb);
        a.hits = a0.hits ? a0.hits + (size_t)h0 * a0.n_patterns_total * a0.hits_wpp : nullptr;
        // a group's lists are at its index in the batch, whichever launch scans it: the
        // key assembly indexes them directly (scan.hpp, hitl / hitn)
        a.region_base = (uint32_t)g0;
        a.mimg_max = (uint32_t)img_bytes;
        hipLaunchKernelGGL(kern, dim3((ng + G - 1) / G), dim3(kMBlock), lds, stream, a);
        launches++;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("scan_mfma_all_kernel launch: ") + hipGetErrorString(e));
    return launches;
}

}  // namespace tfbs
