// MI355X (gfx950) scan kernel for dinucleotide PWMs (TFBS_KIND_DIPWM).
//
// The score of the window starting at base i of a strand of L bases is the wrapping
// int32 sum of W[j][4 s[i+j] + s[i+j+1]] over its L - 1 transitions; a pair with an N
// adds 0; the window matches iff score > min_score, with the match range
// [pos_i, pos_i + L - 1].  The contract is scan_generic_kernel's: the grid is tiles x
// haplotype groups, every distinct haplotype is scanned whole, and the kernel stores
// the dense counts of its tile's pattern_id slots.
//
//  * A lane owns one window start i and funnel-shifts the 64-bit image of bases
//    i..i+31 out of three packed words, once per (haplotype, tile), as
//    scan_fast_kernel does.
//  * Strands are packed four to a unit (plan_dinuc.cpp).  Lookup block b of a unit is
//    indexed by the k-mer at bases (k-1) b .. (k-1) b + k - 1 of the image -- bits
//    [2 (k-1) b, 2 (k-1) b + 2k) -- and one ds_read_b128 returns the four strands'
//    partial sums over the k - 1 transitions inside it.  Bits past the image read as
//    zero: a strand of at most 32 bases has no transition there and its last block's
//    entries do not depend on them.
//  * N packs as A plus a per-haplotype bit mask; the windows whose first L bases hold
//    an N are rescored exactly, pair by pair, from the rows kept in global memory.
//  * A ballot of the threshold compare gates the inner-range counting (count_hits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "scan.hpp"
#include "scan_count.hpp"

namespace tfbs {
namespace {

constexpr int kChunks = 4;  // 64-window chunks per lane (256 windows per pass)
constexpr uint32_t kDiBlock = 512;
// minimum waves per SIMD: two workgroups per CU with k = 3 tiles (64 KiB at most), one
// with a k = 5 tile (up to 144 KiB)
constexpr int kDiMinWaves = kDiK == 3 ? 4 : 2;

typedef const __attribute__((address_space(4))) DevUnit CUnit;  // wave-uniform fields: scalar loads

// Exact score of the window starting at base i, pairs with an N adding 0.  Only
// lanes whose window contains an N run it.  nmbits: the N bits of bases i..i+L-1.
__device__ __noinline__ int32_t di_exact_score(const uint32_t *words, uint32_t i, uint32_t nmbits, uint32_t L,
                                               const int32_t *w16) {
    uint32_t s = 0;
    uint32_t a = (words[i >> 4] >> (2 * (i & 15))) & 3u;
    for (uint32_t j = 0; j + 1 < L; j++) {
        const uint32_t q = i + j + 1;
        const uint32_t b = (words[q >> 4] >> (2 * (q & 15))) & 3u;
        if (((nmbits >> j) & 3u) == 0) s += (uint32_t)w16[16 * j + 4 * a + b];
        a = b;
    }
    return (int32_t)s;
}

// Score NCH 64-window chunks starting at window cg against every unit of the tile.
template <int NCH>
__device__ __forceinline__ void di_chunks(const ScanArgs &A, const DevTile &t, const char *s_lut, CUnit *units,
                                          const DevHap &hm, uint32_t h, uint32_t cg, const int32_t *inner,
                                          uint32_t n_pass, bool write_hits, uint32_t lane,
                                          uint32_t (&acc)[kMaxInnerPass]) {
    const bool has_n = (hm.flags & HAP_HAS_N) != 0;
    const bool has_pos = (hm.flags & HAP_HAS_POS) != 0;
    uint64_t img[NCH];  // bases i..i+31, 2 bits each
    int32_t rem[NCH];   // bases from the window start to the haplotype end
    int32_t pos[NCH];   // pos_i relative to ext_start
    uint32_t nm[NCH];   // N bits of bases i..i+31
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t i = cg + 64 * c + lane;
        const uint32_t ic = min(i, hm.len);  // keep reads inside the +3 word pad
        const uint32_t *w = A.words + hm.word_off + (ic >> 4);
        const uint32_t sh = 2 * (ic & 15);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh);
        const uint32_t hi = __builtin_amdgcn_alignbit(w2, w1, sh);
        img[c] = ((uint64_t)hi << 32) | lo;
        rem[c] = (int32_t)hm.len - (int32_t)i;
        pos[c] = has_pos ? (i < hm.len ? A.posrel[hm.pos_off + i] : 0) : (int32_t)i;
        if (has_n) {
            const uint32_t *m = A.nmask + hm.nmask_off + (ic >> 5);
            nm[c] = __builtin_amdgcn_alignbit(m[1], m[0], ic & 31);
        } else {
            nm[c] = 0;
        }
    }
    for (uint32_t ui = 0; ui < t.last - t.first; ui++) {
        CUnit &U = units[ui];
        const char *base = s_lut + (size_t)U.lut_off * kDiBlockBytes;
        const uint32_t nblk = U.nblk;
        uint32_t sum[NCH][4];
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int d = 0; d < 4; d++) sum[c][d] = 0u;
        for (uint32_t b = 0; b < nblk; b++) {  // (wave-uniform trip count, at most kDiMaxBlocks)
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint32_t code = (uint32_t)(img[c] >> (2 * kDiStride * b)) & (uint32_t)(kDiCodes - 1);
                const uint4 v = *reinterpret_cast<const uint4 *>(base + b * kDiBlockBytes + (code << 4));
                sum[c][0] += v.x;
                sum[c][1] += v.y;
                sum[c][2] += v.z;
                sum[c][3] += v.w;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if ((uint32_t)s >= U.nstrand) break;
            const uint32_t L = U.len[s];
            const int32_t min_score = U.min_score[s];
            uint64_t hit[NCH];
            uint64_t any = 0;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const bool valid = rem[c] >= (int32_t)L;
                bool hb = (int32_t)sum[c][s] > min_score;
                if (has_n) {
                    const uint32_t lm = L >= 32 ? 0xFFFFFFFFu : ((1u << L) - 1u);
                    const uint32_t m = nm[c] & lm;
                    if (m && valid)
                        hb = di_exact_score(A.words + hm.word_off, cg + 64 * c + lane, m, L,
                                            A.wfull + 16 * (size_t)U.wofs[s]) > min_score;
                }
                hit[c] = __ballot(hb && valid);
                any |= hit[c];
            }
            if (__builtin_expect(write_hits, 0) && lane == 0) {
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const uint32_t wi = cg / 64 + c;
                    if (wi < A.hits_wpp)
                        A.hits[((size_t)h * A.n_patterns_total + U.orig_index[s]) * A.hits_wpp + wi] = hit[c];
                }
            }
            if (__builtin_expect(any != 0, 0)) count_hits<NCH>(hit, pos, L, inner, n_pass, U.slot_local[s], lane, acc);
        }
    }
}

// Grid: n_tiles x ceil(n_haps / haps_per_block); 512 threads.  LDS: the tile's blocks.
__global__ __launch_bounds__(kDiBlock, kDiMinWaves) void scan_dinuc_kernel(ScanArgs A) {
    extern __shared__ __attribute__((aligned(16))) int32_t smem[];
    constexpr uint32_t kWaves = kDiBlock / 64;
    const uint32_t tile_idx = blockIdx.x % A.n_tiles;
    const uint32_t hg = blockIdx.x / A.n_tiles;
    const DevTile t = A.tiles[tile_idx];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(A.lut + (size_t)t.lut_begin * kDiBlockInts);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        const uint32_t n4 = t.nblocks * (kDiBlockInts / 4);
        for (uint32_t i = threadIdx.x; i < n4; i += kDiBlock) dst[i] = src[i];
    }
    __syncthreads();
    const char *s_lut = reinterpret_cast<const char *>(smem);
    CUnit *units = (CUnit *)(A.units + t.first);

    for (uint32_t hh = wave; hh < A.haps_per_block; hh += kWaves) {
        const uint32_t h = hg * A.haps_per_block + hh;
        if (h >= A.n_haps) break;
        const DevHap hm = A.haps[h];
        const DevRegion rg = A.regions[hm.region];
        const uint32_t n_inner = rg.n_inner;
        const uint32_t nwin = hm.len >= t.lmin ? hm.len - t.lmin + 1 : 0;
        // no inner range: nothing to count (a pass for the hit bitmaps of tfbs_matches);
        // more than kMaxInnerPass: the windows are scored once per pass of ranges
        const uint32_t n_passes =
            n_inner == 0 ? (A.hits ? 1u : 0u) : (n_inner + kMaxInnerPass - 1) / kMaxInnerPass;
        for (uint32_t pass = 0; pass < n_passes; pass++) {
            const uint32_t k0 = pass * kMaxInnerPass;
            const uint32_t n_pass = n_inner > k0 ? min((uint32_t)kMaxInnerPass, n_inner - k0) : 0u;
            const int32_t *inner = A.inner + 2 * (size_t)(rg.inner_off + k0);
            uint32_t acc[kMaxInnerPass];
#pragma unroll
            for (int kk = 0; kk < kMaxInnerPass; kk++) acc[kk] = 0;
            const bool write_hits = A.hits != nullptr && pass == 0;
            for (uint32_t cg = 0; cg < nwin; cg += 64 * kChunks) {
                const uint32_t nch = min((uint32_t)kChunks, (nwin - cg + 63) / 64);
                if (nch >= 3)  // a 3-chunk tail scores one chunk of invalid windows (rem < L)
                    di_chunks<4>(A, t, s_lut, units, hm, h, cg, inner, n_pass, write_hits, lane, acc);
                else if (nch == 2)
                    di_chunks<2>(A, t, s_lut, units, hm, h, cg, inner, n_pass, write_hits, lane, acc);
                else
                    di_chunks<1>(A, t, s_lut, units, hm, h, cg, inner, n_pass, write_hits, lane, acc);
            }
            if (n_pass && lane < t.nslots) {
                const size_t st = rg.count_stride;
                uint32_t *out = A.counts + hm.count_off + ((size_t)(t.slot_begin + lane) * n_inner + k0) * st;
#pragma unroll
                for (int kk = 0; kk < kMaxInnerPass; kk++)
                    if ((uint32_t)kk < n_pass) out[kk * st] = acc[kk];
            }
        }
    }
}

}  // namespace

int dinuc_kernel_set_lds(size_t lds_bytes) {
    if (lds_bytes <= 64 * 1024) return TFBS_OK;
    hipError_t e = hipFuncSetAttribute((const void *)scan_dinuc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds_bytes);
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("LDS attribute: ") + hipGetErrorString(e));
    return TFBS_OK;
}

// Grids stay below 2^31 workgroups by splitting along haplotype groups.
int launch_dinuc(const ScanArgs &a0, size_t lds_bytes, uint32_t n_haps, hipStream_t stream) {
    if (n_haps == 0 || a0.n_tiles == 0) return 0;
    const uint32_t hpb = a0.haps_per_block;
    const uint32_t n_hg = (n_haps + hpb - 1) / hpb;
    const uint64_t max_hg = std::max<uint64_t>(1, (1ull << 31) / a0.n_tiles - 1);
    int launches = 0;
    for (uint64_t g0 = 0; g0 < n_hg; g0 += max_hg) {
        const uint32_t ng = (uint32_t)std::min<uint64_t>(max_hg, n_hg - g0);
        const uint32_t h0 = (uint32_t)(g0 * hpb);
        ScanArgs a = a0;
        a.haps = a0.haps + h0;
        a.n_haps = std::min<uint32_t>(n_haps - h0, ng * hpb);
        a.hits = a0.hits ? a0.hits + (size_t)h0 * a0.n_patterns_total * a0.hits_wpp : nullptr;
        hipLaunchKernelGGL(scan_dinuc_kernel, dim3(a0.n_tiles * ng), dim3(kDiBlock), lds_bytes, stream, a);
        launches++;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("scan_dinuc_kernel launch: ") + hipGetErrorString(e));
    return launches;
}

}  // namespace tfbs
