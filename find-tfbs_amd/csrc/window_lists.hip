// Window lists of the matrix-core scan (ScanArgs::wlist, scan.hpp): which windows of
// which haplotype the scan kernel (scan_mfma.hip) reads, built on the device when a
// batch is uploaded -- the per-haplotype counts, an exclusive scan into offsets, the
// fill; with shared windows, the donors' sharer entries too -- and the small kernels
// that go with them: the compact haplotype descriptors (ScanArgs::hd), the groups'
// costs for the scan's workgroup order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "scan.hpp"

namespace tfbs {
namespace {

// ---------------------------------------------------------------------------
// Window lists (ScanArgs::wlist): per depth class of span S, the windows [0, len
// - lmin + 1) of every haplotype, only those meeting a diff run for a HAP_DEDUP
// haplotype (tfbs_internal.hpp): f(lo, hi) gets them as ascending intervals.
template <class F>
__device__ __forceinline__ uint32_t for_windows(const DevHap &hm, const uint32_t *druns, uint32_t lmin, uint32_t S,
                                                uint32_t dedup, F &&f) {
    if (hm.len < lmin) return 0;
    const uint32_t nw = hm.len - lmin + 1;
    if (!dedup || !(hm.flags & HAP_DEDUP)) {
        f(0u, nw);
        return nw;
    }
    uint32_t n = 0, next = 0;  // windows below next are listed
    for (uint32_t k = 0; k < hm.n_druns; k++) {
        const uint32_t a = druns[2 * (hm.drun_off + k)], b = druns[2 * (hm.drun_off + k) + 1];
        const uint32_t lo = max(next, a >= S - 1 ? a - (S - 1) : 0u), hi = min(b, nw - 1) + 1;
        if (hi > lo) {
            f(lo, hi);
            n += hi - lo;
            next = hi;
        }
    }
    return n;
}

__global__ __launch_bounds__(256) void wl_count_kernel(const DevHap *__restrict__ haps, uint32_t n,
                                                       const uint32_t *__restrict__ druns, uint32_t lmin, uint32_t S,
                                                       uint32_t dedup, uint64_t *__restrict__ cnt) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h > n) return;
    cnt[h] = h < n ? for_windows(haps[h], druns, lmin, S, dedup, [](uint32_t, uint32_t) {}) : 0u;
}

// one wave per haplotype: its entries written 64 at a time
__global__ __launch_bounds__(256) void wl_fill_kernel(const DevHap *__restrict__ haps, uint32_t n,
                                                      const uint32_t *__restrict__ druns, uint32_t lmin, uint32_t S,
                                                      uint32_t dedup, uint32_t hpb, const uint64_t *__restrict__ off,
                                                      uint32_t *__restrict__ list, uint16_t *__restrict__ list16,
                                                      const uint8_t *__restrict__ gnarrow) {
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= n) return;
    uint64_t at = off[h];
    const uint32_t hl = h % hpb;
    const bool narrow = gnarrow && gnarrow[h / hpb];
    for_windows(haps[h], druns, lmin, S, dedup, [&](uint32_t lo, uint32_t hi) {
        for (uint32_t w = lo + lane; w < hi; w += 64) {
            if (narrow) list16[at + (w - lo)] = (uint16_t)((w << 6) | hl);
            else list[at + (w - lo)] = (w << 6) | hl;
        }
        at += hi - lo;
    });
}

// ---------------------------------------------------------------------------
// Shared windows.  Haplotypes of one region mostly differ at sites far apart, so near
// any one site many of them are base for base the same: window i of a depth class of
// span S is *shared* by two HAP_DEDUP haplotypes of the region without indels or N, of
// equal length, when it is dirty in both and their bases AND diff columns on [i, i + S)
// (clipped to the length) are equal -- the exact 64-bit base image and 32-bit column
// mask are compared, no hash.  The lowest-indexed such haplotype is the window's
// *donor*: only the donor lists it; the others (its sharers) get one (sharer, [i_lo,
// i_hi)) entry per run of consecutive windows taken from the same donor, in the
// donor's entry range (ScanArgs::share), and the rescoring lists a donor's hits for
// every sharer whose entry covers the window.  That is exact: position, inner ranges
// and length are the region's, score and the dirty-for-L test depend only on the
// window's bases and diff columns.  Everything else (the reference, a helper, indel
// or N haplotypes, haplotypes scanned whole) lists its windows as before.
__device__ __forceinline__ bool hap_shares(uint32_t flags) {
    return (flags & (HAP_DEDUP | HAP_REF | HAP_HAS_POS | HAP_HAS_N)) == HAP_DEDUP;
}
// bit j: column i + j (j < n <= 32) lies in one of the haplotype's diff runs
__device__ __forceinline__ uint32_t run_mask(const uint32_t *__restrict__ druns, uint32_t off, uint32_t nr, uint32_t i,
                                             uint32_t n) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < nr; k++) {
        const uint32_t a = druns[2 * (off + k)], b = druns[2 * (off + k) + 1];
        const uint32_t lo = max(a, i), hi = min(b, i + n - 1);
        if (hi < lo) continue;  // (also a boundary run [a, a - 1])
        const uint32_t cnt = hi - lo + 1;
        m |= (cnt >= 32 ? 0xFFFFFFFFu : (1u << cnt) - 1) << (lo - i);
    }
    return m;
}
// the 2-bit bases of columns [i, i + n), n <= 32 (the words carry 3 pad words)
__device__ __forceinline__ uint64_t window_bases(const uint32_t *__restrict__ words, uint32_t word_off, uint32_t i,
                                                 uint32_t n) {
    const uint32_t *w = words + word_off + (i >> 4);
    const uint32_t sh = 2 * (i & 15);
    const uint64_t v = (uint64_t)__builtin_amdgcn_alignbit(w[1], w[0], sh) |
                       ((uint64_t)__builtin_amdgcn_alignbit(w[2], w[1], sh) << 32);
    return n >= 32 ? v : v & ((1ull << (2 * n)) - 1);
}

// The donor of window i of haplotype h (hm; `active` lanes, one window each, windows
// [c_lo, c_hi] over the wave): the lowest-indexed haplotype of the region sharing it,
// h itself when none does.  h and hm are wave-uniform.
__device__ __forceinline__ uint32_t find_donor(const DevHap *__restrict__ haps, const DevRegion *__restrict__ regions,
                                               const uint32_t *__restrict__ druns, const uint32_t *__restrict__ words,
                                               uint32_t h, const DevHap &hm, uint32_t i, bool active, uint32_t S,
                                               uint32_t c_lo, uint32_t c_hi, uint32_t lane) {
    if (!hap_shares(hm.flags)) return h;
    const uint32_t n = active ? min(S, hm.len - i) : 1u;
    const uint32_t ii = active ? i : 0u;
    const uint32_t rm = run_mask(druns, hm.drun_off, hm.n_druns, ii, n);
    const uint64_t key = window_bases(words, hm.word_off, ii, n);
    uint32_t donor = h;
    uint64_t open = __ballot(active);
    // 64 lower-indexed haplotypes at a time, one per lane: those that may share (some run
    // of theirs meets the columns of the wave's windows); then the wave compares its
    // windows with each of them in ascending order
    for (uint32_t b0 = regions[hm.region].hap_begin; b0 < h && open; b0 += 64) {
        bool cand = false;
        if (b0 + lane < h) {
            const DevHap o = haps[b0 + lane];
            if (hap_shares(o.flags) && o.len == hm.len)
                for (uint32_t k = 0; k < o.n_druns && !cand; k++)
                    cand = druns[2 * (o.drun_off + k)] <= c_hi + S - 1 && druns[2 * (o.drun_off + k) + 1] >= c_lo;
        }
        for (uint64_t cm = __ballot(cand); cm && open; cm &= cm - 1) {
            const uint32_t h2 = b0 + (uint32_t)__builtin_ctzll(cm);
            const uint32_t o_runs = haps[h2].drun_off, o_nr = haps[h2].n_druns, o_words = haps[h2].word_off;
            bool eq = false;
            if (active && donor == h && run_mask(druns, o_runs, o_nr, ii, n) == rm)
                eq = window_bases(words, o_words, ii, n) == key;
            if (eq) donor = h2;
            open &= ~__ballot(eq);
        }
    }
    return donor;
}

// One wave per haplotype h, its listed windows (for_windows) 64 at a time: f(w, active,
// donor) with the lane's window, whether it has one, and the window's donor.
template <class F>
__device__ __forceinline__ void for_shared_windows(const DevHap *__restrict__ haps,
                                                   const DevRegion *__restrict__ regions,
                                                   const uint32_t *__restrict__ druns,
                                                   const uint32_t *__restrict__ words, uint32_t h, const DevHap &hm,
                                                   uint32_t lmin, uint32_t S, uint32_t lane, F &&f) {
    for_windows(hm, druns, lmin, S, 1u, [&](uint32_t lo, uint32_t hi) {
        for (uint32_t w0 = lo; w0 < hi; w0 += 64) {
            const uint32_t w = w0 + lane;
            const bool active = w < hi;
            f(w, active, find_donor(haps, regions, druns, words, h, hm, w, active, S, w0, min(w0 + 63, hi - 1), lane));
        }
    });
}

// Of the lanes with `sh` (a sharer's window, its donor d): whether the lane starts a
// run of consecutive lanes with the same donor, and the run's length.
__device__ __forceinline__ bool sharer_run(bool sh, uint32_t d, uint32_t lane, uint32_t *len) {
    const uint32_t pd = (uint32_t)__shfl_up((int)d, 1);
    const bool psh = __shfl_up((int)sh, 1) != 0;
    const bool start = sh && (lane == 0 || !psh || pd != d);
    const uint64_t cont = __ballot(sh && !start);
    const uint64_t after = lane == 63 ? 0ull : cont >> (lane + 1);
    *len = 1 + (uint32_t)__builtin_ctzll(~after);
    return start;
}

// cnt[h]: the windows haplotype h lists itself; scnt[d] += the sharer entries of donor
// d (zeroed before); hstat[2 h], [2 h + 1]: the (window, strand) pairs and cells of the
// windows h lists (tab: the class's strand lengths).
__global__ __launch_bounds__(256) void wl_share_count_kernel(const DevHap *__restrict__ haps, uint32_t n,
                                                             const DevRegion *__restrict__ regions,
                                                             const uint32_t *__restrict__ druns,
                                                             const uint32_t *__restrict__ words, uint32_t lmin,
                                                             uint32_t S, const ClassTab *__restrict__ tab,
                                                             uint64_t *__restrict__ cnt,
                                                             unsigned long long *__restrict__ scnt,
                                                             uint32_t *__restrict__ hstat) {
    const uint32_t h = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (h > n) return;
    if (h == n) {
        if (lane == 0) cnt[n] = 0;
        return;
    }
    const DevHap hm = haps[h];
    uint32_t own = 0, rw = 0, rc = 0;
    for_shared_windows(haps, regions, druns, words, h, hm, lmin, S, lane, [&](uint32_t w, bool active, uint32_t d) {
        const bool mine = active && d == h;
        own += (uint32_t)__popcll(__ballot(mine));
        uint32_t len;
        if (sharer_run(active && !mine, d, lane, &len)) atomicAdd(scnt + d, 1ull);
        if (mine) {
            const uint32_t r = min(hm.len - w, 32u);
            rw += tab->w[r];
            rc += tab->c[r];
        }
    });
    for (uint32_t o = 32; o; o >>= 1) {
        rw += (uint32_t)__shfl_down((int)rw, o);
        rc += (uint32_t)__shfl_down((int)rc, o);
    }
    if (lane == 0) {
        cnt[h] = own;
        hstat[2 * (size_t)h] = rw;
        hstat[2 * (size_t)h + 1] = rc;
    }
}

// The haplotype's own windows to its list range (ascending), its sharer entries to
// their donors' ranges (soff; scur: fill cursors, zeroed before).
__global__ __launch_bounds__(256) void wl_share_fill_kernel(const DevHap *__restrict__ haps, uint32_t n,
                                                            const DevRegion *__restrict__ regions,
                                                            const uint32_t *__restrict__ druns,
                                                            const uint32_t *__restrict__ words, uint32_t lmin, uint32_t S,
                                                            uint32_t hpb, const uint64_t *__restrict__ off,
                                                            uint32_t *__restrict__ list, uint16_t *__restrict__ list16,
                                                            const uint8_t *__restrict__ gnarrow,
                                                            const uint64_t *__restrict__ soff,
                                                            uint32_t *__restrict__ scur, uint2 *__restrict__ share) {
    const uint32_t h = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (h >= n) return;
    const DevHap hm = haps[h];
    uint64_t at = off[h];
    const uint64_t end = off[h + 1];
    const uint32_t hl = h % hpb;
    const bool narrow = gnarrow && gnarrow[h / hpb];
    for_shared_windows(haps, regions, druns, words, h, hm, lmin, S, lane, [&](uint32_t w, bool active, uint32_t d) {
        const bool own = active && d == h;
        const uint64_t ob = __ballot(own);
        const uint64_t q = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(ob >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ob, 0));
        if (own && q < end) {  // (q < end: the count pass's number, whatever happens)
            if (narrow) list16[q] = (uint16_t)((w << 6) | hl);
            else list[q] = (w << 6) | hl;
        }
        at += (uint32_t)__popcll(ob);
        uint32_t len;
        if (sharer_run(active && d != h, d, lane, &len)) {
            const uint64_t e = soff[d] + atomicAdd(scur + d, 1u);
            if (e < soff[d + 1]) share[e] = make_uint2(h, w | ((w + len) << 16));
        }
    });
}

// sum[0], sum[1] += the even and the odd words of x[0 .. 2 n)
__global__ __launch_bounds__(256) void pair_sum_kernel(const uint32_t *__restrict__ x, uint32_t n,
                                                       unsigned long long *__restrict__ sum) {
    unsigned long long a = 0, b = 0;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        a += x[2 * (size_t)k];
        b += x[2 * (size_t)k + 1];
    }
    for (uint32_t o = 32; o; o >>= 1) {
        a += (unsigned long long)__shfl_down((long long)a, o);
        b += (unsigned long long)__shfl_down((long long)b, o);
    }
    if ((threadIdx.x & 63) == 0 && (a | b)) {
        atomicAdd(sum, a);
        atomicAdd(sum + 1, b);
    }
}

__global__ __launch_bounds__(256) void group_cost_kernel(const uint64_t *__restrict__ off0,
                                                         const uint64_t *__restrict__ off1, uint32_t n_haps, uint32_t hpb,
                                                         uint32_t n_groups, uint32_t w0, uint32_t w1,
                                                         uint32_t *__restrict__ cost) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t h0 = g * hpb, h1 = min(h0 + hpb, n_haps);
    uint64_t c = 0;
    if (off0) c += (off0[h1] - off0[h0] + 2 * kMWindows - 1) / (2 * kMWindows) * w0;
    if (off1) c += (off1[h1] - off1[h0] + 2 * kMWindows - 1) / (2 * kMWindows) * w1;
    cost[g] = (uint32_t)min<uint64_t>(c, 0xFFFFFFFFu);
}

// The scan's compact haplotype descriptors (ScanArgs::hd): word offset, length,
// flags, N-mask offset of every DevHap.
__global__ __launch_bounds__(256) void hd_kernel(const DevHap *__restrict__ haps, uint32_t n, uint4 *__restrict__ hd,
                                                  uint4 *__restrict__ hd2) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h < n) {
        const DevHap x = haps[h];
        hd[h] = make_uint4(x.word_off, x.len, x.flags, x.nmask_off);
        hd2[h] = make_uint4(x.region, x.pos_off, x.drun_off, x.n_druns);
    }
}

// The key assembly's static records (launch_region_asm, scan.hpp): a wave per region,
// one pass for the region's span of runs and its longest haplotype, one for the
// haplotypes' descriptors against that span's start.
__global__ __launch_bounds__(256) void region_asm_kernel(const DevHap *__restrict__ haps,
                                                          const DevRegion *__restrict__ regions, uint32_t n_regions,
                                                          uint32_t *__restrict__ hap_reuse, uint4 *__restrict__ region_asm) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6); r < n_regions; r += gridDim.x * 4) {
        const DevRegion rg = regions[r];
        uint32_t lo = UINT32_MAX, hi = 0, lmax = 0;
        for (uint32_t l = lane; l < rg.hap_count; l += 64) {
            const DevHap &h = haps[rg.hap_begin + l];
            lmax = max(lmax, h.len);
            if (h.flags & HAP_DEDUP) {  // its runs in the reference's columns
                lo = min(lo, h.rrun_off);
                hi = max(hi, h.rrun_off + h.n_rruns);
            }
        }
        if (lane == 0 && rg.ref_hap != UINT32_MAX) lmax = max(lmax, haps[rg.ref_hap].len);  // (R's haplotype)
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor((int)lo, o));
            hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
            lmax = max(lmax, (uint32_t)__shfl_xor((int)lmax, o));
        }
        for (uint32_t l = lane; l < rg.hap_count; l += 64) {
            const DevHap &h = haps[rg.hap_begin + l];
            hap_reuse[rg.hap_begin + l] = (h.flags & HAP_DEDUP) ? (h.rrun_off - lo) | (h.n_rruns << 16) : UINT32_MAX;
        }
        if (lane == 0) region_asm[r] = make_uint4(lo, lo == UINT32_MAX ? 0u : hi - lo, lmax, 0u);
    }
}

// In-place exclusive scan of u64 values, 4096 per workgroup; sums[b] = tile b's total.
constexpr uint32_t kScanThreads = 1024, kScanTile = 4 * kScanThreads;
__global__ __launch_bounds__(kScanThreads) void scan_tile_kernel(uint64_t *__restrict__ x, uint64_t n,
                                                                 uint64_t *__restrict__ sums) {
    __shared__ uint64_t s[2][kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + 4 * t;
    uint64_t v[4], tot = 0;
    for (int k = 0; k < 4; k++) {
        v[k] = base + k < n ? x[base + k] : 0;
        tot += v[k];
    }
    int cur = 0;
    s[0][t] = tot;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= o ? s[cur][t - o] : 0);
        cur ^= 1;
        __syncthreads();
    }
    uint64_t run = s[cur][t] - tot;
    for (int k = 0; k < 4; k++) {
        if (base + k < n) x[base + k] = run;
        run += v[k];
    }
    if (t == kScanThreads - 1) sums[blockIdx.x] = s[cur][t];
}

__global__ __launch_bounds__(256) void scan_add_kernel(uint64_t *__restrict__ x, uint64_t n,
                                                       const uint64_t *__restrict__ sums) {
    const uint64_t add = sums[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < kScanTile; k += 256) {
        const uint64_t i = (uint64_t)blockIdx.x * kScanTile + k;
        if (i < n) x[i] += add;
    }
}

}  // namespace

int exclusive_scan(uint64_t *x, uint64_t n, uint64_t *tmp, hipStream_t stream) {
    const uint64_t nt = (n + kScanTile - 1) / kScanTile;
    if (nt == 0) return TFBS_OK;
    hipLaunchKernelGGL(scan_tile_kernel, dim3((uint32_t)nt), dim3(kScanThreads), 0, stream, x, n, tmp);
    if (nt > 1) {
        if (int rc = exclusive_scan(tmp, nt, tmp + nt, stream)) return rc;
        hipLaunchKernelGGL(scan_add_kernel, dim3((uint32_t)nt), dim3(256), 0, stream, x, n, tmp);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("scan kernels: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_region_asm(const DevHap *haps, uint32_t n_haps, const DevRegion *regions, uint32_t n_regions,
                      uint32_t *hap_reuse, uint4 *region_asm, hipStream_t stream) {
    // (a haplotype of no region's hap_count -- a helper reference -- reuses nothing)
    hipError_t e = hipMemsetAsync(hap_reuse, 0xFF, (size_t)std::max<uint32_t>(n_haps, 1) * 4, stream);
    if (e == hipSuccess && n_regions) {
        hipLaunchKernelGGL(region_asm_kernel, dim3(std::min<uint32_t>((n_regions + 3) / 4, 2048)), dim3(256), 0, stream, haps,
                           regions, n_regions, hap_reuse, region_asm);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("region_asm_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

uint32_t mfma_group_words(const DevHap *haps, uint32_t n_haps, uint32_t hpb) {
    uint32_t mx = 0;
    for (uint32_t h0 = 0; h0 < n_haps; h0 += hpb) {
        const uint32_t hl = std::min(h0 + hpb, n_haps) - 1;
        mx = std::max(mx, haps[hl].word_off + (haps[hl].len + 15) / 16 + 3 - haps[h0].word_off);
    }
    return mx;
}

size_t scan_tmp_words(size_t n) {
    size_t w = 0;
    for (size_t nt = (n + kScanTile - 1) / kScanTile; nt > 0; nt = nt > 1 ? (nt + kScanTile - 1) / kScanTile : 0) w += nt;
    return w + 1;
}

int build_window_lists(const DevHap *haps, uint32_t n_haps, const uint32_t *druns, const uint32_t lmin[2],
                       const uint32_t span[2], uint32_t hpb, uint32_t dedup, WindowListBufs &bufs, uint64_t total[2], hipStream_t stream,
                       int (*ensure_list)(void *ctx, int c, uint64_t n, uint32_t **p, uint16_t **p16),
                       void *ensure_ctx, uint32_t share, const DevRegion *regions, const uint32_t *words,
                       const ClassTab *tab, int (*ensure_share)(void *ctx, int c, uint64_t n, uint2 **p),
                       uint64_t shared[2], uint64_t listed[2][2]) {
    if (n_haps && bufs.hd) hipLaunchKernelGGL(hd_kernel, dim3((n_haps + 255) / 256), dim3(256), 0, stream, haps, n_haps,
                                             bufs.hd, bufs.hd2);
    share = share && dedup && n_haps;
    if (share) {
        hipError_t e = hipMemsetAsync(bufs.stat, 0, 4 * sizeof(uint64_t), stream);
        if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("window lists: ") + hipGetErrorString(e));
    }
    for (int c = 0; c < 2; c++) {
        total[c] = 0;
        if (shared) shared[c] = 0;
        if (listed) listed[c][0] = listed[c][1] = 0;
        if (!lmin[c]) continue;
        const uint32_t S = span[c] ? span[c] : kMChunkCols * (c ? 4 : 2);  // the windows dirty for the longest strand
        if (share) {  // count (own windows, sharer entries per donor) -> offsets -> fill
            unsigned long long *scnt = reinterpret_cast<unsigned long long *>(bufs.soff[c]);
            hipError_t e = hipMemsetAsync(bufs.soff[c], 0, ((size_t)n_haps + 1) * 8, stream);
            if (e == hipSuccess) e = hipMemsetAsync(bufs.scur, 0, (size_t)n_haps * 8, stream);  // (the count's hstat)
            if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("window lists: ") + hipGetErrorString(e));
            hipLaunchKernelGGL(wl_share_count_kernel, dim3(n_haps / 4 + 1), dim3(256), 0, stream, haps, n_haps, regions,
                               druns, words, lmin[c], S, tab + c, bufs.off[c], scnt, bufs.scur);
            hipLaunchKernelGGL(pair_sum_kernel, dim3(256), dim3(256), 0, stream, bufs.scur, n_haps,
                               reinterpret_cast<unsigned long long *>(bufs.stat) + 2 * c);
            int rc;
            if ((rc = exclusive_scan(bufs.off[c], (uint64_t)n_haps + 1, bufs.scan_tmp, stream)) ||
                (rc = exclusive_scan(bufs.soff[c], (uint64_t)n_haps + 1, bufs.scan_tmp, stream)))
                return rc;
            uint64_t ns = 0;
            e = hipMemcpyAsync(&total[c], bufs.off[c] + n_haps, 8, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&ns, bufs.soff[c] + n_haps, 8, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(listed[c], bufs.stat + 2 * c, 16, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("window list size: ") + hipGetErrorString(e));
            shared[c] = ns;
            if ((rc = ensure_list(ensure_ctx, c, std::max<uint64_t>(total[c], 1), &bufs.list[c], &bufs.list16[c])) ||
                (rc = ensure_share(ensure_ctx, c, std::max<uint64_t>(ns, 1), &bufs.share[c])))
                return rc;
            e = hipMemsetAsync(bufs.scur, 0, (size_t)n_haps * 4, stream);
            if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("window lists: ") + hipGetErrorString(e));
            hipLaunchKernelGGL(wl_share_fill_kernel, dim3((n_haps + 3) / 4), dim3(256), 0, stream, haps, n_haps, regions,
                               druns, words, lmin[c], S, hpb, bufs.off[c], bufs.list[c], bufs.list16[c], bufs.gnarrow,
                               bufs.soff[c], bufs.scur, bufs.share[c]);
            e = hipGetLastError();
            if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("wl_share_fill_kernel: ") + hipGetErrorString(e));
            continue;
        }
        hipLaunchKernelGGL(wl_count_kernel, dim3(n_haps / 256 + 1), dim3(256), 0, stream, haps, n_haps, druns, lmin[c],
                           S, dedup, bufs.off[c]);
        if (int rc = exclusive_scan(bufs.off[c], (uint64_t)n_haps + 1, bufs.scan_tmp, stream)) return rc;
        hipError_t e = hipMemcpyAsync(&total[c], bufs.off[c] + n_haps, 8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("window list size: ") + hipGetErrorString(e));
        if (int rc = ensure_list(ensure_ctx, c, std::max<uint64_t>(total[c], 1), &bufs.list[c], &bufs.list16[c]))
            return rc;
        if (n_haps)
            hipLaunchKernelGGL(wl_fill_kernel, dim3((n_haps + 3) / 4), dim3(256), 0, stream, haps, n_haps, druns,
                               lmin[c], S, dedup, hpb, bufs.off[c], bufs.list[c], bufs.list16[c], bufs.gnarrow);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("wl_fill_kernel: ") + hipGetErrorString(e));
    }
    return TFBS_OK;
}

int group_costs(const uint64_t *off0, const uint64_t *off1, uint32_t n_haps, uint32_t hpb, uint32_t w0, uint32_t w1,
                uint32_t *cost, hipStream_t stream) {
    const uint32_t ng = (n_haps + hpb - 1) / hpb;
    if (ng == 0) return TFBS_OK;
    hipLaunchKernelGGL(group_cost_kernel, dim3((ng + 255) / 256), dim3(256), 0, stream, off0, off1, n_haps, hpb, ng, w0,
                       w1, cost);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("group_cost_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

}  // namespace tfbs
