// Exact score distributions on the device (include/tfbs_amd.h, "Thresholds from a p-value";
// DESIGN.md, "score_dist kernels").
//
// A chunk of strands lies in two ping-pong buffers of 128-bit bins (two u64, carries by
// hand).  Step j of every strand that still has one is one launch of dist_step_kernel: a
// gather, no atomics; a read outside the previous step's span counts 0 and is never made,
// so bins past a step's span are never read and nothing has to be cleared.  Step j reads
// buffer j & 1 and writes the other; a strand of n steps is left alone from launch n on and
// its counts lie in buffer n & 1.  The suffix sum (cnt -> tail, from the top) is three
// launches: per tile of kDistScanTile bins its 128-bit sum, per strand the exclusive suffix
// sums of its tiles, per tile the scan inside it; the last one stores the one bin whose
// tail is > x while the next bin's is <= x (tail is monotone: one writer, a plain store),
// or, for tail queries, the table a gather kernel then reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "hip_util.hpp"
#include "score_dist.hpp"

namespace tfbs {
namespace {

struct alignas(16) Bin { uint64_t lo, hi; };  // a 128-bit count

struct DevDist {  // one strand of a chunk
    uint64_t buf;      // its tables' first bin in either buffer; tables are `bins` apart
    uint64_t x_lo, x_hi;
    int64_t base;      // the score of bin 0
    uint32_t bins;     // the final span
    uint32_t steps;
    uint32_t width;    // 4: mono, one table; 16: dinucleotide, four
    uint32_t sh_off;   // its first shift
    uint32_t sp_off;   // its first span
    uint32_t pad;
};

__device__ __forceinline__ Bin add128(Bin a, Bin b) {
    Bin r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);
    return r;
}
__device__ __forceinline__ Bin sub128(Bin a, Bin b) {
    Bin r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
    return r;
}
__device__ __forceinline__ bool gt128(Bin a, uint64_t lo, uint64_t hi) { return a.hi > hi || (a.hi == hi && a.lo > lo); }

// The strand whose tiles hold tile `t`: the last s < n with begin[s] <= t (a strand
// without tiles shares its begin with the next one and is never found).
__device__ __forceinline__ uint32_t strand_of_tile(const uint32_t *begin, uint32_t n, uint32_t t) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (begin[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Step j of every strand of the chunk that has one.  begin: the step's tile offsets (n + 1).
__global__ __launch_bounds__(kDistStepTile) void dist_step_kernel(const DevDist *__restrict__ D,
                                                                  const uint32_t *__restrict__ begin, uint32_t n,
                                                                  const uint32_t *__restrict__ shift,
                                                                  const uint32_t *__restrict__ span, Bin *A, Bin *B,
                                                                  uint32_t j) {
    const uint32_t s = strand_of_tile(begin, n, blockIdx.x);
    const DevDist d = D[s];
    const uint32_t t = blockIdx.x - begin[s];
    const uint32_t cur = span[d.sp_off + j], prev = j ? span[d.sp_off + j - 1] : 1u;
    const uint32_t per_table = (cur + kDistStepTile - 1) / kDistStepTile;
    const uint32_t tab = t / per_table;
    const uint32_t b = (t - tab * per_table) * kDistStepTile + threadIdx.x;
    if (b >= cur) return;
    const Bin *src = ((j & 1) ? B : A) + d.buf;
    Bin *dst = ((j & 1) ? A : B) + d.buf;
    const uint32_t *sh = shift + d.sh_off + (size_t)j * d.width;
    Bin v = {0, 0};
    if (d.width == 4) {
        for (int k = 0; k < 4; k++) {
            const uint32_t o = sh[k];
            if (b >= o && b - o < prev) v = add128(v, j ? src[b - o] : Bin{1, 0});
        }
    } else {
        for (int f = 0; f < 4; f++) {  // the previous last base; tab is the new one
            const uint32_t o = sh[4 * f + tab];
            if (b >= o && b - o < prev) v = add128(v, j ? src[(size_t)f * d.bins + b - o] : Bin{1, 0});
        }
    }
    dst[(size_t)tab * d.bins + b] = v;
}

// cnt of bin b < bins from the strand's final tables.
__device__ __forceinline__ Bin dist_cnt(const DevDist &d, const Bin *fin, uint32_t b) {
    if (!d.steps) return Bin{1, 0};  // (the empty strand: one sequence, score 0, one bin)
    Bin v = fin[b];
    if (d.width == 16)
        v = add128(add128(v, fin[(size_t)d.bins + b]), add128(fin[2 * (size_t)d.bins + b], fin[3 * (size_t)d.bins + b]));
    return v;
}

// Inclusive scan over the workgroup in rank order r (0 .. 255), 128 bits wide.
__device__ __forceinline__ Bin block_scan(Bin v, Bin *lds, uint32_t r) {
    lds[r] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const Bin o = r >= off ? lds[r - off] : Bin{0, 0};
        __syncthreads();
        v = add128(v, o);
        lds[r] = v;
        __syncthreads();
    }
    return v;
}

constexpr uint32_t kPerLane = kDistScanTile / 256;  // consecutive bins of one lane

// The 128-bit sum of every scan tile.
__global__ __launch_bounds__(256) void dist_tile_sum_kernel(const DevDist *__restrict__ D,
                                                            const uint32_t *__restrict__ begin, uint32_t n,
                                                            const Bin *A, const Bin *B, Bin *tsum) {
    __shared__ Bin lds[256];
    const uint32_t s = strand_of_tile(begin, n, blockIdx.x);
    const DevDist d = D[s];
    const uint32_t t = blockIdx.x - begin[s];
    const Bin *fin = ((d.steps & 1) ? B : A) + d.buf;
    Bin v = {0, 0};
    for (uint32_t k = 0; k < kPerLane; k++) {
        const uint32_t b = t * kDistScanTile + threadIdx.x * kPerLane + k;
        if (b < d.bins) v = add128(v, dist_cnt(d, fin, b));
    }
    v = block_scan(v, lds, threadIdx.x);
    if (threadIdx.x == 255) tsum[blockIdx.x] = v;
}

// Per strand: tsum[t] becomes the sum of the tiles above t.
__global__ __launch_bounds__(256) void dist_tile_scan_kernel(const uint32_t *__restrict__ begin, Bin *tsum) {
    __shared__ Bin lds[256];
    const uint32_t t0 = begin[blockIdx.x], nt = begin[blockIdx.x + 1] - t0;
    Bin carry = {0, 0};
    for (uint32_t done = 0; done < nt; done += 256) {  // from the top tile down
        const uint32_t r = threadIdx.x;
        const bool live = done + r < nt;
        const uint32_t t = live ? nt - 1 - done - r : 0;
        const Bin own = live ? tsum[t0 + t] : Bin{0, 0};
        const Bin incl = block_scan(own, lds, r);
        if (live) tsum[t0 + t] = add128(carry, sub128(incl, own));
        carry = add128(carry, lds[255]);
        __syncthreads();
    }
}

// The scan inside every tile: the threshold's bin, and the tail table when asked for.
__global__ __launch_bounds__(256) void dist_pick_kernel(const DevDist *__restrict__ D,
                                                        const uint32_t *__restrict__ begin, uint32_t n, Bin *A, Bin *B,
                                                        const Bin *__restrict__ toff, int32_t *thr, int store_tail) {
    __shared__ Bin lds[256];
    const uint32_t s = strand_of_tile(begin, n, blockIdx.x);
    const DevDist d = D[s];
    const uint32_t t = blockIdx.x - begin[s];
    const Bin *fin = ((d.steps & 1) ? B : A) + d.buf;
    Bin *tail = ((d.steps & 1) ? A : B) + d.buf;  // the buffer the counts are not in
    const uint32_t b0 = t * kDistScanTile + threadIdx.x * kPerLane;
    Bin c[kPerLane], suf[kPerLane];
    Bin run = {0, 0};
    for (int k = (int)kPerLane - 1; k >= 0; k--) {
        c[k] = b0 + k < d.bins ? dist_cnt(d, fin, b0 + k) : Bin{0, 0};
        run = add128(run, c[k]);
        suf[k] = run;
    }
    const uint32_t r = 255 - threadIdx.x;  // the lanes above come first
    const Bin incl = block_scan(run, lds, r);
    const Bin above = add128(toff[blockIdx.x], sub128(incl, run));
    for (uint32_t k = 0; k < kPerLane; k++) {
        const uint32_t b = b0 + k;
        if (b >= d.bins) break;
        const Bin tl = add128(above, suf[k]);
        if (store_tail) tail[b] = tl;
        else if (gt128(tl, d.x_lo, d.x_hi) && !gt128(sub128(tl, c[k]), d.x_lo, d.x_hi)) thr[s] = (int32_t)(d.base + b);
    }
}

// tail(score) of one strand from its stored table.
__global__ __launch_bounds__(256) void dist_gather_kernel(const DevDist *__restrict__ D, const Bin *A, const Bin *B,
                                                          const int32_t *__restrict__ scores, uint32_t n, uint64_t *lo,
                                                          uint64_t *hi) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const DevDist d = D[0];
    const Bin *tail = ((d.steps & 1) ? A : B) + d.buf;
    const int64_t b = (int64_t)scores[k] - d.base;
    Bin v = {0, 0};
    if (b < (int64_t)d.bins) v = tail[b <= 0 ? 0 : b];
    lo[k] = v.lo;
    hi[k] = v.hi;
}

// floor(p 4^L), 0 <= p < 1: the 53-bit mantissa shifted inside two u64.
void pvalue_x(double p, uint32_t L, uint64_t *lo, uint64_t *hi) {
    *lo = *hi = 0;
    if (p == 0.0) return;
    int e;
    const double f = std::frexp(p, &e);
    const uint64_t m = (uint64_t)std::ldexp(f, 53);
    const int sh = e - 53 + 2 * (int)L;  // at most 126 - 53
    if (sh >= 64) *hi = m << (sh - 64);
    else if (sh > 0) {
        *lo = m << sh;
        *hi = m >> (64 - sh);
    } else if (sh > -64) *lo = m >> -sh;
}

struct DistDev {  // one call's device state; released in reverse: the buffers, the stream, then the device restored
    struct Restore {
        int device = -1;  // the device current before the call
        ~Restore() {
            if (device >= 0) (void)hipSetDevice(device);
        }
    } prev;
    Stream stream;
    DevBuf<Bin> A, B;  // the ping-pong buffers, sized for the call's largest chunk
    int buffers(uint64_t bins) {
        const int rc = A.ensure_exact(std::max<uint64_t>(bins, 1));
        return rc ? rc : B.ensure_exact(std::max<uint64_t>(bins, 1));
    }
};

template <typename T>
int upload(DistDev &M, const std::vector<T> &v, DevBuf<T> &out) {
    if (int rc = out.ensure_exact(std::max<size_t>(v.size(), 1))) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(out.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, M.stream));
    return TFBS_OK;
}

int open_device(DistDev &M, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return fail(TFBS_E_NODEVICE, "no HIP device");
    }
    if (device >= n) return fail(TFBS_E_ARG, "no HIP device " + std::to_string(device));
    int prev = -1;
    (void)hipGetDevice(&prev);
    HIP_TRY(hipSetDevice(device));
    M.prev.device = prev;
    HIP_TRY(M.stream.create());
    return TFBS_OK;
}

uint64_t strand_bins(const DistStrand &s) { return (uint64_t)s.tables() * s.bins; }
uint64_t strand_bytes(const DistStrand &s) { return 2 * strand_bins(s) * sizeof(Bin); }

// The distributions of strands [first, last) of S: their thresholds into thr (by pattern
// index), or, store_tail (one strand), tail(scores) into lo / hi.
int run_chunk(DistDev &M, const std::vector<DistStrand> &S, size_t first, size_t last, double p, int32_t *thr,
              const int32_t *scores, size_t n_scores, uint64_t *lo, uint64_t *hi) {
    const uint32_t n = (uint32_t)(last - first);
    const bool store_tail = scores != nullptr;
    std::vector<DevDist> D(n);
    std::vector<uint32_t> shift, span, scan_begin(n + 1, 0);
    uint64_t bins = 0;
    uint32_t max_steps = 0;
    for (uint32_t k = 0; k < n; k++) {
        const DistStrand &s = S[first + k];
        DevDist &d = D[k];
        d = DevDist{};
        d.buf = bins;
        pvalue_x(p, s.L, &d.x_lo, &d.x_hi);
        d.base = s.base;
        d.bins = (uint32_t)s.bins;
        d.steps = s.steps;
        d.width = s.width;
        d.sh_off = (uint32_t)shift.size();
        d.sp_off = (uint32_t)span.size();
        shift.insert(shift.end(), s.shift.begin(), s.shift.end());
        span.insert(span.end(), s.span.begin(), s.span.end());
        bins += (uint64_t)s.tables() * s.bins;
        max_steps = std::max(max_steps, s.steps);
        scan_begin[k + 1] = scan_begin[k] + (uint32_t)((s.bins + kDistScanTile - 1) / kDistScanTile);
    }
    // per step the tile offsets of the strands that take it
    std::vector<uint32_t> step_begin((size_t)max_steps * (n + 1), 0);
    for (uint32_t j = 0; j < max_steps; j++) {
        uint32_t *row = &step_begin[(size_t)j * (n + 1)];
        for (uint32_t k = 0; k < n; k++) {
            const DistStrand &s = S[first + k];
            const uint32_t tiles = j < s.steps ? s.tables() * ((s.span[j] + kDistStepTile - 1) / kDistStepTile) : 0;
            row[k + 1] = row[k] + tiles;
        }
    }
    DevBuf<DevDist> dD;  // the chunk's own, freed on return
    DevBuf<uint32_t> d_shift, d_span, d_step_begin, d_scan_begin;
    DevBuf<Bin> tsum;
    DevBuf<int32_t> d_thr;
    Bin *const A = M.A.p, *const B = M.B.p;
    int rc;
    if ((rc = upload(M, D, dD)) || (rc = upload(M, shift, d_shift)) || (rc = upload(M, span, d_span)) ||
        (rc = upload(M, step_begin, d_step_begin)) || (rc = upload(M, scan_begin, d_scan_begin)) ||
        (rc = tsum.ensure_exact(std::max<uint32_t>(scan_begin[n], 1))) || (rc = d_thr.ensure_exact(std::max<uint32_t>(n, 1))))
        return rc;
    for (uint32_t j = 0; j < max_steps; j++) {
        const uint32_t *row = d_step_begin.p + (size_t)j * (n + 1);
        const uint32_t tiles = step_begin[(size_t)j * (n + 1) + n];
        hipLaunchKernelGGL(dist_step_kernel, dim3(tiles), dim3(kDistStepTile), 0, M.stream, dD.p, row, n, d_shift.p, d_span.p,
                           A, B, j);
    }
    const uint32_t st = scan_begin[n];
    hipLaunchKernelGGL(dist_tile_sum_kernel, dim3(st), dim3(256), 0, M.stream, dD.p, d_scan_begin.p, n, A, B, tsum.p);
    hipLaunchKernelGGL(dist_tile_scan_kernel, dim3(n), dim3(256), 0, M.stream, d_scan_begin.p, tsum.p);
    hipLaunchKernelGGL(dist_pick_kernel, dim3(st), dim3(256), 0, M.stream, dD.p, d_scan_begin.p, n, A, B, tsum.p, d_thr.p,
                       store_tail ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (!store_tail) {
        std::vector<int32_t> h(n);
        HIP_TRY(hipMemcpyAsync(h.data(), d_thr.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, M.stream));
        HIP_TRY(hipStreamSynchronize(M.stream));
        for (uint32_t k = 0; k < n; k++) thr[S[first + k].index] = h[k];
    } else {
        DevBuf<int32_t> d_scores;
        DevBuf<uint64_t> d_lo, d_hi;
        const size_t ns = std::max<size_t>(n_scores, 1);
        if ((rc = d_scores.ensure_exact(ns)) || (rc = d_lo.ensure_exact(ns)) || (rc = d_hi.ensure_exact(ns))) return rc;
        HIP_TRY(hipMemcpyAsync(d_scores.p, scores, n_scores * sizeof(int32_t), hipMemcpyHostToDevice, M.stream));
        hipLaunchKernelGGL(dist_gather_kernel, dim3((uint32_t)((n_scores + 255) / 256)), dim3(256), 0, M.stream, dD.p, A, B,
                           d_scores.p, (uint32_t)n_scores, d_lo.p, d_hi.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(lo, d_lo.p, n_scores * sizeof(uint64_t), hipMemcpyDeviceToHost, M.stream));
        HIP_TRY(hipMemcpyAsync(hi, d_hi.p, n_scores * sizeof(uint64_t), hipMemcpyDeviceToHost, M.stream));
        HIP_TRY(hipStreamSynchronize(M.stream));
    }
    return TFBS_OK;
}

}  // namespace

int dev_pvalue_thresholds(const std::vector<DistStrand> &S, int device, double p, int32_t *min_scores) {
    DistDev M;
    if (int rc = open_device(M, device)) return rc;
    const uint64_t budget = scratch_budget("TFBS_PVALUE_SCRATCH_MB", 256.0);
    std::vector<size_t> ends;  // chunks of whole strands, at least one
    uint64_t most = 0;
    for (size_t first = 0; first < S.size();) {
        size_t last = first + 1;
        uint64_t bytes = strand_bytes(S[first]);
        while (last < S.size() && last - first < 32768 && bytes + strand_bytes(S[last]) <= budget)
            bytes += strand_bytes(S[last++]);
        most = std::max(most, bytes);
        ends.push_back(last);
        first = last;
    }
    if (int rc = M.buffers(most / (2 * sizeof(Bin)))) return rc;
    size_t first = 0;
    for (size_t last : ends) {
        if (int rc = run_chunk(M, S, first, last, p, min_scores, nullptr, 0, nullptr, nullptr)) return rc;
        first = last;
    }
    return TFBS_OK;
}

int dev_score_tails(const DistStrand &S, int device, const int32_t *scores, size_t n, uint64_t *lo, uint64_t *hi) {
    if (n > UINT32_MAX) return fail(TFBS_E_ARG, "more than 2^32 - 1 scores in one call");
    DistDev M;
    if (int rc = open_device(M, device)) return rc;
    const std::vector<DistStrand> one{S};
    if (int rc = M.buffers(strand_bins(S))) return rc;
    return run_chunk(M, one, 0, 1, 0.0, nullptr, scores, n, lo, hi);
}

}  // namespace tfbs
