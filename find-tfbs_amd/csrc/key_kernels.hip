// Per-region key assembly on the device.
//
// count_matches_by_sample (main.rs:500-534) builds, per key (bed, inner range,
// pattern_id), the per-sample L/R vectors; counts_as_genotypes (main.rs:439-498)
// emits a row only when the per-sample totals differ.  Every sample's total is
// a sum of two distinct haplotypes' counts, so a key can only produce a row if
// its counts over the region's distinct haplotypes are not constant.
//
// The matrix-core scan leaves no count matrix: per hit one (haplotype, key =
// slot * n_inner + range) pair in its workgroup's hit list (or the spill list),
// plus the region's reference hits (strand, window) that every HAP_DEDUP
// haplotype inherits in the window tiles it did not scan.  key_asm_kernel (one
// workgroup per region) counts them into a [key][distinct haplotype] block in
// LDS, a chunk of keys at a time -- the LUT/generic kernels' slots are copied
// from their dense counts -- and then either classifies every key (any count
// != 0 -> the key exists in the reference's HashMap; counts differ -> it may
// emit a row) and appends the varying keys' counts to a compact list (the run
// flow's reduction), or stores the block into the dense matrix (the debug
// download).
#include <hip/hip_runtime.h>

#include <mutex>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "keys.hpp"

namespace tfbs {
namespace {

constexpr int kAsmBlock = 256;
constexpr uint32_t kAsmWaves = kAsmBlock / 64;
constexpr uint32_t kAsmCounters = 6144;  // u32 counters of the LDS block (24 KiB)
constexpr uint32_t kAsmHaps = 1024;      // haplotypes whose diff runs sit in LDS (else read from L2)

constexpr uint32_t kAsmRuns = 2048;      // diff runs staged in LDS
constexpr uint32_t kAsmHits = 2048;      // own hits staged in LDS (else re-read from the lists per pass)
constexpr uint32_t kAsmRefs = 256;       // reference hits staged in LDS (else re-read)
constexpr uint32_t kAsmKeyWords = 2048;  // touched-key bitmap: keys handled per key window
constexpr uint32_t kAsmKeyWin = 32 * kAsmKeyWords;

// Region r's spill records (bucketed: spill_cnt[r] of them at spill_off[r] of spill_sorted;
// spill_off[r] means nothing where there is none).
// In place (AsmArgs::spill_inplace): every record the assembly reads, [0, n) of the scan's own
// list spill_raw, in no order; the reader keeps those of its region (spill_mine).
__device__ __forceinline__ uint2 spill_range(const AsmArgs &A, uint32_t r) {
    if (!A.spill_count || !*A.spill_count) return make_uint2(0, 0);
    if (A.spill_inplace) return make_uint2(0, min(*A.spill_count, min(A.spill_inplace, A.spill_cap)));
    const uint32_t c = A.spill_cnt[r];
    if (c == 0) return make_uint2(0, 0);
    const uint32_t o = A.spill_off[r];
    return make_uint2(o, o + c);
}
__device__ __forceinline__ const uint32_t *spill_list(const AsmArgs &A) {
    return A.spill_inplace ? A.spill_raw : A.spill_sorted;
}
// A record's first word: region | kind << 31.  (A bucket holds its region's records alone.)
__device__ __forceinline__ bool spill_mine(const AsmArgs &A, uint32_t w, uint32_t r) {
    return !A.spill_inplace || (w & 0x7FFFFFFFu) == r;
}

// The inner ranges [k0, k0 + nk) a reference hit (window i of a strand of length L)
// overlaps (range.rs:18-21 as main.rs:503 uses it; the reference's positions are
// affine): bit k - k0.
__device__ __forceinline__ uint32_t ref_overlaps(const AsmArgs &A, const DevRegion &rg, uint32_t L, uint32_t i,
                                                 uint32_t k0, uint32_t nk) {
    const int32_t *inner = A.inner + 2 * (size_t)rg.inner_off;
    uint32_t mask = 0;
    for (uint32_t k = k0; k < k0 + nk; k++) {
        const int32_t s = inner[2 * k], en = inner[2 * k + 1];
        const uint32_t span = (uint32_t)(en - s);
        if ((uint32_t)((int32_t)i - s) <= span || (uint32_t)((int32_t)(i + L) - 1 - s) <= span) mask |= 1u << (k - k0);
    }
    return mask;
}

// A reference hit (strand g, window i) as the assembly uses it: {first key
// (slot * n_inner), window, L | (K depth - 1) << 16, inner ranges < 32 it overlaps}.
__device__ __forceinline__ uint4 make_ref(const AsmArgs &A, const DevRegion &rg, uint32_t g, uint32_t i) {
    const int32_t *meta = A.mmeta + (size_t)(g >> 6) * kGMetaInts;
    const uint32_t sn = g & 63u, L = (uint32_t)meta[kGStrandInts * sn + kGLen];
    const uint32_t dk = (uint32_t)meta[kGDepth] - 1;
    const uint32_t key0 = (uint32_t)meta[kGStrandInts * sn + kGSlot] * rg.n_inner;
    return make_uint4(key0, i, L | (dk << 16), ref_overlaps(A, rg, L, i, 0, min(rg.n_inner, 32u)));
}

// make_ref from the three meta fields already loaded (key_fast_kernel loads them a round early).
__device__ __forceinline__ uint4 make_ref_loaded(const AsmArgs &A, const DevRegion &rg, uint32_t L, uint32_t depth,
                                                 uint32_t slot, uint32_t i) {
    return make_uint4(slot * rg.n_inner, i, L | ((depth - 1) << 16), ref_overlaps(A, rg, L, i, 0, min(rg.n_inner, 32u)));
}

// Every own hit (local haplotype l < U, key) of region r: the wave lists of the
// region's haplotype groups (group g's are lists g * kMBlockWaves .. + 7, scan.hpp; one
// wave per list), then the region's spill records.
template <class F>
__device__ __forceinline__ void visit_hits(const AsmArgs &A, uint32_t r, uint32_t hb, uint32_t U, F &&f) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t g_lo = hb / A.hpb, g_hi = (hb + U - 1) / A.hpb;
    if (A.mfma)
        for (uint32_t li = g_lo * kMBlockWaves + wave; li < (g_hi + 1) * kMBlockWaves; li += kAsmWaves) {
            const uint32_t n = A.hitn[li];
            const uint2 *lst = reinterpret_cast<const uint2 *>(A.hitl) + (size_t)(li / kMBlockWaves) * A.cand_cap +
                               (size_t)(li % kMBlockWaves) * (A.cand_cap / kMBlockWaves);
            for (uint32_t e = lane; e < n; e += 64) {
                const uint2 h = lst[e];
                if (h.x - hb < U) f(h.x - hb, h.y);
            }
        }
    const uint2 sp = spill_range(A, r);
    for (uint32_t e = sp.x + threadIdx.x; e < sp.y; e += kAsmBlock) {
        const uint32_t *q = spill_list(A) + 3 * (size_t)e;
        if (!(q[0] >> 31) && spill_mine(A, q[0], r) && q[1] - hb < U) f(q[1] - hb, q[2]);
    }
}

// Every reference hit of region r (its list, then its spill records).
template <class F>
__device__ __forceinline__ void visit_refs(const AsmArgs &A, uint32_t r, const DevRegion &rg, F &&f) {
    const uint32_t nl = min(A.ref_count[r], kRefPerRegion);
    for (uint32_t t = threadIdx.x; t < nl; t += kAsmBlock)
        f(make_ref(A, rg, A.ref_hits[2 * ((size_t)r * kRefPerRegion + t)],
                   A.ref_hits[2 * ((size_t)r * kRefPerRegion + t) + 1]));
    const uint2 sp = spill_range(A, r);
    for (uint32_t e = sp.x + threadIdx.x; e < sp.y; e += kAsmBlock) {
        const uint32_t *q = spill_list(A) + 3 * (size_t)e;
        if ((q[0] >> 31) && spill_mine(A, q[0], r)) f(make_ref(A, rg, q[1], q[2]));
    }
}

// One region per iteration: every region (list == nullptr, grid = regions) or the
// *list_n regions at list over a fixed grid.
__global__ __launch_bounds__(kAsmBlock) void key_asm_kernel(AsmArgs A, const uint32_t *list, const uint32_t *list_n) {
    __shared__ uint32_t s_cnt[kAsmCounters];
    __shared__ uint32_t s_rh[kAsmHaps];    // per haplotype: first staged run | runs << 16 (0xFFFFFFFF: not HAP_DEDUP)
    __shared__ uint2 s_run[kAsmRuns];      // the region's diff runs
    __shared__ uint2 s_hit[kAsmHits];      // (local haplotype, key)
    __shared__ uint4 s_ref[kAsmRefs];      // make_ref
    __shared__ uint32_t s_bits[kAsmKeyWords], s_rbase[kAsmKeyWords];  // touched keys of the window, rows before each word
    __shared__ uint32_t s_scan[kAsmBlock];
    __shared__ uint32_t s_nhit, s_nref, s_nvar, s_nput;
    __shared__ unsigned long long s_vbase, s_obase;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (list && A.report && blockIdx.x == 0 && tid < 2) A.report[tid] = A.report_src ? A.report_src[tid] : 0u;
    const uint32_t n_it = list ? *list_n : gridDim.x;
    for (uint32_t it = blockIdx.x; it < n_it; it += gridDim.x) {
    const uint32_t r = list ? list[it] : it;
    __syncthreads();  // the previous region's LDS readers are done
    [&]() {
    const DevRegion rg = A.regions[r];
    const uint32_t U = rg.hap_count, n_inner = rg.n_inner;
    const uint32_t K = A.n_slots * n_inner;
    const uint64_t ko = (uint64_t)rg.inner_off * A.n_slots;
    // tfbs_ctx_assembly_trace: this kernel's bits (the list pass keeps key_fast_kernel's)
    auto trace = [&](uint32_t pw) {
        if (A.path && tid == 0) A.path[r] = (list ? A.path[r] : 0u) | TFBS_PATH_ASM | pw;
    };
    if (U == 0 || K == 0) {  // no samples: no haplotype, no match, no key
        trace(0);
        if (A.mode == 0)
            for (uint32_t j = tid; j < K; j += kAsmBlock) {
                A.key_first[ko + j] = 0;
                A.key_flags[ko + j] = 0;
            }
        return;
    }
    const uint32_t hb = rg.hap_begin;
    // the diff runs of the region's HAP_DEDUP haplotypes (consecutive in the batch's
    // run array) in LDS when they fit
    uint32_t run0 = 0, run1 = 0;
    for (uint32_t l = 0; l < U; l++)  // uniform: the first and last HAP_DEDUP haplotype's runs
        if (A.haps[hb + l].flags & HAP_DEDUP) {
            run0 = A.haps[hb + l].rrun_off;
            break;
        }
    for (uint32_t l = U; l-- > 0;)
        if (A.haps[hb + l].flags & HAP_DEDUP) {
            run1 = A.haps[hb + l].rrun_off + A.haps[hb + l].n_rruns;
            break;
        }
    const bool lds_haps = U <= kAsmHaps && run1 - run0 <= kAsmRuns;
    if (lds_haps) {
        for (uint32_t l = tid; l < U; l += kAsmBlock) {
            const DevHap h = A.haps[hb + l];
            s_rh[l] = (h.flags & HAP_DEDUP) ? (h.rrun_off - run0) | (h.n_rruns << 16) : 0xFFFFFFFFu;
        }
        for (uint32_t k = tid; k < run1 - run0; k += kAsmBlock)
            s_run[k] = make_uint2(A.druns[2 * (run0 + k)], A.druns[2 * (run0 + k) + 1]);
    }
    const bool refs_on = A.mfma && rg.ref_hap != UINT32_MAX;
    // stage the region's own hits and reference hits in LDS (the lists are read once)
    if (tid == 0) s_nhit = s_nref = 0;
    __syncthreads();
    if (A.mfma) {
        visit_hits(A, r, hb, U, [&](uint32_t l, uint32_t key) {
            const uint32_t at = atomicAdd(&s_nhit, 1u);
            if (at < kAsmHits) s_hit[at] = make_uint2(l, key);
        });
        if (refs_on)
            visit_refs(A, r, rg, [&](const uint4 &q) {
                const uint32_t at = atomicAdd(&s_nref, 1u);
                if (at < kAsmRefs) s_ref[at] = q;
            });
    }
    __syncthreads();
    const uint32_t nhit = s_nhit, nref = s_nref;
    const bool hits_lds = nhit <= kAsmHits, refs_lds = nref <= kAsmRefs;
    trace((U > kAsmHaps ? TFBS_PATH_ASM_HAPS : 0u) | (run1 - run0 > kAsmRuns ? TFBS_PATH_ASM_RUNS : 0u) |
          (hits_lds ? 0u : TFBS_PATH_ASM_HITS) | (refs_lds ? 0u : TFBS_PATH_ASM_REFS) |
          (U > kAsmCounters ? TFBS_PATH_ASM_SCRATCH : 0u));
    auto each_hit = [&](auto &&f) {
        if (!A.mfma) return;
        if (hits_lds) {
            for (uint32_t e = tid; e < nhit; e += kAsmBlock) f(s_hit[e].x, s_hit[e].y);
        } else {
            visit_hits(A, r, hb, U, f);
        }
    };
    auto each_ref = [&](auto &&f) {  // thread-parallel over the reference hits
        if (!refs_on) return;
        if (refs_lds) {
            for (uint32_t t = tid; t < nref; t += kAsmBlock) f(s_ref[t]);
        } else {
            visit_refs(A, r, rg, f);
        }
    };
    // the keys a reference hit adds to: its ranges past 32 recomputed, the others in q.w
    auto ref_keys = [&](const uint4 &q, auto &&f) {
        const uint32_t L = q.z & 0xFFFFu;
        for (uint32_t kb = 0; kb < n_inner; kb += 32)
            for (uint32_t m = kb ? ref_overlaps(A, rg, L, q.y, kb, min(32u, n_inner - kb)) : q.w; m; m &= m - 1)
                f(q.x + kb + __builtin_ctz(m));
    };
    const uint64_t dense_base = A.dense_base ? A.haps[hb].count_off : 0;
    const bool lds_cnt = U <= kAsmCounters;
    const uint32_t rows_per = lds_cnt ? kAsmCounters / U : 1;
    uint32_t *cnt = lds_cnt ? s_cnt : A.scratch + rg.big_off;
    for (uint32_t kw0 = 0; kw0 < K; kw0 += kAsmKeyWin) {  // key windows (one unless 65536 keys)
        const uint32_t kwn = min(kAsmKeyWin, K - kw0), nw = (kwn + 31) / 32;
        __syncthreads();
        for (uint32_t w = tid; w < nw; w += kAsmBlock) s_bits[w] = 0;
        __syncthreads();
        // touched keys: own hits, reference hits, every key of a LUT/generic slot
        each_hit([&](uint32_t, uint32_t key) {
            const uint32_t j = key - kw0;
            if (j < kwn) atomicOr(&s_bits[j >> 5], 1u << (j & 31));
        });
        each_ref([&](const uint4 &q) {
            ref_keys(q, [&](uint32_t key) {
                const uint32_t j = key - kw0;
                if (j < kwn) atomicOr(&s_bits[j >> 5], 1u << (j & 31));
            });
        });
        if (A.any_dense)
            for (uint32_t j = tid; j < kwn; j += kAsmBlock)
                if (!A.slot_mfma[(kw0 + j) / n_inner]) atomicOr(&s_bits[j >> 5], 1u << (j & 31));
        __syncthreads();
        // rows: touched keys in key order (block scan of the words' popcounts)
        constexpr uint32_t per = kAsmKeyWords / kAsmBlock;
        uint32_t mine = 0;
        for (uint32_t q = 0; q < per; q++) {
            const uint32_t w = tid * per + q;
            if (w < nw) mine += __popc(s_bits[w]);
        }
        s_scan[tid] = mine;
        __syncthreads();
        for (uint32_t o = 1; o < kAsmBlock; o <<= 1) {
            const uint32_t t = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += t;
            __syncthreads();
        }
        {
            uint32_t run = s_scan[tid] - mine;
            for (uint32_t q = 0; q < per; q++) {
                const uint32_t w = tid * per + q;
                if (w < nw) {
                    s_rbase[w] = run;
                    run += __popc(s_bits[w]);
                }
            }
        }
        const uint32_t T = s_scan[kAsmBlock - 1];
        __syncthreads();
        auto row_of = [&](uint32_t j) { return s_rbase[j >> 5] + __popc(s_bits[j >> 5] & ((1u << (j & 31)) - 1u)); };
        auto key_of_row = [&](uint32_t t) {  // the word whose rows start at or before t, then its bit
            uint32_t lo = 0, hi = nw - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) / 2;
                if (s_rbase[mid] <= t) lo = mid;
                else hi = mid - 1;
            }
            uint32_t b = s_bits[lo];
            for (uint32_t k = t - s_rbase[lo]; k; k--) b &= b - 1;
            return 32 * lo + __builtin_ctz(b);
        };
        // untouched keys: no match -- no key in the reference's HashMap (zeros in the dense matrix)
        for (uint32_t j = tid; j < kwn; j += kAsmBlock) {
            if ((s_bits[j >> 5] >> (j & 31)) & 1u) continue;
            if (A.mode == 0) {
                A.key_first[ko + kw0 + j] = 0;
                A.key_flags[ko + kw0 + j] = 0;
            } else {
                for (uint32_t l = 0; l < U; l++) A.counts[dense_base + (uint64_t)(kw0 + j) * rg.count_stride + l] = 0;
            }
        }
        for (uint32_t t0 = 0; t0 < T; t0 += rows_per) {
            const uint32_t nrow = min(rows_per, T - t0);
            __syncthreads();  // the previous chunk's readers are done
            for (uint32_t rr = wave; rr < nrow; rr += kAsmWaves) {  // a LUT/generic key: its dense counts
                const uint32_t j = kw0 + key_of_row(t0 + rr);
                const bool dense = A.any_dense && !A.slot_mfma[j / n_inner];
                for (uint32_t l = lane; l < U; l += 64)
                    cnt[rr * U + l] = dense ? A.counts[dense_base + (uint64_t)j * rg.count_stride + l] : 0u;
            }
            __syncthreads();
            each_hit([&](uint32_t l, uint32_t key) {
                const uint32_t j = key - kw0;
                if (j >= kwn) return;
                const uint32_t t = row_of(j) - t0;
                if (t < nrow) atomicAdd(&cnt[t * U + l], 1u);
            });
            // reference hits: +1 to every HAP_DEDUP haplotype for which the hit's
            // window is not dirty (in the reference's columns: the haplotype has the
            // window's bases from its start position on, the scan lists no hit there;
            // tfbs_internal.hpp run_meets, span L)
            auto dirty = [&](uint32_t l, uint32_t L, uint32_t w) {
                const uint32_t S = L;
                if (lds_haps) {
                    const uint32_t x = s_rh[l];
                    if (x == 0xFFFFFFFFu) return true;
                    for (uint32_t k = x & 0xFFFFu, e = k + (x >> 16); k < e; k++)
                        if (run_meets(s_run[k].x, s_run[k].y, w, S)) return true;
                    return false;
                }
                const DevHap &h = A.haps[hb + l];
                if (!(h.flags & HAP_DEDUP)) return true;
                for (uint32_t k = h.rrun_off; k < h.rrun_off + h.n_rruns; k++)
                    if (run_meets(A.druns[2 * k], A.druns[2 * k + 1], w, S)) return true;
                return false;
            };
            if (refs_on && refs_lds && U <= 32 * kAsmBlock) {
                for (uint32_t q0 = 0; q0 < nref; q0++) {  // workgroup-uniform; threads over the haplotypes
                    const uint4 q = s_ref[q0];
                    const uint32_t L = q.z & 0xFFFFu;
                    bool here = false;  // uniform: a key of the hit is in this chunk
                    ref_keys(q, [&](uint32_t key) {
                        here = here || (key - kw0 < kwn && row_of(key - kw0) - t0 < nrow);
                    });
                    if (!here) continue;
                    uint32_t keep = 0;  // bit j: haplotype tid + j kAsmBlock inherits the hit
                    for (uint32_t l = tid, j = 0; l < U; l += kAsmBlock, j++)
                        if (!dirty(l, L, q.y)) keep |= 1u << j;
                    ref_keys(q, [&](uint32_t key) {
                        const uint32_t t = key - kw0 < kwn ? row_of(key - kw0) - t0 : UINT32_MAX;
                        if (t >= nrow) return;
                        for (uint32_t m = keep; m; m &= m - 1)
                            atomicAdd(&cnt[t * U + tid + kAsmBlock * __builtin_ctz(m)], 1u);
                    });
                }
            } else if (refs_on) {  // too many for LDS (rare): each thread walks its hits' haplotypes
                visit_refs(A, r, rg, [&](const uint4 &q) {
                    const uint32_t L = q.z & 0xFFFFu;
                    ref_keys(q, [&](uint32_t key) {
                        const uint32_t t = key - kw0 < kwn ? row_of(key - kw0) - t0 : UINT32_MAX;
                        if (t >= nrow) return;
                        for (uint32_t l = 0; l < U; l++)
                            if (!dirty(l, L, q.y)) atomicAdd(&cnt[t * U + l], 1u);
                    });
                });
            }
            __syncthreads();
            if (A.mode == 1) {  // dense: the matrix-core slots' counts into the count matrix
                for (uint32_t rr = wave; rr < nrow; rr += kAsmWaves) {
                    const uint32_t j = kw0 + key_of_row(t0 + rr);
                    if (!A.slot_mfma[j / n_inner]) continue;
                    for (uint32_t l = lane; l < U; l += 64)
                        A.counts[dense_base + (uint64_t)j * rg.count_stride + l] = cnt[rr * U + l];
                }
                continue;
            }
            // classify: one wave per row
            if (tid == 0) s_nvar = 0;
            __syncthreads();
            for (uint32_t rr = wave; rr < nrow; rr += kAsmWaves) {
                const uint32_t j = kw0 + key_of_row(t0 + rr);
                const uint32_t *col = cnt + rr * U;
                const uint32_t c0 = col[0];
                uint32_t any = 0, diff = 0;
                for (uint32_t l = lane; l < U; l += 64) {
                    const uint32_t c = col[l];
                    any |= c;
                    diff |= c ^ c0;
                }
                const bool a = __ballot(any != 0) != 0, v = __ballot(diff != 0) != 0;
                if (lane == 0) {
                    A.key_first[ko + j] = c0;
                    A.key_flags[ko + j] = (uint8_t)((a ? KEY_ANY : 0) | (v ? KEY_VARIES : 0));
                    if (v) atomicAdd(&s_nvar, 1u);
                }
            }
            __syncthreads();
            const uint32_t nvar = s_nvar;  // (reset only after the next chunk's first barrier)
            if (nvar == 0) continue;
            if (tid == 0) {  // the chunk's share of the compact lists
                s_vbase = atomicAdd(A.var_tot, (unsigned long long)nvar);
                s_obase = atomicAdd(A.var_tot + 1, (unsigned long long)nvar * U);
                s_nput = 0;
            }
            __syncthreads();
            for (uint32_t rr = wave; rr < nrow; rr += kAsmWaves) {
                const uint32_t *col = cnt + rr * U;
                const uint32_t c0 = col[0];
                uint32_t diff = 0;
                for (uint32_t l = lane; l < U; l += 64) diff |= col[l] ^ c0;
                if (__ballot(diff != 0) == 0) continue;
                const uint32_t j = kw0 + key_of_row(t0 + rr);
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(&s_nput, 1u);
                at = __shfl(at, 0);
                const uint64_t vi = s_vbase + at;
                const uint64_t off = s_obase + (uint64_t)at * U;
                if (vi < A.var_keys_cap && off + U <= A.var_cap) {
                    if (lane == 0) A.var_keys[vi] = DevVarKey{r, j, off};
                    for (uint32_t l = lane; l < U; l += 64) A.var_counts[off + l] = col[l];
                }
            }
        }
    }
    }();
    }
}

// ---------------------------------------------------------------------------
// key_fast_kernel: the reduction (mode 0) of one region per workgroup with
// every list in LDS.  A distinct haplotype l's count on key j is
//     own(l, j) + [HAP_DEDUP l] * (R(j) - D(l, j))
// (own: its hits, all in windows the scan read; R: the reference hits on j;
// D: those whose window is dirty for l -- the scan read that window of l, so
// its own hits already cover it).  So the region's work is its own hits plus,
// per HAP_DEDUP haplotype, the reference hits inside its few dirty windows
// (found by walking its diff runs over the reference hits sorted by window):
// one "correction" list of (key, l, +1 | -1) entries (in LDS, or for a region
// with many haplotypes a share of a launch-wide arena in global memory), then
// per chunk of touched keys a [key][haplotype] block in LDS that starts at the
// base (R(j) or 0, or the dense count of a LUT/generic slot) and takes the
// corrections with LDS atomics.  A region past the kernel's limits (haplotypes,
// keys, hit lists, reference hits, diff runs, arena) is appended to A.redo and
// left to key_asm_kernel.
#ifndef TFBS_KF_BLOCK
#define TFBS_KF_BLOCK 256
#endif
constexpr uint32_t kFMaxU = 2048;     // distinct haplotypes (11 bits of a correction)
constexpr uint32_t kFKeyWords = 512;  // touched-key bitmap: keys <= 16384
constexpr uint32_t kFBatch = 8;       // hit-list entries each thread has in flight
constexpr uint32_t kFNone = 0xFFFFFFFFu;
// Two shapes of the kernel: the common one (TFBS_KF_BLOCK threads, ~40 KB of LDS,
// four regions per CU) and one for regions of many distinct haplotypes (1 024
// threads and ~154 KB of LDS: a whole CU, counter chunks of 24 Ki u32 -- 17 rows of
// 1 400 haplotypes instead of 2, which sent such a region's counters to the
// global arena).  HAP_LDS: haplotypes whose reuse descriptor sits in LDS (the
// others: read again); COR: corrections in LDS; REFS: reference hits; CNT: u32
// counters of a chunk (rows x U); ROWS: rows (touched keys) per chunk; LISTS: scan
// hit lists staged at a time.
template <int BLOCK, uint32_t HAP_LDS, uint32_t COR, uint32_t REFS, uint32_t CNT, uint32_t ROWS, uint32_t LISTS>
struct KfShape {
    static constexpr int kBlock = BLOCK;
    static constexpr uint32_t kWaves = BLOCK / 64, kHapLds = HAP_LDS, kCor = COR, kRefs = REFS, kCnt = CNT,
                              kRuns = CNT / 2, kRows = ROWS, kLists = LISTS;
    static_assert(kFMaxU % BLOCK == 0 && HAP_LDS % BLOCK == 0 && LISTS <= BLOCK && REFS <= BLOCK,
                  "key_fast_kernel's per-thread shares");
};
constexpr int kFB = TFBS_KF_BLOCK;
#ifdef TFBS_KF_LDS3  // (A/B: the round-4 start's ~51 KB shape, three regions per CU)
using KfSmall = KfShape<kFB, 4 * kFB, 16 * kFB, kFB, 16 * kFB, 2 * kFB, kFB>;
#elif defined(TFBS_KF_LDS6)  // (A/B: ~26 KB, six regions per CU)
using KfSmall = KfShape<kFB, 2 * kFB, 7 * kFB, kFB, 6 * kFB, kFB, kFB / 2>;
#elif defined(TFBS_KF_LDS8)  // (A/B: ~19 KB, eight regions per CU)
using KfSmall = KfShape<kFB, kFB, 4 * kFB, kFB / 2, 4 * kFB, kFB / 2, kFB / 2>;
#else  // ~40 KB: four regions per CU
using KfSmall = KfShape<kFB, 2 * kFB, 14 * kFB, kFB, 12 * kFB, kFB, kFB / 2>;
#endif
using KfBig = KfShape<1024, 2048, 8192, 256, 24576, 1024, 256>;
constexpr uint32_t kFBigU = 384;  // regions of more distinct haplotypes take KfBig

// correction: key << 12 | (-1) << 11 | local haplotype (key < 2^20)
__device__ __forceinline__ uint32_t cor_entry(uint32_t key, uint32_t l, uint32_t neg) {
    return (key << 12) | (neg << 11) | l;
}
__device__ __forceinline__ uint32_t cor_key(uint32_t c) { return c >> 12; }
__device__ __forceinline__ bool cor_neg(uint32_t c) { return (c >> 11) & 1u; }
__device__ __forceinline__ uint32_t cor_hap(uint32_t c) { return c & 2047u; }

// A placement the region body is compiled for (KfTyped: every list it names sits in
// LDS, its accesses are DS instructions) or finds out as it runs (KfAny: a branch in
// front of a DS or a global instruction); no pointer that may be either reaches a load.
using KfTyped = std::true_type;
using KfAny = std::false_type;
// KfAny's global side goes through pointers of the global address space: the branch's
// two loads then differ in type, and the compiler cannot merge them into one load
// through a pointer chosen at run time (a FLAT instruction, which waits on both counters).
typedef uint32_t kf_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t ld_global(const uint32_t *p) {
    return *(const __attribute__((address_space(1))) uint32_t *)p;
}
__device__ __forceinline__ uint2 ld_global(const uint2 *p) {
    const kf_u32x2 v = *(const __attribute__((address_space(1))) kf_u32x2 *)p;
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void st_global(uint32_t *p, uint32_t v) {
    *(__attribute__((address_space(1))) uint32_t *)p = v;
}

// The loads of one round have arrived (one wait per round) and stay where they were issued:
// without a use here the compiler sinks a load into the branch that needs it.
__device__ __forceinline__ void arrived(uint32_t &x) { asm volatile("" : "+v"(x)); }

// Appends v from the wave's lanes with want set, in lane order (one LDS atomic
// per wave), with put(slot, v); *n counts every attempt (> cap: overflow).
template <class Put>
__device__ __forceinline__ void wave_push(Put &&put, uint32_t *n, uint32_t cap, bool want, uint32_t v) {
    const uint64_t m = __ballot(want);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (want) {
        const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        if (at < cap) put(at, v);
    }
}

// Exclusive prefix of v over the workgroup (wave scans + the waves' totals in s_w).
template <uint32_t kFWaves>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kFWaves; w++) {
        const uint32_t t = s_w[w];
        pre += w < wave ? t : 0u;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return pre + x - v;
}

#ifdef TFBS_KF_FINE
#define KF_FINE(...) __VA_ARGS__
#else
#define KF_FINE(...)
#endif
// (the common shape: four workgroups per CU by its LDS, so at least four waves per SIMD -- the
// register allocator's bound, 128 VGPRs; without it the region body takes 150)
#ifndef TFBS_KF_WAVES
#define TFBS_KF_WAVES 4
#endif
template <class C>
__global__ __launch_bounds__(C::kBlock) __attribute__((amdgpu_waves_per_eu(C::kBlock == 1024 ? 1 : TFBS_KF_WAVES)))
void key_fast_kernel(AsmArgs A, uint32_t first, uint32_t count, uint32_t which) {
    constexpr int kFBlock = C::kBlock;
    constexpr uint32_t kFWaves = C::kWaves, kFHapLds = C::kHapLds, kFCor = C::kCor, kFRefs = C::kRefs,
                       kFCnt = C::kCnt, kFRuns = C::kRuns, kFRows = C::kRows, kFLists = C::kLists;
    constexpr uint32_t kPerW = kFKeyWords >= (uint32_t)kFBlock ? kFKeyWords / kFBlock : 1u;  // key words per thread
    __shared__ uint32_t s_cor[kFCor];
    __shared__ uint4 s_ref[kFRefs];          // make_ref, sorted by window
    __shared__ uint32_t s_hap[kFHapLds];     // HAP_DEDUP: its first run (from the region's first) | runs << 16; else kFNone
    __shared__ uint32_t s_cnt[kFCnt];        // the counters; before them the diff runs (s_run)
    uint2 *const s_run = reinterpret_cast<uint2 *>(s_cnt);
    __shared__ uint32_t s_bits[kFKeyWords], s_rbase[kFKeyWords];
    __shared__ uint32_t s_rkey[kFRows], s_rr[kFRows];  // per row of a chunk: its key; R(key), then its varying slot
    __shared__ uint32_t s_loff[kFLists + 1], s_lidx[kFLists];
    __shared__ uint32_t s_w[kFWaves];
    __shared__ uint32_t s_ncor, s_nref, s_nvar, s_arena, s_ndirty, s_nsp;
    __shared__ unsigned long long s_vb[2];  // a chunk's share of the compact lists: first key, first count
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto process = [&](const uint32_t r, const uint32_t by_ticket, const uint64_t t_ticket) {  // one region (every exit is workgroup-uniform)
    // TFBS_KF_PROF: phase times 0-7 (wall_clock64: 100 MHz), then sizes (U, entries, dirty reference hits, rows,
    // chunks), then the first phase's own times 16-19 and, 20, the ticks from the ticket atomic
    // to the order entry in front of the region (kKfProfWords per region)
    auto stamp = [&](uint32_t k, uint64_t v) {
        if (A.prof && tid == 0) A.prof[kKfProfWords * (size_t)r + k] = v;
    };
    stamp(0, wall_clock64());
    stamp(20, t_ticket);
    // TFBS_KF_FINE (a build of its own: the product kernel's registers stay): thread 0's time in the
    // parts of the dirty phase and of the chunks, words kKfProfFine.. of the region's record
    KF_FINE(uint64_t tf[kKfProfFineN] = {}; uint64_t tf_last = 0;
            auto fine_start = [&]() { tf_last = wall_clock64(); };
            auto fine = [&](uint32_t k) {
                const uint64_t t = wall_clock64();
                tf[k] += t - tf_last;
                tf_last = t;
            };)
    // Round 1: every address from r alone, all issued before the first wait -- the region, its
    // static record (run0, nruns, lmax: launch_region_asm), its reference hit count and the
    // thread's reference hit (the buffer always holds it; used only below the count), its spill bucket
    // (spill_off[r] whatever the count: used only where the count is not 0)
    // (the front's addresses from a thread index the compiler takes as new per region: built from
    // tid itself they are hoisted out of the region loop, a register pair each for the kernel's whole run)
    uint32_t ft = tid;
    arrived(ft);
    // (no branch around a load -- a branch ends a round with a wait of its own --: a list this
    // launch does not have is read at `none`, the region's own record, and its value not used;
    // every wave reads the 64 reference hits, lane by lane)
    const uint32_t *const none = reinterpret_cast<const uint32_t *>(A.regions + r);
    auto have = [&](bool c, const auto *p) { return c ? p : reinterpret_cast<decltype(p)>(none); };
    // (records in place, AsmArgs::spill_inplace: the scan's count here, no bucket)
    const bool spills = A.spill_count != nullptr, inplace = spills && A.spill_inplace != 0, buckets = spills && !inplace;
    uint32_t n_rc = ld_global(have(A.mfma, A.ref_count + r));
    const uint2 rh = ld_global(have(A.mfma, reinterpret_cast<const uint2 *>(A.ref_hits) + (size_t)r * kRefPerRegion + (ft & 63u)));
    uint32_t rh_g = rh.x, rh_i = rh.y;
    uint32_t sp_n = ld_global(have(spills, A.spill_count));
    uint32_t sp_c = ld_global(have(buckets, A.spill_cnt + r));
    uint32_t sp_o = ld_global(have(buckets, A.spill_off + r));
    DevRegion rg = A.regions[r];
    uint4 ra = A.region_asm[r];
    arrived(n_rc), arrived(rh_g), arrived(rh_i), arrived(sp_n), arrived(sp_c), arrived(sp_o);
    arrived(rg.hap_count), arrived(ra.x);
    if (!spills) sp_n = 0;
    stamp(16, wall_clock64());
    const uint32_t U = rg.hap_count, n_inner = rg.n_inner, K = A.n_slots * n_inner;
    const uint64_t ko = (uint64_t)rg.inner_off * A.n_slots;
    // tfbs_ctx_assembly_trace: the region's path word, stored once where the region leaves
    uint32_t pw = TFBS_PATH_FAST | (kFBlock == 1024 ? TFBS_PATH_BIG : 0u) | by_ticket;
    auto trace = [&](uint32_t w) {
        if (A.path && tid == 0) A.path[r] = w;
    };
    if (U == 0 || K == 0) {  // no samples: no haplotype, no match, no key
        trace(pw);
        for (uint32_t j = tid; j < K; j += kFBlock) {
            A.key_first[ko + j] = 0;
            A.key_flags[ko + j] = 0;
        }
        return;
    }
    auto give_up = [&](uint32_t why) {  // workgroup-uniform, before any output
        if (tid == 0) {
            A.redo[atomicAdd(A.redo_n, 1u)] = r;
            if (A.why) atomicAdd(A.why + why, 1u);  // (TFBS_DEBUG_OVER: the reasons)
        }
        trace(pw | TFBS_PATH_GIVEUP | (why << TFBS_PATH_WHY_SHIFT));
    };
    if (U > (kFMaxU < A.fast_max_u ? kFMaxU : A.fast_max_u) || K > 32 * kFKeyWords || n_inner > 32) return give_up(0);
    const uint32_t hb = rg.hap_begin;
    const bool refs_on = A.mfma && rg.ref_hap != UINT32_MAX;
    // (the same in every lane: kept in scalar registers)
    const uint32_t run0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ra.x);
    const uint32_t nruns = (uint32_t)__builtin_amdgcn_readfirstlane((int)ra.y);
    const uint32_t lmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)ra.z);
    if (tid == 0) s_ncor = s_nref = s_ndirty = s_nsp = 0;  // (read behind block_excl_scan's barriers)
    // own hits: the wave lists of the region's haplotype groups (one hitn load per
    // thread), their entries read flat over the workgroup below
    const uint32_t g_lo = hb / A.hpb, g_hi = (hb + U - 1) / A.hpb;
    const uint32_t nl = A.mfma ? (g_hi + 1 - g_lo) * kMBlockWaves : 0u;
    // list t of the region's: group g's wave lists are g * kMBlockWaves .. + 7 (scan.hpp)
    auto list_idx = [&](uint32_t t) -> uint32_t { return g_lo * kMBlockWaves + t; };
    const bool lists_staged = nl <= kFLists;  // one list per thread: its offset and index kept for the list pass
    if (!lists_staged) pw |= TFBS_PATH_LISTS_SLICED;
    if (nruns >= 65536) return give_up(2);
    if (nruns > kFRuns) pw |= TFBS_PATH_RUNS_L2;
    // Round 2, all issued before the next wait: the haplotypes' reuse descriptors
    // (hap_reuse: what s_hap holds), the hit lists' lengths, the diff runs' first
    // sweep, the meta fields of the thread's reference hit
    constexpr uint32_t kHapQ = kFHapLds / kFBlock;
    // (again no branch around a load: a thread past a list's end reads the list's last entry,
    // a list that is not there is read at `none`)
    uint32_t hx[kHapQ];
#pragma unroll
    for (uint32_t q = 0; q < kHapQ; q++) hx[q] = ld_global(A.hap_reuse + hb + min(ft + q * kFBlock, U - 1));  // (U >= 1 here)
    // the region's entries (an upper bound of its hits: groups are shared)
    const uint32_t lidx = list_idx(min(ft, nl ? nl - 1 : 0u));
    uint32_t lcnt = ld_global(have(nl != 0, A.hitn + lidx));
    // the runs in LDS when they fit, else read from global memory (L2)
    const bool runs_lds = nruns <= kFRuns;
    const uint2 *const druns = reinterpret_cast<const uint2 *>(A.druns) + (nruns ? run0 : 0u);
    const uint2 run_first = ld_global(have(runs_lds && nruns != 0, druns + min(ft, nruns ? nruns - 1 : 0u)));
    uint32_t run_a = run_first.x, run_b = run_first.y;
    const uint32_t n_list = refs_on ? min(n_rc, kRefPerRegion) : 0u;
    const uint32_t g_ref = ft < n_list ? rh_g : 0u, sn = g_ref & 63u;
    const uint32_t *const meta = have(refs_on, reinterpret_cast<const uint32_t *>(A.mmeta) + (size_t)(g_ref >> 6) * kGMetaInts);
    uint32_t m_len = ld_global(meta + (refs_on ? kGStrandInts * sn + kGLen : 0u));
    uint32_t m_depth = ld_global(meta + (refs_on ? (uint32_t)kGDepth : 0u));
    uint32_t m_slot = ld_global(meta + (refs_on ? kGStrandInts * sn + kGSlot : 0u));
    // records in place: the thread's share of the scan's list, record ft + q * block, each one's
    // first word (region | kind << 31); a thread past the count reads the last record
    // (the 1 024-thread shape, at its register limit and beside the common one, reads them all in
    // rounds of their own: kSpFront = 0)
    constexpr uint32_t kSpFront = kFBlock == 1024 ? 0u : kSpillInPlace, kSpQ = kSpFront / kFBlock;
    static_assert(kSpFront % kFBlock == 0 && kSpQ <= 16, "a thread's records: a mask bit and a kind bit each");
    // (the count in a scalar register: a share past it is a branch of the wave's, no load, and an
    // assembly that reads the buckets, or no record, issues none)
    // (sp_all: every record read in place; those past the first kSpillInPlace -- C3: one step in
    // two hundred -- are read where they are used, in rounds of their own)
    const uint32_t sp_all = (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)(inplace ? min(sp_n, min(A.spill_inplace, A.spill_cap)) : 0u));
    const uint32_t sp_raw = min(sp_all, kSpFront);
    uint32_t sw[kSpQ ? kSpQ : 1];
#pragma unroll
    for (uint32_t q = 0; q < kSpQ; q++) {
        sw[q] = 0xFFFFFFFFu;  // (no region's)
        if (q * kFBlock < sp_raw) sw[q] = ld_global(A.spill_raw + 3 * (size_t)min(ft + q * kFBlock, sp_raw - 1));
    }
#pragma unroll
    for (uint32_t q = 0; q < kHapQ; q++) arrived(hx[q]);
    arrived(lcnt), arrived(run_a), arrived(run_b), arrived(m_len), arrived(m_depth), arrived(m_slot);
    // the region's records among the thread's: bit q (its record q), bit 16 + q (a reference hit)
    // (without a record nothing of it runs: a branch of the wave's)
    uint32_t sp_m = 0;
    if (sp_raw) {
#pragma unroll
        for (uint32_t q = 0; q < kSpQ; q++) {
            arrived(sw[q]);
            if (ft + q * kFBlock < sp_raw && (sw[q] & 0x7FFFFFFFu) == r) sp_m |= (1u | (sw[q] >> 31) << 16) << q;
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < kHapQ; q++)
        if (ft + q * kFBlock >= U) hx[q] = kFNone;
    if (ft >= nl) lcnt = 0;
    for (uint32_t t = ft + kFBlock; t < nl; t += kFBlock) lcnt += ld_global(A.hitn + list_idx(t));  // (past kFBlock lists)
    stamp(17, wall_clock64());
#pragma unroll
    for (uint32_t q = 0; q < kHapQ; q++) {
        const uint32_t l = tid + q * kFBlock;
        if (l < U) s_hap[l] = hx[q];
    }
    uint32_t n_ent = 0;
    const uint32_t loff = block_excl_scan<kFWaves>(lcnt, s_w, n_ent);
    if (lists_staged && tid < nl) {
        s_lidx[tid] = lidx;
        s_loff[tid] = loff;
    }
    if (lists_staged && tid == 0) s_loff[nl] = n_ent;
    stamp(1, wall_clock64());
    auto hap_info = [&](uint32_t l) -> uint32_t {  // s_hap's entry of any haplotype
        if (l < kFHapLds) return s_hap[l];
        return ld_global(A.hap_reuse + hb + l);
    };
    auto run_at = [&](auto typed, uint32_t k) -> uint2 {  // run k of the region's, by placement
        if constexpr (decltype(typed)::value) {
            return s_run[k];
        } else {
            if (runs_lds) return s_run[k];
            return ld_global(druns + k);
        }
    };
    if (runs_lds) {
        if (tid < nruns) s_run[tid] = make_uint2(run_a, run_b);
        for (uint32_t k = tid + kFBlock; k < nruns; k += kFBlock) s_run[k] = ld_global(druns + k);
    }
    stamp(18, wall_clock64());
    // reference hits: the region's list, then its spill records of kind 1
    const uint2 sp = buckets && sp_n && sp_c ? make_uint2(sp_o, sp_o + sp_c) : make_uint2(0, 0);  // (spill_range)
    // (in place: the region's records counted -- s_nsp, zeroed in front of block_excl_scan's
    // barriers, read behind the next scan's --, its reference hits from the threads that hold them)
    if (sp_m) atomicAdd(&s_nsp, (uint32_t)__popc(sp_m & 0xFFFFu));
    if (refs_on)
        for (uint32_t m = sp_m >> 16; m; m &= m - 1) {
            const uint32_t *q = A.spill_raw + 3 * (size_t)(tid + (uint32_t)__builtin_ctz(m) * kFBlock);
            const uint32_t at = atomicAdd(&s_nref, 1u);
            if (at < kFRefs) s_ref[at] = make_ref(A, rg, q[1], q[2]);
        }
    for (uint32_t e = kSpFront + tid; e < sp_all; e += kFBlock) {  // (records past the front's round)
        const uint32_t *q = A.spill_raw + 3 * (size_t)e;
        const uint32_t w = q[0];
        if ((w & 0x7FFFFFFFu) != r) continue;
        atomicAdd(&s_nsp, 1u);
        if (refs_on && (w >> 31)) {
            const uint32_t at = atomicAdd(&s_nref, 1u);
            if (at < kFRefs) s_ref[at] = make_ref(A, rg, q[1], q[2]);
        }
    }
    if (refs_on) {
        if (tid < n_list) {
            const uint32_t at = atomicAdd(&s_nref, 1u);
            if (at < kFRefs) s_ref[at] = make_ref_loaded(A, rg, m_len, m_depth, m_slot, rh_i);
        }
        for (uint32_t e = sp.x + tid; e < sp.y; e += kFBlock) {
            const uint32_t *q = A.spill_sorted + 3 * (size_t)e;
            if (q[0] >> 31) {
                const uint32_t at = atomicAdd(&s_nref, 1u);
                if (at < kFRefs) s_ref[at] = make_ref(A, rg, q[1], q[2]);
            }
        }
    }
    __syncthreads();
    const uint32_t nref = s_nref;
    stamp(19, wall_clock64());
    if (nref > kFRefs) return give_up(3);
    // D: per HAP_DEDUP haplotype the reference hits in its dirty windows (a run
    // [a, b] meets the columns [w, w + L - 1] of window w).  Up to 64 Ki (haplotype,
    // reference hit) pairs are tested pairwise, a lane per haplotype and a lane mask per
    // hit (dirty_hits below); past that the hits are sorted
    // by window and each haplotype walks its runs over them (a hit in [a - 31, b] of
    // run [a, b] tested once: runs ascend, the cursor only moves forward).
    const bool pairwise = (uint64_t)U * nref <= 65536;
    if (!pairwise) pw |= TFBS_PATH_WALK;
    if (!pairwise) {  // the reference hits by window (rank sort; ties by list position)
        uint4 mine = make_uint4(0, 0, 0, 0);
        uint32_t rank = 0;
        if (tid < nref) {
            mine = s_ref[tid];
            for (uint32_t j = 0; j < nref; j++) {
                const uint32_t w = s_ref[j].y;
                rank += (w < mine.y || (w == mine.y && j < tid)) ? 1u : 0u;
            }
        }
        __syncthreads();
        if (tid < nref) s_ref[rank] = mine;
        __syncthreads();
    }
    stamp(2, wall_clock64());
    KF_FINE(fine_start();)
    // The pairwise test, hit-major: a wave takes 64 haplotypes, a lane each, and a slice of at most
    // 64 of its share [h0, h1) of the reference hits.  Lane p of the slice holds hit p's record; a
    // group of kDGroup hits has its first and last column in scalar registers (v_readlane: no LDS
    // read), each lane reads its runs once per group (the run loop is the wave's: a lane past its
    // own tries a run that meets nothing), and a (run, hit) test is two vector compares whose lane
    // mask is OR-ed into the hit's 64-bit scalar mask.  Hit p's mask then sits in lane p; the
    // slice's corrections are counted in scalars (dirty haplotypes x inner ranges per hit), take one
    // slot reservation, and are listed hit by hit: every dirty lane stores its entry at the
    // base + the hits before + its rank among the dirty lanes.  put(slot, entry); returns the
    // wave's count (the same in every lane).
    // A region whose haplotype blocks fill at most half of the workgroup's waves gives each block to
    // several waves, which take shares of the hits.
    constexpr uint32_t kDGroup = 8;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    const uint32_t nblk = (U + 63) / 64;
    const uint32_t shares = 2 * nblk <= kFWaves ? kFWaves / nblk : 1u;
    auto dirty_hits = [&](auto typed, uint32_t *ctr, auto &&put) -> uint32_t {
        uint32_t total = 0;
        const uint32_t share = shares > 1 ? wv / nblk : 0u;
        if (share >= shares) return 0;  // (a wave left over: kFWaves is no multiple of the blocks)
        const uint32_t per = (nref + shares - 1) / shares;
        const uint32_t h0 = min(share * per, nref), h1 = min(h0 + per, nref);
        for (uint32_t l0 = 64 * (shares > 1 ? wv % nblk : wv); l0 < U; l0 += shares > 1 ? 64 * nblk : kFBlock) {
            const uint32_t l = l0 + lane;
            const uint32_t x = l < U ? hap_info(l) : kFNone;
            const uint32_t k0 = x == kFNone ? 0u : x & 0xFFFFu, nk = x == kFNone ? 0u : x >> 16;
            for (uint32_t p0 = h0; p0 < h1; p0 += 64) {
                const uint32_t np = min(64u, h1 - p0);
                // (a lane past the slice: a hit no run meets)
                uint32_t rw = 0xFFFFFFFFu, re = 0, rx = 0, rb = 0;
                if (lane < np) {
                    const uint4 q = s_ref[p0 + lane];
                    rw = q.y, re = q.y + (q.z & 0xFFFFu) - 1, rx = q.x, rb = q.w;
                }
                uint32_t mlo = 0, mhi = 0, tot = 0;
                for (uint32_t g0 = 0; g0 < np; g0 += kDGroup) {
                    uint32_t w[kDGroup], e[kDGroup];
                    uint64_t mk[kDGroup];
#pragma unroll
                    for (uint32_t g = 0; g < kDGroup; g++) {
                        w[g] = (uint32_t)__builtin_amdgcn_readlane((int)rw, (int)(g0 + g));
                        e[g] = (uint32_t)__builtin_amdgcn_readlane((int)re, (int)(g0 + g));
                        mk[g] = 0;
                    }
                    for (uint32_t i = 0; __ballot(i < nk) != 0; i++) {
                        uint2 ab = make_uint2(0xFFFFFFFFu, 0u);
                        if (i < nk) ab = run_at(typed, k0 + i);
#pragma unroll
                        for (uint32_t g = 0; g < kDGroup; g++)  // (run_meets: a <= w + L - 1 and b >= w)
                            mk[g] |= __builtin_amdgcn_uicmp(ab.x, e[g], 37) & __builtin_amdgcn_uicmp(ab.y, w[g], 35);  // (ule, uge: lane masks)
                    }
#pragma unroll
                    for (uint32_t g = 0; g < kDGroup; g++) {
                        if (lane == g0 + g) mlo = (uint32_t)mk[g], mhi = (uint32_t)(mk[g] >> 32);
                        tot += (uint32_t)__popcll(mk[g]) * (uint32_t)__popc((uint32_t)__builtin_amdgcn_readlane((int)rb, (int)(g0 + g)));
                    }
                }
                KF_FINE(fine(0);)
                if (tot == 0) continue;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(ctr, tot);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                total += tot;
                for (uint64_t hm = __ballot((mlo | mhi) != 0); hm; hm &= hm - 1) {  // the slice's dirty hits
                    const int p = __builtin_ctzll(hm);
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)mlo, p);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)mhi, p);
                    const uint32_t qx = (uint32_t)__builtin_amdgcn_readlane((int)rx, p);
                    const uint32_t qb = (uint32_t)__builtin_amdgcn_readlane((int)rb, p);
                    const bool mine = (((uint64_t)hi << 32 | lo) >> lane) & 1u;
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0));
                    const uint32_t n = (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
                    for (uint32_t b = qb; b; b &= b - 1, base += n)
                        if (mine) put(base + rank, cor_entry(qx + (uint32_t)__builtin_ctz(b), l, 1));
                }
                KF_FINE(fine(1);)
            }
        }
        return total;
    };
    // f(l, reference hit) for every dirty pair, each lane on its own
    auto dirty_walk = [&](auto typed, auto &&f) {
        for (uint32_t l = tid; l < U; l += kFBlock) {
            const uint32_t x = hap_info(l);
            if (x == kFNone) continue;
            const uint32_t k0 = x & 0xFFFFu, k1 = k0 + (x >> 16);
            uint32_t p = 0;
            for (uint32_t k = k0; k < k1 && p < nref; k++) {
                const uint2 ab = run_at(typed, k);
                const uint32_t a = ab.x, b = ab.y;
                const uint32_t lo = a >= kMChunkCols * kMMaxChunks - 1 ? a - (kMChunkCols * kMMaxChunks - 1) : 0u;
                while (p < nref && s_ref[p].y < lo) p++;
                for (; p < nref && s_ref[p].y <= b; p++) {
                    const uint4 q = s_ref[p];
                    bool dirty = false;
                    for (uint32_t k2 = k0; k2 < k1 && !dirty; k2++) {
                        const uint2 r2 = run_at(typed, k2);
                        dirty = run_meets(r2.x, r2.y, q.y, q.z & 0xFFFFu);
                    }
                    if (dirty) f(l, q);
                }
            }
        }
    };
    // pairwise mode lists the dirty corrections while counting them, at the top of
    // s_cor downwards (the first kFCor); the walk lists them in a second pass
    // (TFBS_PATH_STEPBITS: the figure the report has carried since a wave kept one bit
    // per pairwise step of hpw haplotypes x rpl hits -- wave 0 had at most 64 of them)
    const uint32_t rpl = nref <= 1 ? 1u : nref >= 64 ? 64u : 1u << (32 - __clz(nref - 1));
    const uint32_t hpw = 64 / rpl, n_p = (nref + rpl - 1) / rpl;
    const bool stepbits = pairwise && (U + kFWaves * hpw - 1) / (kFWaves * hpw) * n_p <= 64;
    uint32_t nd = 0;
    if (nref) {
        auto count_and_list = [&](auto typed) {
            if (pairwise) {
                const uint32_t c = dirty_hits(typed, &s_ndirty, [&](uint32_t at, uint32_t v) {
                    if (at < kFCor) s_cor[kFCor - 1 - at] = v;
                });
                nd += lane == 0 ? c : 0u;  // (the wave's count once)
            } else
                dirty_walk(typed, [&](uint32_t, const uint4 &q) { nd += __popc(q.w); });
        };
        if (runs_lds) count_and_list(KfTyped{});
        else count_and_list(KfAny{});
    }
    uint32_t nD = 0;
    (void)block_excl_scan<kFWaves>(nd, s_w, nD);
    const bool dirty_listed = pairwise && nD <= kFCor;
    // the corrections' list: LDS when they fit (own hits from the bottom, the dirty
    // ones at the top), else a share of the launch's arena (the dirty ones first)
    // (an upper bound: entries of other regions' haplotypes; the region's spill records from its
    // bucket, or counted in place -- the same figure, so the same placement)
    const uint32_t need = n_ent + (sp.y - sp.x) + s_nsp + nD;
    const bool in_lds = need <= (kFCor < A.cor_lds ? kFCor : A.cor_lds);
    pw |= (stepbits ? TFBS_PATH_STEPBITS : 0u) | (dirty_listed ? TFBS_PATH_DIRTY_LISTED : 0u) |
          (in_lds ? 0u : TFBS_PATH_COR_ARENA);
    if (tid == 0) {
        s_arena = kFNone;
        if (!in_lds) {
            const uint32_t at = atomicAdd(A.cor_used, need);
            if (at <= A.cor_cap && need <= A.cor_cap - at) s_arena = at;
            if (dirty_listed) s_ncor = nD;
        }
    }
    __syncthreads();
    if (!in_lds && s_arena == kFNone) return give_up(4);  // the host grows the arena for the next call
    stamp(3, wall_clock64());
    KF_FINE(fine(2);)
    uint32_t *const cor_g = A.cor_arena + (in_lds ? 0u : s_arena);  // (the arena share: global memory)
    auto cor_ld = [&](auto typed, uint32_t e) -> uint32_t {  // entry e of the list, by placement
        if constexpr (decltype(typed)::value) {
            return s_cor[e];
        } else {
            if (in_lds) return s_cor[e];
            return ld_global(cor_g + e);
        }
    };
    auto cor_st = [&](auto typed, uint32_t e, uint32_t v) {
        if constexpr (decltype(typed)::value) {
            s_cor[e] = v;
        } else {
            if (in_lds) s_cor[e] = v;
            else st_global(cor_g + e, v);
        }
    };
    if (!in_lds && dirty_listed)
        for (uint32_t e = tid; e < nD; e += kFBlock) st_global(cor_g + e, s_cor[kFCor - 1 - e]);
    const uint32_t nw = (K + 31) / 32;
    uint32_t nA = 0, nB = 0, ncor = 0, T = 0;
    // the list and the touched keys, compiled twice: for corrections and runs in LDS
    // (typed), and for any placement
    auto lists_and_rows = [&](auto typed) {
    auto put = [&](uint32_t at, uint32_t v) { cor_st(typed, at, v); };
    const uint2 *hitl = reinterpret_cast<const uint2 *>(A.hitl);
    for (uint32_t l0 = 0; l0 < nl; l0 += kFLists) {  // kFLists lists at a time: their offsets in LDS
        const uint32_t nlc = min(kFLists, nl - l0);
        uint32_t tot = n_ent;
        if (!lists_staged) {
            uint32_t lc = 0;
            if (tid < nlc) {
                const uint32_t idx = list_idx(l0 + tid);
                lc = A.hitn[idx];
                s_lidx[tid] = idx;
            }
            const uint32_t off = block_excl_scan<kFWaves>(lc, s_w, tot);
            if (tid < nlc) s_loff[tid] = off;
            if (tid == 0) s_loff[nlc] = tot;
            __syncthreads();
        }
        for (uint32_t e0 = 0; e0 < tot; e0 += kFBlock * kFBatch) {  // kFBatch loads in flight per thread
            uint2 h[kFBatch];
#pragma unroll
            for (uint32_t q = 0; q < kFBatch; q++) {
                const uint32_t e = e0 + q * kFBlock + tid;
                h[q] = make_uint2(hb + U, 0);  // (no entry: not the region's)
                if (e < tot) {
                    uint32_t lo = 0, hi = nlc - 1;  // the list holding entry e: the last with s_loff <= e
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi + 1) / 2;
                        if (s_loff[mid] <= e) lo = mid;
                        else hi = mid - 1;
                    }
                    const uint32_t idx = s_lidx[lo];
                    h[q] = hitl[(size_t)(idx / kMBlockWaves) * A.cand_cap +
                                (size_t)(idx % kMBlockWaves) * (A.cand_cap / kMBlockWaves) + (e - s_loff[lo])];
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < kFBatch; q++)
                wave_push(put, &s_ncor, need, h[q].x - hb < U, cor_entry(h[q].y, h[q].x - hb, 0));
        }
        __syncthreads();  // s_loff / s_lidx reused by the next lists
    }
    for (uint32_t e0 = sp.x; e0 < sp.y; e0 += kFBlock) {  // own hits of the spill list (kind 0)
        const uint32_t e = e0 + tid;
        bool want = false;
        uint32_t v = 0;
        if (e < sp.y) {
            const uint32_t *q = A.spill_sorted + 3 * (size_t)e;
            want = !(q[0] >> 31) && q[1] - hb < U;
            v = cor_entry(q[2], q[1] - hb, 0);
        }
        wave_push(put, &s_ncor, need, want, v);
    }
    // (in place: the own hits among the threads' records, a record per lane and turn of the wave)
    for (uint32_t m = sp_m & ~(sp_m >> 16) & 0xFFFFu; __ballot(m != 0) != 0; m &= m - 1) {
        bool want = false;
        uint32_t v = 0;
        if (m) {
            const uint32_t *q = A.spill_raw + 3 * (size_t)(tid + (uint32_t)__builtin_ctz(m) * kFBlock);
            want = q[1] - hb < U;
            v = cor_entry(q[2], q[1] - hb, 0);
        }
        wave_push(put, &s_ncor, need, want, v);
    }
    for (uint32_t e0 = kSpFront; e0 < sp_all; e0 += kFBlock) {  // (and those past the front's round)
        const uint32_t e = e0 + tid;
        bool want = false;
        uint32_t v = 0;
        if (e < sp_all) {
            const uint32_t *q = A.spill_raw + 3 * (size_t)e;
            want = q[0] == r && q[1] - hb < U;  // (bit 31 clear: an own hit)
            v = cor_entry(q[2], q[1] - hb, 0);
        }
        wave_push(put, &s_ncor, need, want, v);
    }
    if (!dirty_listed && nref) {  // (the walk, or more dirty corrections than the top of s_cor holds)
        KF_FINE(fine_start();)
        auto put_in = [&](uint32_t at, uint32_t v) {
            if (at < need) cor_st(typed, at, v);
        };
        if (pairwise)
            (void)dirty_hits(typed, &s_ncor, put_in);
        else
            dirty_walk(typed, [&](uint32_t l, const uint4 &q) {
                uint32_t at = atomicAdd(&s_ncor, (uint32_t)__popc(q.w));
                for (uint32_t m = q.w; m; m &= m - 1, at++) put_in(at, cor_entry(q.x + __builtin_ctz(m), l, 1));
            });
    }
    for (uint32_t w = tid; w < nw; w += kFBlock) s_bits[w] = 0;
    __syncthreads();
    stamp(4, wall_clock64());
    // the corrections: [0, nA) and, listed at the top of s_cor, [kFCor - nB, kFCor)
    nA = s_ncor, nB = in_lds && dirty_listed ? nD : 0u, ncor = nA + nB;  // (nA <= need)
    // touched keys: own hits (the dirty reference hits' keys are reference keys),
    // reference hits, every key of a LUT/generic slot; rows in key order
    for (uint32_t e = tid; e < nA; e += kFBlock) {
        const uint32_t c = cor_ld(typed, e);
        if (!cor_neg(c)) atomicOr(&s_bits[cor_key(c) >> 5], 1u << (cor_key(c) & 31u));
    }
    if (tid < nref)
        for (uint32_t m = s_ref[tid].w; m; m &= m - 1) {
            const uint32_t key = s_ref[tid].x + __builtin_ctz(m);
            atomicOr(&s_bits[key >> 5], 1u << (key & 31u));
        }
    if (A.any_dense)
        for (uint32_t j = tid; j < K; j += kFBlock)
            if (!A.slot_mfma[j / n_inner]) atomicOr(&s_bits[j >> 5], 1u << (j & 31u));
    __syncthreads();
    {
        constexpr uint32_t per = kPerW;
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t q = 0; q < per; q++) {
            const uint32_t w = tid * per + q;
            if (w < nw) mine += __popc(s_bits[w]);
        }
        uint32_t run = block_excl_scan<kFWaves>(mine, s_w, T);
#pragma unroll
        for (uint32_t q = 0; q < per; q++) {
            const uint32_t w = tid * per + q;
            if (w < nw) {
                s_rbase[w] = run;
                run += __popc(s_bits[w]);
            }
        }
    }
    };
    if (in_lds && runs_lds) lists_and_rows(KfTyped{});
    else lists_and_rows(KfAny{});
    __syncthreads();  // s_rbase written: row_of reads other threads' words from here on
    stamp(5, wall_clock64());
    auto row_of = [&](uint32_t j) { return s_rbase[j >> 5] + __popc(s_bits[j >> 5] & ((1u << (j & 31)) - 1u)); };
    // the counter block: LDS chunks of rows x U, or -- when that would take more than
    // 32 chunks (hundreds of haplotypes and keys: each chunk re-reads every
    // correction and costs a few barriers) -- chunks of kFRows rows in a share of
    // the arena (global atomics)
    // u16 counters in LDS (two per word) when no count can reach 2^16, also while the
    // corrections land: a key's count on a haplotype is at most its 2 strands'
    // windows (< 2 x length), but the unordered atomics can add every +1 (own hits,
    // < 2 x length) to the base R (< 2 x length) before any -1, so the bound is
    // 4 x length; the -1 corrections never take a count below 0 (a haplotype's
    // dirty reference hits on a key are some of its base R), so a packed pair
    // never borrows or carries
    const bool half = 4 * (lmax + 64) < 65536 && A.cor_lds != 0;
    uint32_t rows_per = min((half ? 2 : 1) * kFCnt / U, kFRows);
    uint16_t *const cnt16 = reinterpret_cast<uint16_t *>(s_cnt);
    bool h16 = half, cnt_arena = false;
    uint32_t *cnt_g = A.cor_arena;  // (the counters' arena share: global memory)
    if ((T + rows_per - 1) / rows_per > 32 || A.cor_lds == 0) {  // (cor_lds 0: the tests' all-global path)
        h16 = false;
        cnt_arena = true;
        pw |= TFBS_PATH_CNT_ARENA;
        rows_per = min(T, kFRows);
        if (tid == 0) {
            s_arena = kFNone;
            const uint32_t want = rows_per * U, at = atomicAdd(A.cor_used, want);
            if (at <= A.cor_cap && want <= A.cor_cap - at) s_arena = at;
        }
        __syncthreads();
        if (s_arena == kFNone) return give_up(5);  // the host grows the arena for the next call
        cnt_g = A.cor_arena + s_arena;
    }
    pw |= (h16 ? 0u : TFBS_PATH_U32) | (U > kFHapLds ? TFBS_PATH_HAP_GLOBAL : 0u);
    // untouched keys: no match -- no key in the reference's HashMap
    for (uint32_t j = tid; j < K; j += kFBlock)
        if (!((s_bits[j >> 5] >> (j & 31)) & 1u)) {
            A.key_first[ko + j] = 0;
            A.key_flags[ko + j] = 0;
        }
    const uint64_t dense_base = A.dense_base ? A.haps[hb].count_off : 0;
    uint64_t t_atomics = 0;  // (TFBS_KF_PROF)
    // the counter chunks, compiled twice: for corrections in LDS and packed u16 counters
    // (typed: h16 is a constant there), and for any placement of either
    auto chunks = [&](auto typed) {
    constexpr bool kTyped = decltype(typed)::value;
    // where correction e sits: the list, or the dirty ones at the top of s_cor
    auto cor_top = [&](uint32_t e) -> uint32_t { return kFCor - nB + (e - nA); };
    auto cor_at = [&](uint32_t e) -> uint32_t {
        if constexpr (kTyped) return s_cor[e < nA ? e : cor_top(e)];
        else return e < nA ? cor_ld(typed, e) : s_cor[cor_top(e)];
    };
    auto cnt_set = [&](uint32_t x, uint32_t v) {
        if (kTyped || h16) cnt16[x] = (uint16_t)v;
        else if (cnt_arena) st_global(cnt_g + x, v);
        else s_cnt[x] = v;
    };
    auto cnt_add = [&](uint32_t x, uint32_t d) {  // d: +1 | -1
        if (kTyped || h16) atomicAdd(&s_cnt[x >> 1], d << (16 * (x & 1u)));
        else if (cnt_arena) atomicAdd(&cnt_g[x], d);
        else atomicAdd(&s_cnt[x], d);
    };
    auto count_at = [&](uint32_t x) -> uint32_t {
        if (kTyped || h16) return (uint32_t)cnt16[x];
        if (cnt_arena) return ld_global(cnt_g + x);
        return s_cnt[x];
    };
    KF_FINE(fine_start();)
    // the corrections by row (key << 12 becomes row << 12: no row_of per chunk)
    for (uint32_t e = tid; e < ncor; e += kFBlock) {
        const uint32_t c = cor_at(e), v = (row_of(cor_key(c)) << 12) | (c & 4095u);
        if (e < nA) cor_st(typed, e, v);
        else s_cor[cor_top(e)] = v;
    }
    KF_FINE(fine(3);)
    uint32_t dedup_bits = 0;  // bit i: haplotype lane + 64 i takes the reference's counts as its base
    for (uint32_t i = 0, l = lane; l < U; i++, l += 64)
        if (hap_info(l) != kFNone) dedup_bits |= 1u << i;
    // R(j), the reference hits on key j (the same in every lane), by the wave together: a hit adds to
    // the keys x + (a bit of w), so each hit counts at most once -- a ballot.  Hit `lane` (fx, fw: its
    // first key and ranges, read once per chunk) is in registers; the hits past 64 are read again
    auto ref_count = [&](uint32_t j, uint32_t fx, uint32_t fw) -> uint32_t {
        uint32_t d = j - fx;
        uint32_t R = (uint32_t)__popcll(__ballot(d < 32 && ((fw >> d) & 1u)));
        for (uint32_t p0 = 64; p0 < nref; p0 += 64) {
            uint32_t x = 0, w = 0;
            if (p0 + lane < nref) {
                const uint4 q = s_ref[p0 + lane];
                x = q.x, w = q.w;
            }
            d = j - x;
            R += (uint32_t)__popcll(__ballot(d < 32 && ((w >> d) & 1u)));
        }
        return R;
    };
    // rows [t0, t0 + nrow)'s keys into s_rkey[0, nrow), from the key words this thread scanned (rows
    // [s_rbase[w], ..)): once for the region when its rows fit s_rkey, else per chunk
    auto row_keys = [&](uint32_t t0, uint32_t nrow) {
        constexpr uint32_t per = kPerW;
#pragma unroll
        for (uint32_t q = 0; q < per; q++) {
            const uint32_t w = tid * per + q;
            if (w >= nw) continue;
            uint32_t t = s_rbase[w], b = s_bits[w];
            if (t >= t0 + nrow || t + __popc(b) <= t0) continue;
            for (; b; b &= b - 1, t++)
                if (t - t0 < nrow) s_rkey[t - t0] = 32 * w + __builtin_ctz(b);
        }
    };
    if constexpr (kFBlock == 1024) {
    // The 1 024-thread shape keeps the chunk body it had (the row-lane body below takes it past its
    // 128 registers): keys and R per chunk through s_rr, a wave's rows one after another
    for (uint32_t t0 = 0; t0 < T; t0 += rows_per) {
        const uint32_t nrow = min(rows_per, T - t0);
        __syncthreads();  // s_rbase / cor rows written, the previous chunk's readers done
        if (tid == 0) s_nvar = 0;
        row_keys(t0, nrow);
        for (uint32_t rr = tid; rr < nrow; rr += kFBlock) s_rr[rr] = 0;
        __syncthreads();
        if (tid < nref)  // R: reference hits per key
            for (uint32_t m = s_ref[tid].w; m; m &= m - 1) {
                const uint32_t t = row_of(s_ref[tid].x + __builtin_ctz(m)) - t0;
                if (t < nrow) atomicAdd(&s_rr[t], 1u);
            }
        __syncthreads();
        for (uint32_t rr = wave; rr < nrow; rr += kFWaves) {  // the base of every haplotype
            const uint32_t j = s_rkey[rr], R = s_rr[rr];
            const bool dense = A.any_dense && !A.slot_mfma[j / n_inner];
            for (uint32_t i = 0, l = lane; l < U; i++, l += 64) {
                const uint32_t v = dense ? A.counts[dense_base + (uint64_t)j * rg.count_stride + l]
                                         : ((dedup_bits >> i) & 1u ? R : 0u);
                cnt_set(rr * U + l, v);
            }
        }
        __syncthreads();
        for (uint32_t e = tid; e < ncor; e += kFBlock) {
            const uint32_t c = cor_at(e);
            const uint32_t t = cor_key(c) - t0;  // (its row)
            if (t < nrow) cnt_add(t * U + cor_hap(c), cor_neg(c) ? 0xFFFFFFFFu : 1u);
        }
        __syncthreads();
        // classify: one wave per row
        for (uint32_t rr = wave; rr < nrow; rr += kFWaves) {
            const uint32_t c0 = count_at(rr * U);
            uint32_t any = 0, diff = 0;
            for (uint32_t l = lane; l < U; l += 64) {
                const uint32_t c = count_at(rr * U + l);
                any |= c;
                diff |= c ^ c0;
            }
            const bool a = __ballot(any != 0) != 0, v = __ballot(diff != 0) != 0;
            if (lane == 0) {
                const uint32_t j = s_rkey[rr];
                A.key_first[ko + j] = c0;
                A.key_flags[ko + j] = (uint8_t)((a ? KEY_ANY : 0) | (v ? KEY_VARIES : 0));
                s_rr[rr] = v ? atomicAdd(&s_nvar, 1u) : kFNone;
            }
        }
        __syncthreads();
        const uint64_t ta = A.prof ? wall_clock64() : 0;
        if (tid == 0 && s_nvar) {  // the chunk's share of the compact lists
            s_vb[0] = atomicAdd(A.var_tot, (unsigned long long)s_nvar);
            s_vb[1] = atomicAdd(A.var_tot + 1, (unsigned long long)s_nvar * U);
        }
        __syncthreads();
        if (A.prof) t_atomics += wall_clock64() - ta;
        for (uint32_t rr = wave; rr < nrow; rr += kFWaves) {
            const uint32_t slot = s_rr[rr];
            if (slot == kFNone) continue;
            const uint64_t vi = s_vb[0] + slot, off = s_vb[1] + (uint64_t)slot * U;
            if (vi >= A.var_keys_cap || off + U > A.var_cap) continue;  // the host grows the lists and reruns
            if (lane == 0) A.var_keys[vi] = DevVarKey{r, s_rkey[rr], off};
            for (uint32_t l = lane; l < U; l += 64) A.var_counts[off + l] = count_at(rr * U + l);
        }
    }
    } else {
    const bool keys_once = T <= kFRows;
    // (the rows' lane terms from a thread index the compiler takes as new per region: built from tid
    // itself they are hoisted out of the region loop, registers for the kernel's whole run)
    uint32_t ct = tid;
    arrived(ct);
    const uint32_t cl = ct & 63u;
    if (keys_once) row_keys(0, T);
    // a wave takes rows wv, wv + kFWaves, ..; its i-th row's key and results stay in lane i (a chunk
    // has at most kFRows rows: 64 per wave), and no LDS read of a row waits for the row before
    static_assert(kFRows <= 64 * kFWaves, "a wave's rows of a chunk: one per lane");
    for (uint32_t t0 = 0; t0 < T; t0 += rows_per) {
        const uint32_t nrow = min(rows_per, T - t0);
        __syncthreads();  // cor rows and row keys written, the previous chunk's readers done
        if (!keys_once) {
            row_keys(t0, nrow);
            __syncthreads();
        }
        const uint32_t kb = keys_once ? t0 : 0u;  // the chunk's keys: s_rkey[kb, kb + nrow)
        KF_FINE(fine(4);)
        uint32_t fx = 0, fw = 0;
        if (lane < nref) {
            const uint4 q = s_ref[lane];
            fx = q.x, fw = q.w;
        }
        // (the keys of the wave's rows: one read, row i's in lane i, handed out by v_readlane)
        const uint32_t my_rr = wv + cl * kFWaves;  // the row whose key and results this lane holds
        const uint32_t my_j = s_rkey[kb + min(my_rr, nrow - 1)];
        for (uint32_t rr = wv, ri = 0; rr < nrow; rr += kFWaves, ri++) {  // the base of every haplotype
            const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)my_j, (int)ri);
            const uint32_t R = ref_count(j, fx, fw);
            const bool dense = A.any_dense && !A.slot_mfma[j / n_inner];
            for (uint32_t i = 0, l = lane; l < U; i++, l += 64) {
                const uint32_t v = dense ? A.counts[dense_base + (uint64_t)j * rg.count_stride + l]
                                         : ((dedup_bits >> i) & 1u ? R : 0u);
                cnt_set(rr * U + l, v);
            }
        }
        __syncthreads();
        KF_FINE(fine(5);)
        for (uint32_t e = tid; e < ncor; e += kFBlock) {
            const uint32_t c = cor_at(e);
            const uint32_t t = cor_key(c) - t0;  // (its row)
            if (t < nrow) cnt_add(t * U + cor_hap(c), cor_neg(c) ? 0xFFFFFFFFu : 1u);
        }
        __syncthreads();
        KF_FINE(fine(6);)
        // classify: one wave per row.  A lane past U reads haplotype U - 1 again (no branch around the
        // reads); the first haplotype's count is lane 0's first
        uint32_t my_res = 0;  // the first haplotype's count (< 2^30) | KeyFlags << 30
        {  // (the next row's first two reads are issued before this row's are used)
            const uint32_t la = min(cl, U - 1), lb = min(cl + 64, U - 1);
            uint32_t na = count_at(min(wv, nrow - 1) * U + la), nb = count_at(min(wv, nrow - 1) * U + lb);
            for (uint32_t rr = wv, i = 0; rr < nrow; rr += kFWaves, i++) {
                const uint32_t ca = na, cb = nb, nx = min(rr + kFWaves, nrow - 1) * U;
                na = count_at(nx + la), nb = count_at(nx + lb);
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ca);
                uint32_t any = ca | cb, diff = (ca ^ c0) | (cb ^ c0);
                for (uint32_t l = cl + 128; l < U; l += 64) {
                    const uint32_t c = count_at(rr * U + l);
                    any |= c;
                    diff |= c ^ c0;
                }
                const bool a = __ballot(any != 0) != 0, v = __ballot(diff != 0) != 0;
                if (cl == i) my_res = c0 | ((a ? KEY_ANY : 0u) | (v ? KEY_VARIES : 0u)) << 30;
            }
        }
        if (my_rr < nrow) s_rr[my_rr] = my_res >> 30;
        __syncthreads();
        KF_FINE(fine(7);)
        const uint64_t ta = A.prof ? wall_clock64() : 0;
        // a varying row's slot in the chunk's share of the compact lists: the varying rows before it
        // (a prefix over the rows' flags, 64 rows a ballot)
        uint32_t slot = 0, nvar = 0;
        for (uint32_t r0 = 0; r0 < nrow; r0 += 64) {
            const uint64_t m = __ballot(r0 + cl < nrow && (s_rr[min(r0 + cl, nrow - 1)] & KEY_VARIES));
            if ((my_rr >> 6) == (r0 >> 6)) slot = nvar + (uint32_t)__popcll(m & ((1ull << (my_rr & 63u)) - 1ull));
            nvar += (uint32_t)__popcll(m);
        }
        // the share: both totals in one atomic instruction (lane 0 the keys, lane 1 the counts), issued
        // in front of the rows' key_first / key_flags stores, so its wait does not drain them
        unsigned long long got = 0;
        if (nvar && ct < 2) got = atomicAdd(A.var_tot + ct, ct ? (unsigned long long)nvar * U : (unsigned long long)nvar);
        if (my_rr < nrow) {
            A.key_first[ko + my_j] = my_res & 0x3FFFFFFFu;
            A.key_flags[ko + my_j] = (uint8_t)(my_res >> 30);
        }
        if (nvar == 0) continue;
        if (ct < 2) s_vb[ct] = got;
        __syncthreads();
        KF_FINE(fine(8);)
        if (A.prof) t_atomics += wall_clock64() - ta;  // (slots, the atomic, the rows' stores, the barrier)
        // the varying rows: their keys by the lanes that hold them, one store; their counts row by
        // row, the next row's first two reads issued before this row's are stored
        auto uni64 = [](unsigned long long v) -> uint64_t {  // (the same in every lane: scalar registers)
            return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
                   (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32;
        };
        const uint64_t vbase = uni64(s_vb[0]), obase = uni64(s_vb[1]);
        const uint64_t my_off = obase + (uint64_t)slot * U;
        // (a row past the lists' capacity is left out: the host grows the lists and reruns)
        const bool my_put = my_rr < nrow && ((my_res >> 30) & KEY_VARIES) && vbase + slot < A.var_keys_cap &&
                            my_off + U <= A.var_cap;
        if (my_put) A.var_keys[vbase + slot] = DevVarKey{r, my_j, my_off};
        uint64_t vm = __ballot(my_put);
        if (vm) {
            const uint32_t la = min(cl, U - 1), lb = min(cl + 64, U - 1);
            uint32_t nx = (wv + (uint32_t)__builtin_ctzll(vm) * kFWaves) * U;
            uint32_t na = count_at(nx + la), nb = count_at(nx + lb);
            while (vm) {
                const int i = __builtin_ctzll(vm);
                vm &= vm - 1;
                const uint32_t ca = na, cb = nb, x0 = nx;
                if (vm) {
                    nx = (wv + (uint32_t)__builtin_ctzll(vm) * kFWaves) * U;
                    na = count_at(nx + la), nb = count_at(nx + lb);
                }
                const uint64_t off = obase + (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)slot, i) * U;
                if (cl < U) A.var_counts[off + cl] = ca;
                if (cl + 64 < U) A.var_counts[off + cl + 64] = cb;
                for (uint32_t l = cl + 128; l < U; l += 64) A.var_counts[off + l] = count_at(x0 + l);
            }
        }
        KF_FINE(fine(9);)
    }
    }
    };
    if (in_lds && h16) chunks(KfTyped{});
    else chunks(KfAny{});
    stamp(6, wall_clock64());
    stamp(7, t_atomics);
    KF_FINE(for (uint32_t k = 0; k < kKfProfFineN; k++) stamp(kKfProfFine + k, tf[k]);)
    stamp(8, U);
    stamp(9, n_ent);
    stamp(10, nD);
    stamp(11, ncor);
    stamp(12, T);
    stamp(13, (T + rows_per - 1) / rows_per);
    stamp(14, blockIdx.x | (which << 24));  // (the workgroup: its timeline in the report)
    stamp(15, nref);
    trace(pw);
    };
    // regions [first, first + count) in A.order's order (most haplotypes first): with
    // A.persist a grid of a few workgroups per CU takes them -- its first region by
    // workgroup index, the next ones from the counter A.next[which] (gridDim.x + ticket),
    // the ticket for the next region taken as this one starts (the order entry's load behind it
    // waits for it: TFBS_KF_PROF's word 20) --, else one per workgroup.  A grid with one
    // workgroup per region takes no ticket (1 000 tickets at once cost microseconds).
    __shared__ uint32_t s_tk;
    const bool tickets = A.persist && gridDim.x < count;
    uint32_t i = blockIdx.x;
    while (i < count) {
        uint32_t tk = 0;
        uint64_t t_ticket = A.prof ? wall_clock64() : 0;
        if (tickets && tid == 0) tk = gridDim.x + atomicAdd(A.next + which, 1u);
        const uint32_t r = A.order ? A.order[first + i] : first + i;
        if (A.prof) {
            asm volatile("" ::"v"(r));  // (the entry has arrived)
            t_ticket = wall_clock64() - t_ticket;
        }
        process(r, i == blockIdx.x ? 0u : (uint32_t)TFBS_PATH_TICKET, t_ticket);
        if (!tickets) break;
        if (tid == 0) s_tk = tk;
        __syncthreads();
        i = s_tk;
        __syncthreads();
    }
    // (here, every region's registers dead: at the kernel's start this one line cost the small
    // shape 18 VGPRs and a wave of occupancy)
    if (A.report_fast && blockIdx.x == 0 && tid < 2) A.report[tid] = A.report_src ? A.report_src[tid] : 0u;
}

// Spill bucketing: per-region record counts, their exclusive scan (one
// workgroup), and the scatter into region order.
__global__ __launch_bounds__(256) void spill_hist_kernel(const uint32_t *__restrict__ over, uint32_t cap,
                                                          const uint32_t *__restrict__ spill, uint32_t *__restrict__ bcnt) {
    const uint32_t n = min(over[0], cap);
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256)
        atomicAdd(&bcnt[spill[3 * (size_t)e] & 0x7FFFFFFFu], 1u);
}

__global__ __launch_bounds__(1024) void spill_scan_kernel(const uint32_t *__restrict__ over, uint32_t *__restrict__ bcnt,
                                                          uint32_t n, uint32_t *__restrict__ boff) {
    __shared__ uint32_t s[1024];
    if (over[0] == 0) return;  // no records: the readers skip the buckets (AsmArgs::spill_count)
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < n ? bcnt[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
            const uint32_t t = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) {
            boff[i] = carry + s[threadIdx.x] - v;
            bcnt[i] = 0;  // the scatter's fill counters
        }
        carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) boff[n] = carry;
}

__global__ __launch_bounds__(256) void spill_scatter_kernel(const uint32_t *__restrict__ over, uint32_t cap,
                                                            const uint32_t *__restrict__ spill,
                                                            const uint32_t *__restrict__ boff,
                                                            uint32_t *__restrict__ bfill, uint32_t *__restrict__ out) {
    const uint32_t n = min(over[0], cap);
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const uint32_t r = spill[3 * (size_t)e] & 0x7FFFFFFFu;
        const uint32_t at = boff[r] + atomicAdd(&bfill[r], 1u);
        out[3 * (size_t)at] = spill[3 * (size_t)e];
        out[3 * (size_t)at + 1] = spill[3 * (size_t)e + 1];
        out[3 * (size_t)at + 2] = spill[3 * (size_t)e + 2];
    }
}

// A region's distinct (left, right) haplotype pairs: sample s carries distinct
// haplotypes (a, b) = (memb[2 s], memb[2 s + 1]) of its u16 membership row.  The
// pairs (key a | b << 16) go into an LDS hash table with their sample counts
// (one insert per wave for the lanes sharing lane 0's pair, which is most of
// them: the reference group on both sides), are listed at r * kEncMaxPairs of
// pab / pcnt in table order, and each sample gets its pair's index in pidx.
// More than kEncMaxPairs pairs: pair_n[r] = UINT32_MAX (the host path).
constexpr int kPairBlock = 512;
constexpr uint32_t kPairSlots = 2 * kEncMaxPairs;
constexpr uint32_t kPairEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t pair_slot(uint32_t key) { return (key * 0x9E3779B1u) >> (32 - 14); }
static_assert(kPairSlots == 1u << 14, "pair_slot hashes into 2^14 slots");

__global__ __launch_bounds__(kPairBlock) void pair_table_kernel(const uint64_t *__restrict__ rows, uint32_t n_samples,
                                                                uint32_t *__restrict__ pab, uint32_t *__restrict__ pcnt,
                                                                uint32_t *__restrict__ pair_n,
                                                                uint16_t *__restrict__ pidx) {
    __shared__ uint32_t s_key[kPairSlots];
    __shared__ uint32_t s_val[kPairSlots];  // sample counts, then the pairs' indices
    __shared__ uint32_t s_n, s_over, s_pos;
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const uint16_t *m = reinterpret_cast<const uint16_t *>(rows[r]);
    if (!m) {
        if (tid == 0) pair_n[r] = kPairEmpty;
        return;
    }
    for (uint32_t t = tid; t < kPairSlots; t += kPairBlock) {
        s_key[t] = kPairEmpty;
        s_val[t] = 0;
    }
    if (tid == 0) {
        s_n = 0;
        s_over = 0;
        s_pos = 0;
    }
    __syncthreads();
    auto insert = [&](uint32_t key, uint32_t add) {
        uint32_t sl = pair_slot(key);
        while (!*(volatile uint32_t *)&s_over) {
            const uint32_t old = atomicCAS(&s_key[sl], kPairEmpty, key);
            if (old == kPairEmpty && atomicAdd(&s_n, 1u) >= kEncMaxPairs) atomicOr(&s_over, 1u);
            if (old == kPairEmpty || old == key) {
                atomicAdd(&s_val[sl], add);
                return;
            }
            sl = (sl + 1) & (kPairSlots - 1);
        }
    };
    for (uint32_t s0 = 0; s0 < n_samples; s0 += kPairBlock) {
        const uint32_t s = s0 + tid;
        const bool valid = s < n_samples;
        const uint32_t key = valid ? (uint32_t)m[2 * s] | ((uint32_t)m[2 * s + 1] << 16) : kPairEmpty;
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
        const unsigned long long same = __ballot(valid && key == k0);
        if (valid && key == k0) {
            if (lane == (uint32_t)__builtin_ctzll(same)) insert(k0, (uint32_t)__popcll(same));
        } else if (valid) {
            insert(key, 1u);
        }
    }
    __syncthreads();
    if (s_over) {
        if (tid == 0) pair_n[r] = kPairEmpty;
        return;
    }
    const size_t p0 = (size_t)r * kEncMaxPairs;
    for (uint32_t t = tid; t < kPairSlots; t += kPairBlock)
        if (s_key[t] != kPairEmpty) {
            const uint32_t i = atomicAdd(&s_pos, 1u);
            pab[p0 + i] = s_key[t];
            pcnt[p0 + i] = s_val[t];
            s_val[t] = i;
        }
    __syncthreads();
    uint16_t *out = pidx + (size_t)r * n_samples;
    for (uint32_t s = tid; s < n_samples; s += kPairBlock) {
        const uint32_t key = (uint32_t)m[2 * s] | ((uint32_t)m[2 * s + 1] << 16);
        uint32_t sl = pair_slot(key);
        while (s_key[sl] != key) sl = (sl + 1) & (kPairSlots - 1);
        out[s] = (uint16_t)s_val[sl];
    }
    if (tid == 0) pair_n[r] = s_n;
}

// counts_as_genotypes' per-sample half (main.rs:439-498) for one varying key.
// A sample's total is C[a] + C[b] for its two haplotypes' distinct indices (a,
// b); pair_table_kernel lists each region's distinct (a, b) pairs with their
// sample counts and gives every sample its pair index, so the key's totals, min
// / max, distinct values (a bitmap of hi - lo + 1 bits), their ranks and sample
// counts are computed over the P pairs, not the N samples (no per-sample
// atomics); the one per-sample pass packs code[pair[s]].  The range
// multiplicity and the text stay on the host, which formats a row from the
// value table and the codes (aggregate.cpp).
constexpr int kEncBlock = 256;
constexpr uint32_t kEncWords = kEncMaxRange / 32;
constexpr uint32_t kEncWordsPerThread = kEncWords / kEncBlock;  // the rank scan's share of the bitmap

__global__ __launch_bounds__(kEncBlock) void key_encode_kernel(const uint32_t *__restrict__ var_counts,
                                                                 const DevVarKey *__restrict__ keys,
                                                                 const uint32_t *__restrict__ pab,
                                                                 const uint32_t *__restrict__ pcnt,
                                                                 const uint32_t *__restrict__ pair_n,
                                                                 const uint16_t *__restrict__ pidx, uint32_t region0,
                                                                 uint32_t n_samples, EncHdr *__restrict__ hdr,
                                                                 uint32_t *__restrict__ vals,
                                                                 uint32_t *__restrict__ hist,
                                                                 uint8_t *__restrict__ codes) {
    __shared__ uint32_t s_v[kEncMaxPairs];   // the pairs' totals, then their codes
    __shared__ uint32_t s_bits[kEncWords];
    __shared__ uint16_t s_rank[kEncWords];   // distinct values in the words before
    __shared__ uint32_t s_hist[kEncMaxVals + 1];
    __shared__ uint32_t s_red[2 * kEncBlock / 64];
    __shared__ uint32_t s_tsum[kEncBlock];
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const DevVarKey vk = keys[k];
    const uint32_t r = vk.region - region0;
    const size_t p0 = (size_t)r * kEncMaxPairs;
    const uint32_t P = pair_n[r];
    // each pair's total (u32 wrapping, as the reference's additions) from the key's
    // distinct-haplotype counts (a region's U counts, cache-resident); the host
    // sends only keys of regions with <= kEncMaxPairs pairs
    const uint32_t *cnt = var_counts + vk.out_off;
    uint32_t lo = UINT32_MAX, hi = 0;
    {
        for (uint32_t p = tid; p < P; p += kEncBlock) {
            const uint32_t ab = pab[p0 + p];
            const uint32_t v = cnt[ab & 0xFFFFu] + cnt[ab >> 16];
            s_v[p] = v;
            if (pcnt[p0 + p] == 0) continue;  // the reference group's pair when every sample carries a variant
            lo = min(lo, v);
            hi = max(hi, v);
        }
    }
    for (int o = 32; o; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    }
    const uint32_t wave = tid >> 6;
    if ((tid & 63) == 0) {
        s_red[wave] = lo;
        s_red[kEncBlock / 64 + wave] = hi;
    }
    for (uint32_t w = tid; w < kEncWords; w += kEncBlock) s_bits[w] = 0;
    for (uint32_t i = tid; i <= kEncMaxVals; i += kEncBlock) s_hist[i] = 0;
    __syncthreads();
    lo = s_red[0];
    hi = s_red[kEncBlock / 64];
    for (int w = 1; w < kEncBlock / 64; w++) {
        lo = min(lo, s_red[w]);
        hi = max(hi, s_red[kEncBlock / 64 + w]);
    }
    if (hi - lo >= kEncMaxRange) {
        if (tid == 0) hdr[k] = EncHdr{lo, hi, 0, 1, 0};
        return;
    }
    // which totals occur: one bit per pair (P LDS ORs, not N)
    for (uint32_t p = tid; p < P; p += kEncBlock) {
        if (pcnt[p0 + p] == 0) continue;
        const uint32_t d = s_v[p] - lo;
        atomicOr(&s_bits[d >> 5], 1u << (d & 31));
    }
    __syncthreads();
    // ranks: each thread's words summed, a block scan of the sums, the words' prefixes
    const uint32_t nw = (hi - lo) / 32 + 1;
    uint32_t mine = 0;
    for (uint32_t q = 0; q < kEncWordsPerThread; q++) {
        const uint32_t w = tid * kEncWordsPerThread + q;
        if (w < nw) mine += __popc(s_bits[w]);
    }
    s_tsum[tid] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < kEncBlock; o <<= 1) {
        const uint32_t t = tid >= o ? s_tsum[tid - o] : 0;
        __syncthreads();
        s_tsum[tid] += t;
        __syncthreads();
    }
    {
        uint32_t run = s_tsum[tid] - mine;
        for (uint32_t q = 0; q < kEncWordsPerThread; q++) {
            const uint32_t w = tid * kEncWordsPerThread + q;
            if (w < nw) {
                s_rank[w] = (uint16_t)min(run, 0xFFFFu);
                run += __popc(s_bits[w]);
            }
        }
    }
    const uint32_t nv = s_tsum[kEncBlock - 1];
    __syncthreads();
    if (nv > kEncMaxVals) {
        if (tid == 0) hdr[k] = EncHdr{lo, hi, nv, 1, 0};
        return;
    }
    for (uint32_t w = tid; w < nw; w += kEncBlock) {  // the sorted value table
        uint32_t b = s_bits[w], rk = s_rank[w];
        while (b) {
            const uint32_t t = __ffs(b) - 1;
            b &= b - 1;
            vals[(size_t)k * (kEncMaxVals + 1) + rk++] = lo + 32 * w + t;
        }
    }
    // each pair's code and its samples into the histogram (P LDS adds)
    for (uint32_t p = tid; p < P; p += kEncBlock) {
        const uint32_t n = pcnt[p0 + p];
        if (n == 0) {  // no sample has this pair: no code (its total may lie outside [lo, hi])
            s_v[p] = 0;
            continue;
        }
        const uint32_t d = s_v[p] - lo, w = d >> 5;
        const uint32_t c = s_rank[w] + __popc(s_bits[w] & ((1u << (d & 31)) - 1u));
        s_v[p] = c;
        atomicAdd(&s_hist[c], n);
    }
    __syncthreads();
    // the per-sample pass: code[pair[s]] packed (each thread writes whole bytes)
    const uint32_t width = nv <= 4 ? 2 : (nv <= 16 ? 4 : 8), per = 8 / width;
    uint8_t *out = codes + (size_t)k * n_samples;
    const uint16_t *pi = pidx + (size_t)r * n_samples;
    const uint32_t nbytes = (n_samples + per - 1) / per;
    for (uint32_t byte = tid; byte < nbytes; byte += kEncBlock) {
        uint32_t packed = 0;
        for (uint32_t q = 0; q < per; q++) {
            const uint32_t smp = byte * per + q;
            if (smp >= n_samples) break;
            packed |= s_v[pi[smp]] << (q * width);
        }
        out[byte] = (uint8_t)packed;
    }
    for (uint32_t i = tid; i < nv; i += kEncBlock) hist[(size_t)k * (kEncMaxVals + 1) + i] = s_hist[i];
    if (tid == 0) hdr[k] = EncHdr{lo, hi, nv, 0, width};
}

// Membership rows of host-built regions from their non-reference lists: row k
// (Hp u16 at k * Hp) is the region's reference group everywhere (meta[2k + 1]),
// then its entries [meta[2k], meta[2k + 2]) of ids / loc scattered over it.
__global__ __launch_bounds__(256) void memb_fill_kernel(const uint32_t *__restrict__ meta, const uint32_t *__restrict__ ids,
                                                        const uint16_t *__restrict__ loc, uint32_t Hp,
                                                        uint16_t *__restrict__ memb) {
    const uint32_t k = blockIdx.x;
    const uint32_t o0 = meta[2 * k], o1 = meta[2 * k + 2], ref = meta[2 * k + 1] & 0xFFFFu;
    uint16_t *row = memb + (size_t)k * Hp;
    const uint32_t v = ref | (ref << 16);
    for (uint32_t i = threadIdx.x; i < Hp / 8; i += 256) reinterpret_cast<uint4 *>(row)[i] = uint4{v, v, v, v};
    __syncthreads();
    for (uint32_t i = o0 + threadIdx.x; i < o1; i += 256) row[ids[i]] = loc[i];
}

// Copies each key's packed codes (at k * n_samples) to off[k] of a contiguous buffer.
__global__ __launch_bounds__(256) void code_compact_kernel(const uint8_t *__restrict__ codes, uint32_t n_samples,
                                                           const uint64_t *__restrict__ off, uint8_t *__restrict__ dst) {
    const uint32_t k = blockIdx.x;
    const uint64_t o = off[k], n = off[k + 1] - o;
    const uint8_t *src = codes + (size_t)k * n_samples;
    for (uint64_t i = threadIdx.x; i < n; i += 256) dst[o + i] = src[i];
}

// Each key's n_vals value-table entries and histogram counts (of kEncMaxVals + 1
// slots) back to back at off[k].
__global__ __launch_bounds__(64) void val_compact_kernel(const uint32_t *__restrict__ vals,
                                                         const uint32_t *__restrict__ hist,
                                                         const uint32_t *__restrict__ off, uint32_t *__restrict__ ov,
                                                         uint32_t *__restrict__ oh) {
    const uint32_t k = blockIdx.x, o = off[k], n = off[k + 1] - o;
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        ov[o + i] = vals[(size_t)k * (kEncMaxVals + 1) + i];
        oh[o + i] = hist[(size_t)k * (kEncMaxVals + 1) + i];
    }
}

}  // namespace

int launch_val_compact(const uint32_t *vals, const uint32_t *hist, uint32_t n_keys, const uint32_t *off, uint32_t *ov,
                       uint32_t *oh, hipStream_t stream) {
    if (n_keys == 0) return TFBS_OK;
    hipLaunchKernelGGL(val_compact_kernel, dim3(n_keys), dim3(64), 0, stream, vals, hist, off, ov, oh);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("val_compact_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_memb_fill(const uint32_t *meta, const uint32_t *ids, const uint16_t *loc, uint32_t n_rows, uint32_t Hp,
                     uint16_t *memb, hipStream_t stream) {
    if (n_rows == 0) return TFBS_OK;
    hipLaunchKernelGGL(memb_fill_kernel, dim3(n_rows), dim3(256), 0, stream, meta, ids, loc, Hp, memb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("memb_fill_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_pair_table(const uint64_t *rows, uint32_t n_regions, uint32_t n_samples, uint32_t *pab, uint32_t *pcnt,
                      uint32_t *pair_n, uint16_t *pidx, hipStream_t stream) {
    if (n_regions == 0) return TFBS_OK;
    hipLaunchKernelGGL(pair_table_kernel, dim3(n_regions), dim3(kPairBlock), 0, stream, rows, n_samples, pab, pcnt,
                       pair_n, pidx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("pair_table_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_key_encode(const uint32_t *var_counts, const DevVarKey *keys, uint32_t n_keys, const uint32_t *pab,
                      const uint32_t *pcnt, const uint32_t *pair_n, const uint16_t *pidx, uint32_t region0,
                      uint32_t n_samples, EncHdr *hdr, uint32_t *vals, uint32_t *hist, uint8_t *codes,
                      hipStream_t stream) {
    if (n_keys == 0) return TFBS_OK;
    hipLaunchKernelGGL(key_encode_kernel, dim3(n_keys), dim3(kEncBlock), 0, stream, var_counts, keys, pab, pcnt,
                       pair_n, pidx, region0, n_samples, hdr, vals, hist, codes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("key_encode_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_code_compact(const uint8_t *codes, uint32_t n_keys, uint32_t n_samples, const uint64_t *off, uint8_t *dst,
                        hipStream_t stream) {
    if (n_keys == 0) return TFBS_OK;
    hipLaunchKernelGGL(code_compact_kernel, dim3(n_keys), dim3(256), 0, stream, codes, n_samples, off, dst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("code_compact_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_spill_buckets(const uint32_t *over, uint32_t cap, const uint32_t *spill, uint32_t n_regions, uint32_t *bcnt,
                         uint32_t *boff, uint32_t *sorted, hipStream_t stream, bool bcnt_zeroed) {
    hipError_t e = bcnt_zeroed ? hipSuccess : hipMemsetAsync(bcnt, 0, (size_t)(n_regions + 1) * 4, stream);
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("spill bucket memset: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(spill_hist_kernel, dim3(64), dim3(256), 0, stream, over, cap, spill, bcnt);
    hipLaunchKernelGGL(spill_scan_kernel, dim3(1), dim3(1024), 0, stream, over, bcnt, n_regions, boff);
    hipLaunchKernelGGL(spill_scatter_kernel, dim3(64), dim3(256), 0, stream, over, cap, spill, boff, bcnt, sorted);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("spill bucket kernels: ") + hipGetErrorString(e));
    return TFBS_OK;
}

int launch_key_asm(const AsmArgs &a, uint32_t n_regions, hipStream_t stream) {
    if (n_regions == 0) return TFBS_OK;
    hipLaunchKernelGGL(key_asm_kernel, dim3(n_regions), dim3(kAsmBlock), 0, stream, a, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("key_asm_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

static size_t key_fast_lds_bytes(bool big) {
    hipFuncAttributes fa{};
    const hipError_t e = big ? hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(key_fast_kernel<KfBig>))
                             : hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(key_fast_kernel<KfSmall>));
    return e == hipSuccess ? fa.sharedSizeBytes : 0;
}

int launch_key_fast(const AsmArgs &a, uint32_t n_regions, uint32_t n_big, hipStream_t stream, hipStream_t side,
                    hipEvent_t fork, hipEvent_t join, bool leftover) {
    if (n_regions == 0) return TFBS_OK;
    if (!a.order || !side) n_big = 0;
    n_big = std::min(n_big, n_regions);
    // persistent grids (a.persist): the workgroups of each shape that fit the device at
    // once, queried once per device (the calling thread's current device: the ctx's),
    // thread-safe for contexts on several threads
    struct Fit {
        int n_cu = 256, per_small = 2, per_big = 1;
    };
    constexpr int kMaxDev = 64;
    static std::once_flag once[kMaxDev];
    static Fit fits[kMaxDev];
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev = std::min(std::max(dev, 0), kMaxDev - 1);
    std::call_once(once[dev], [dev] {
        Fit &f = fits[dev];
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) f.n_cu = v;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, key_fast_kernel<KfSmall>, KfSmall::kBlock, 0) ==
                hipSuccess && v > 0)
            f.per_small = v;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, key_fast_kernel<KfBig>, KfBig::kBlock, 0) == hipSuccess &&
            v > 0)
            f.per_big = v;
        (void)hipGetLastError();
        if (getenv("TFBS_KF_PROF"))
            fprintf(stderr, "[kf prof] device %d: CUs %d, workgroups per CU: %d (%d threads, %zu B LDS), %d (%d threads, %zu B LDS)\n",
                    dev, f.n_cu, f.per_small, KfSmall::kBlock, key_fast_lds_bytes(false), f.per_big, KfBig::kBlock,
                    key_fast_lds_bytes(true));
    });
    const Fit &fit = fits[dev];
    const int n_cu = fit.n_cu, per_small = fit.per_small, per_big = fit.per_big;
    auto grid = [&](uint32_t n, int per) {  // (a.grid_cap: TFBS_KF_GRID, so that a few regions take tickets)
        const uint32_t fit_wg = (uint32_t)(n_cu * per);
        return a.persist ? std::min<uint32_t>(n, a.grid_cap ? std::min(a.grid_cap, fit_wg) : fit_wg) : n;
    };
    hipError_t e = hipSuccess;
    // two shapes at once: the regions of many haplotypes (order[0, n_big), whole-CU
    // workgroups) go first on `stream` -- queued ahead, they take their CUs before the
    // others fill every CU -- and the rest on `side`, forked before and joined after
    const bool two = n_big && n_regions > n_big;
    if (two) {
        if ((e = hipEventRecord(fork, stream)) == hipSuccess) e = hipStreamWaitEvent(side, fork, 0);
        if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("key_fast_kernel fork: ") + hipGetErrorString(e));
    }
    if (n_big)
        hipLaunchKernelGGL(key_fast_kernel<KfBig>, dim3(grid(n_big, per_big)), dim3(KfBig::kBlock), 0, stream, a, 0u,
                           n_big, 1u);
    if (n_regions > n_big)
        hipLaunchKernelGGL(key_fast_kernel<KfSmall>, dim3(grid(n_regions - n_big, per_small)), dim3(KfSmall::kBlock), 0,
                           two ? side : stream, a, n_big, n_regions - n_big, 0u);
    if (two) {
        if ((e = hipEventRecord(join, side)) == hipSuccess) e = hipStreamWaitEvent(stream, join, 0);
        if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("key_fast_kernel join: ") + hipGetErrorString(e));
    }
    // the regions it left: a fixed grid over the list (no host round trip)
    if (leftover)
        hipLaunchKernelGGL(key_asm_kernel, dim3(std::min<uint32_t>(n_regions, 256)), dim3(kAsmBlock), 0, stream, a,
                           (const uint32_t *)a.redo, (const uint32_t *)a.redo_n);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("key_fast_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

__global__ void asm_report_kernel(const uint32_t *__restrict__ over, uint32_t *__restrict__ ctr) {
    if (threadIdx.x < 2) ctr[threadIdx.x] = over ? over[threadIdx.x] : 0u;
}

int launch_asm_report(const uint32_t *over, uint32_t *ctr, hipStream_t stream) {
    hipLaunchKernelGGL(asm_report_kernel, dim3(1), dim3(64), 0, stream, over, ctr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFBS_E_HIP, std::string("asm_report_kernel: ") + hipGetErrorString(e));
    return TFBS_OK;
}

uint32_t key_asm_lds_counters() { return kAsmCounters; }
uint32_t key_fast_big_u() { return kFBigU; }

}  // namespace tfbs
