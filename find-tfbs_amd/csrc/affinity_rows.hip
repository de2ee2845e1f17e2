// MI355X (gfx950) affinity rows (include/tfbs_amd.h, "Affinity rows"): a second VCF whose
// per-sample value is mlog2 of the sum of the two haplotypes' binding affinities of a pattern id
// inside an inner range, mlog2(x) = floor(1000 * log2(x)) in exact integers.
//
// The frame is the score rows' (row_frame.hpp): the chunks of whole regions, the pair tables, the
// candidate rows, the tokens, the host's selection, the text kernel and the fallback.  This file
// keeps the affinity kind:
//  * scan_affinity_kernel (scan_affinity.hip, through affinity_launch_chunk) writes its 16-byte
//    records, which stay on the device.
//  * affinity_fold_kernel, one thread per (range, pattern id, distinct haplotype), reads the id's
//    strands' records where they lie (hap_off[h] + strand * n_ranges + range) and writes
//    A = the sum of their sums (u64; below 2^63 by the affinity call's refusal) and a none byte
//    (N = the sum of their windows == 0).
//  * affinity_stats_kernel, one workgroup per candidate row, stages the logarithm's table
//    (kAffLogP, 8 000 bytes) in LDS once, then works over the region's distinct (left, right)
//    pairs: pass 1 the pairs' u64 sums x, their minimum xlo, maximum xhi and the none test;
//    lo = mlog2(xlo), hi = mlog2(xhi) (mlog2 is monotone); pass 2 each pair's y = mlog2(x) -- ten
//    LDS reads of a binary search --, d = y - lo, its token (row_token), the three counts and the
//    text length weighted by the pairs' sample counts.  One header, which also carries xlo and
//    xhi, and a 4-byte token per pair: what score_text_kernel reads.
//  * affinity_mlog2_kernel runs the same device function on an array (tfbs_affinity_mlog2).
// A region whose pairs launch_pair_table does not list takes affinity_as_genotypes on the host
// from its folded values: the same text.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "affinity_log_table.hpp"
#include "affinity_rows.hpp"
#include "row_frame.hpp"

namespace tfbs {
namespace {

constexpr int kLogBlock = 256;

struct DevAffHdr {
    int64_t lo, hi;     // mlog2(xlo), mlog2(xhi)
    uint64_t text_len;  // of the genotype text
    uint32_t zero, one, two;
    uint32_t none;      // a carried haplotype without a value: no row
    uint64_t xlo, xhi;  // the exact minimum and maximum of the samples' sums
};

// Grid: (blocks over the region's values, the chunk's regions).
__global__ __launch_bounds__(kFoldBlock) void affinity_fold_kernel(const DevFoldRegion *__restrict__ regs,
                                                                   const uint64_t *__restrict__ hap_off,
                                                                   const DevAffRec *__restrict__ recs, uint64_t rec_cap,
                                                                   const uint32_t *__restrict__ pid_off,
                                                                   const uint32_t *__restrict__ pid_strand, uint32_t n_pids,
                                                                   uint64_t *__restrict__ vals, uint8_t *__restrict__ none) {
    const DevFoldRegion R = regs[blockIdx.y];
    const uint64_t n = (uint64_t)R.nr * n_pids * R.U;
    for (uint64_t i = (uint64_t)blockIdx.x * kFoldBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFoldBlock) {
        const uint32_t h = (uint32_t)(i % R.U);
        const uint32_t rq = (uint32_t)(i / R.U), q = rq % n_pids, range = rq / n_pids;
        const uint64_t base = hap_off[R.k0 + h] + range;
        uint64_t a = 0, nw = 0;
        for (uint32_t x = pid_off[q]; x < pid_off[q + 1]; x++) {  // integer adds: any order
            const uint64_t at = base + (uint64_t)pid_strand[x] * R.nr;
            if (at >= rec_cap) continue;
            const DevAffRec rec = recs[at];
            a += rec.sum;
            nw += rec.n_windows;
        }
        vals[R.val_off + i] = a;
        none[R.val_off + i] = nw ? 0 : 1;
    }
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) { return (uint64_t)__shfl_xor((long long)v, m); }

// Grid: one workgroup per candidate row.
__global__ __launch_bounds__(kStatBlock) void affinity_stats_kernel(const DevCand *__restrict__ cands,
                                                                    const uint64_t *__restrict__ vals,
                                                                    const uint8_t *__restrict__ none,
                                                                    const uint32_t *__restrict__ pab,
                                                                    const uint32_t *__restrict__ pcnt,
                                                                    const uint32_t *__restrict__ pair_n,
                                                                    const uint64_t *__restrict__ logp,
                                                                    DevAffHdr *__restrict__ hdr, uint32_t *__restrict__ toks) {
    __shared__ uint64_t s_p[kAffLogLen];
    __shared__ uint64_t s_lo[kStatBlock / 64], s_hi[kStatBlock / 64], s_len[kStatBlock / 64];
    __shared__ uint32_t s_cnt[kStatBlock / 64][4];
    const DevCand C = cands[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t P = pair_n[C.region];
    if (P == kNotListed || P > kEncMaxPairs) return;  // (the host takes such a region; its rows are not candidates here)
    for (uint32_t x = tid; x < kAffLogLen; x += kStatBlock) s_p[x] = logp[x];  // (the barrier below covers it)
    const uint32_t *ab = pab + (size_t)C.region * kEncMaxPairs, *cn = pcnt + (size_t)C.region * kEncMaxPairs;
    const uint64_t *v = vals + C.val_off;
    const uint8_t *nv = none + C.val_off;
    uint64_t xlo = UINT64_MAX, xhi = 0;
    uint32_t bad = 0;
    for (uint32_t i = tid; i < P; i += kStatBlock) {
        const uint32_t a = ab[i] & 0xFFFFu, b = ab[i] >> 16;
        if (a >= C.U || b >= C.U) {  // (a membership row names the region's haplotypes only)
            bad = 1;
            continue;
        }
        bad |= nv[a] | nv[b];
        const uint64_t x = v[a] + v[b];  // (each below 2^63: no wrap)
        xlo = x < xlo ? x : xlo;
        xhi = x > xhi ? x : xhi;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t ol = shfl_xor_u64(xlo, m), oh = shfl_xor_u64(xhi, m);
        xlo = ol < xlo ? ol : xlo;
        xhi = oh > xhi ? oh : xhi;
        bad |= (uint32_t)__shfl_xor((int)bad, m);
    }
    if (lane == 0) {
        s_lo[wave] = xlo;
        s_hi[wave] = xhi;
        s_cnt[wave][3] = bad;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kStatBlock / 64; w++) {
        xlo = s_lo[w] < xlo ? s_lo[w] : xlo;
        xhi = s_hi[w] > xhi ? s_hi[w] : xhi;
        bad |= s_cnt[w][3];
    }
    if (bad || P == 0) {  // (uniform over the workgroup)
        if (tid == 0) hdr[blockIdx.x] = DevAffHdr{0, 0, 0, 0, 0, 0, bad ? 1u : 0u, 0, 0};
        return;
    }
    const int64_t lo = affinity_mlog2(xlo, s_p), hi = affinity_mlog2(xhi, s_p);
    if (hi == lo) {
        if (tid == 0) hdr[blockIdx.x] = DevAffHdr{lo, hi, 0, 0, 0, 0, 0, xlo, xhi};
        return;
    }
    const uint64_t spread = (uint64_t)(hi - lo);  // (at most 64000)
    uint32_t cnt[3] = {0, 0, 0};
    uint64_t len = 0;
    for (uint32_t i = tid; i < P; i += kStatBlock) {
        const uint32_t a = ab[i] & 0xFFFFu, b = ab[i] >> 16, w = cn[i];
        const uint64_t d = (uint64_t)((int64_t)affinity_mlog2(v[a] + v[b], s_p) - lo);
        toks[C.tok_off + i] = row_token(d, spread, w, cnt, len);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        len += shfl_xor_u64(len, m);
#pragma unroll
        for (int k = 0; k < 3; k++) cnt[k] += (uint32_t)__shfl_xor((int)cnt[k], m);
    }
    __syncthreads();  // (s_cnt[.][3] has been read)
    if (lane == 0) {
        s_len[wave] = len;
        for (int k = 0; k < 3; k++) s_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (tid == 0) {
        DevAffHdr h{lo, hi, 0, 0, 0, 0, 0, xlo, xhi};
        for (int w = 0; w < kStatBlock / 64; w++) {
            h.text_len += s_len[w];
            h.zero += s_cnt[w][0];
            h.one += s_cnt[w][1];
            h.two += s_cnt[w][2];
        }
        hdr[blockIdx.x] = h;
    }
}

// Grid: blocks over the array (a grid-stride loop).
__global__ __launch_bounds__(kLogBlock) void affinity_mlog2_kernel(const uint64_t *__restrict__ x, uint64_t n,
                                                                   const uint64_t *__restrict__ logp,
                                                                   int32_t *__restrict__ out) {
    __shared__ uint64_t s_p[kAffLogLen];
    for (uint32_t k = threadIdx.x; k < kAffLogLen; k += kLogBlock) s_p[k] = logp[k];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kLogBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kLogBlock)
        out[i] = affinity_mlog2(x[i], s_p);
}

int put_log_table(DevBuf<uint64_t> &b, hipStream_t stream) {
    if (int rc = b.ensure_exact(kAffLogLen)) return rc;
    HIP_TRY(hipMemcpyAsync(b.p, kAffLogP, sizeof kAffLogP, hipMemcpyHostToDevice, stream));
    return TFBS_OK;
}

}  // namespace

// The affinity kind's own: the logarithm's table, the values, the headers, the tops and the timers.
struct AffinityRowsState {
    DevBuf<uint64_t> logp, vals;
    DevBuf<DevAffHdr> hdr;
    std::vector<int32_t> tops;  // per strand (affinity_tops)
    double ms[4] = {0, 0, 0, 0};
};

void affinity_rows_state_destroy(AffinityRowsState *s) { delete s; }

void affinity_rows_last_ms(const AffinityRowsState *s, double out[4]) {
    for (int k = 0; k < 4; k++) out[k] = s ? s->ms[k] : 0.0;
}

namespace {

struct AffinityKind {  // rows_run's kind (row_frame.hpp)
    typedef DevAffRec Rec;
    typedef uint64_t Val;
    typedef DevAffHdr Hdr;
    static constexpr const char *scratch_env = "TFBS_AFFINITY_ROWS_SCRATCH_MB", *label = "affinity";
    AffinityRowsState &S;
    AffinityState *aff;
    const RowFrame &F;
    const Batch &B;
    int32_t top_of(uint32_t q) const { return S.tops[F.first_strand[q]]; }
    int region_check(size_t r, const RegionH &R) { return affinity_region_check(aff, B, r, R); }
    int launch_records(hipStream_t stream, const ScanImage &img, const uint32_t *ids, const uint64_t *hap_off, size_t nh,
                       uint64_t nrec, const uint64_t **d_hap_off, const Rec **recs, double *ms) {
        return affinity_launch_chunk(aff, stream, img, ids, hap_off, nh, nrec, d_hap_off, recs, ms);
    }
    DevBuf<Val> &vals() { return S.vals; }
    DevBuf<Hdr> &hdr() { return S.hdr; }
    void fold(dim3 grid, hipStream_t stream, RowFrame &f, const uint64_t *d_hap_off, const Rec *recs, uint64_t nrec,
              uint32_t npid) {
        hipLaunchKernelGGL(affinity_fold_kernel, grid, dim3(kFoldBlock), 0, stream, f.regs.p, d_hap_off, recs, nrec,
                           f.pid_off.p, f.pid_strand.p, npid, S.vals.p, f.none.p);
    }
    void stats(uint32_t n, hipStream_t stream, RowFrame &f) {
        hipLaunchKernelGGL(affinity_stats_kernel, dim3(n), dim3(kStatBlock), 0, stream, f.cands.p, S.vals.p, f.none.p,
                           f.pab.p, f.pcnt.p, f.pair_n.p, S.logp.p, S.hdr.p, f.toks.p);
    }
    bool pick(const Hdr &h, uint32_t q, uint64_t min_spread, uint32_t min_maf, std::string &info) {
        const uint64_t spread = (uint64_t)(h.hi - h.lo);
        if (h.none || spread == 0 || spread < min_spread) return false;
        if (maf_of(h.zero, h.one, h.two) < min_maf) return false;
        info = affinity_row_info(h.lo, h.hi, h.xlo, h.xhi, top_of(q), h.zero, h.one, h.two);
        return true;
    }
    bool host_row(const Val *left, const Val *right, size_t n, uint32_t q, uint64_t min_spread, uint32_t *maf,
                  std::string &info, std::string &gts) {
        return affinity_as_genotypes(left, right, n, top_of(q), min_spread, maf, info, gts);
    }
};

}  // namespace

int affinity_rows_run(AffinityRowsState **state, ScoresState **frame, AffinityState **aff, int device, void *stream_,
                      const Patterns &P, const ScanImage &img, const Batch &B, size_t r0, size_t r1,
                      const std::string &chrom, uint32_t min_maf, uint64_t min_spread, uint32_t *fake, std::string *out,
                      uint64_t *n_rows) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(device));
    *n_rows = 0;
    uint32_t n_strands = 0;
    int rc;
    // (the affinity tables first: a pattern set that affinity_tops refuses is refused before anything is made)
    if ((rc = affinity_prepare(aff, device, stream_, P, &n_strands)) || (rc = scores_state_ensure(frame, P, stream))) return rc;
    if (!*state) {
        AffinityRowsState *s = new AffinityRowsState();
        if ((rc = affinity_tops(P, &s->tops)) || (rc = put_log_table(s->logp, stream))) {
            delete s;
            return rc;
        }
        *state = s;
    }
    AffinityKind kind{**state, *aff, (*frame)->F, B};
    return rows_run((*frame)->F, kind, (*state)->ms, device, stream, n_strands, img, B, r0, r1, chrom, min_maf, min_spread,
                    fake, out, n_rows);
}

int affinity_mlog2_device(const uint64_t *x, size_t n, int device, int32_t *out) {
    if (n == 0) return TFBS_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint64_t> dx, logp;
    DevBuf<int32_t> dout;
    int rc;
    if ((rc = dx.ensure_exact(n)) || (rc = dout.ensure_exact(n)) || (rc = put_log_table(logp, nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(dx.p, x, 8 * n, hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(affinity_mlog2_kernel, dim3((uint32_t)std::min<uint64_t>((n + kLogBlock - 1) / kLogBlock, 4096)),
                       dim3(kLogBlock), 0, nullptr, dx.p, (uint64_t)n, logp.p, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, 4 * n, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return TFBS_OK;
}

}  // namespace tfbs
