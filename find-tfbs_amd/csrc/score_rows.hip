// MI355X (gfx950) score rows (include/tfbs_amd.h, "Score rows"): a second VCF whose per-sample
// value is the sum of the two haplotypes' best scores of a pattern id inside an inner range.
//
// A chunk of whole regions goes through four steps, the records never leaving the device:
//  * scan_best_kernel (scan_best.hip, through best_launch_chunk) writes its 16-byte records.
//  * score_fold_kernel reads them where they lie (hap_off[h] + strand * n_ranges + range) and
//    writes, per (range, pattern id, distinct haplotype), the value B -- the best over the
//    id's strands, ties to the strand earlier in creation order -- and a none flag.
//  * score_stats_kernel, one workgroup per candidate row (key, pattern id), works over the
//    region's distinct (left, right) pairs of launch_pair_table, not over the samples: the
//    pair sums in int64, lo / hi, the none test, then each pair's class and DS numerator t
//    (score_class, scores.hpp), the three counts and the text length weighted by the pairs'
//    sample counts.  It writes one header and a 4-byte token per pair.
//  * The host picks the rows from the headers (min_spread, min_maf), numbers them and formats
//    their heads; score_text_kernel, one workgroup per picked row, writes the genotype text:
//    a sample's field comes from its pair's token through pidx, its place from a prefix sum of
//    the field lengths over the tile (a wave scan, the waves' totals through LDS) carried from
//    tile to tile.  A tile's bytes are put together in LDS at the phase of their destination
//    (its address mod 16) and stored 16 bytes per lane (one dwordx4 vector store, a wave's
//    lanes on consecutive 16-byte pieces); the ragged first and last piece go as bytes.  Every
//    destination is known: no atomics.
// A region whose pairs launch_pair_table does not list (more than kEncMaxPairs pairs or more
// than kEncMaxHaps distinct haplotypes) takes scores_as_genotypes on the host from its folded
// values: the same text.
// The chunk and group loop, the pair tables, the candidate and picked rows and the fallback are
// row_frame.hpp's (rows_run), shared with the affinity rows (affinity_rows.hip), whose tokens
// score_text_kernel writes too (launch_row_text).  This file keeps the score kind and that kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "row_frame.hpp"

namespace tfbs {
namespace {

constexpr int kTextBlock = 512;  // samples per tile: one per thread

// Grid: (blocks over the region's values, the chunk's regions).
__global__ __launch_bounds__(kFoldBlock) void score_fold_kernel(const DevFoldRegion *__restrict__ regs,
                                                                const uint64_t *__restrict__ hap_off,
                                                                const DevBestRec *__restrict__ recs, uint64_t rec_cap,
                                                                const uint32_t *__restrict__ pid_off,
                                                                const uint32_t *__restrict__ pid_strand, uint32_t n_pids,
                                                                int32_t *__restrict__ vals, uint8_t *__restrict__ none) {
    const DevFoldRegion R = regs[blockIdx.y];
    const uint64_t n = (uint64_t)R.nr * n_pids * R.U;
    for (uint64_t i = (uint64_t)blockIdx.x * kFoldBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFoldBlock) {
        const uint32_t h = (uint32_t)(i % R.U);
        const uint32_t rq = (uint32_t)(i / R.U), q = rq % n_pids, range = rq / n_pids;
        const uint64_t base = hap_off[R.k0 + h] + range;
        int32_t v = 0;
        bool have = false;
        for (uint32_t x = pid_off[q]; x < pid_off[q + 1]; x++) {  // creation order: a tie keeps the earlier strand
            const uint64_t at = base + (uint64_t)pid_strand[x] * R.nr;
            if (at >= rec_cap) continue;
            const DevBestRec rec = recs[at];
            if (rec.n_windows && (!have || rec.score > v)) {
                v = rec.score;
                have = true;
            }
        }
        vals[R.val_off + i] = v;
        none[R.val_off + i] = have ? 0 : 1;
    }
}

__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int m) { return (int64_t)__shfl_xor((long long)v, m); }

// Grid: one workgroup per candidate row.
__global__ __launch_bounds__(kStatBlock) void score_stats_kernel(const DevCand *__restrict__ cands,
                                                                 const int32_t *__restrict__ vals,
                                                                 const uint8_t *__restrict__ none,
                                                                 const uint32_t *__restrict__ pab,
                                                                 const uint32_t *__restrict__ pcnt,
                                                                 const uint32_t *__restrict__ pair_n,
                                                                 DevScoreHdr *__restrict__ hdr, uint32_t *__restrict__ toks) {
    __shared__ int64_t s_lo[kStatBlock / 64], s_hi[kStatBlock / 64];
    __shared__ uint64_t s_len[kStatBlock / 64];
    __shared__ uint32_t s_cnt[kStatBlock / 64][4];
    const DevCand C = cands[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t P = pair_n[C.region];
    if (P == kNotListed || P > kEncMaxPairs) return;  // (the host takes such a region; its rows are not candidates here)
    const uint32_t *ab = pab + (size_t)C.region * kEncMaxPairs, *cn = pcnt + (size_t)C.region * kEncMaxPairs;
    const int32_t *v = vals + C.val_off;
    const uint8_t *nv = none + C.val_off;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    uint32_t bad = 0;
    for (uint32_t i = tid; i < P; i += kStatBlock) {
        const uint32_t a = ab[i] & 0xFFFFu, b = ab[i] >> 16;
        if (a >= C.U || b >= C.U) {  // (a membership row names the region's haplotypes only)
            bad = 1;
            continue;
        }
        bad |= nv[a] | nv[b];
        const int64_t x = (int64_t)v[a] + (int64_t)v[b];
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t ol = shfl_xor64(lo, m), oh = shfl_xor64(hi, m);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
        bad |= (uint32_t)__shfl_xor((int)bad, m);
    }
    if (lane == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
        s_cnt[wave][3] = bad;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kStatBlock / 64; w++) {
        lo = s_lo[w] < lo ? s_lo[w] : lo;
        hi = s_hi[w] > hi ? s_hi[w] : hi;
        bad |= s_cnt[w][3];
    }
    if (bad || P == 0 || hi == lo) {  // (uniform over the workgroup)
        if (tid == 0) hdr[blockIdx.x] = DevScoreHdr{P ? lo : 0, P ? hi : 0, 0, 0, 0, 0, bad ? 1u : 0u};
        return;
    }
    const uint64_t spread = (uint64_t)(hi - lo);
    uint32_t cnt[3] = {0, 0, 0};
    uint64_t len = 0;
    for (uint32_t i = tid; i < P; i += kStatBlock) {
        const uint32_t a = ab[i] & 0xFFFFu, b = ab[i] >> 16, w = cn[i];
        const uint64_t d = (uint64_t)((int64_t)v[a] + (int64_t)v[b] - lo);
        toks[C.tok_off + i] = row_token(d, spread, w, cnt, len);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        len += (uint64_t)__shfl_xor((long long)len, m);
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
        DevScoreHdr h{lo, hi, 0, 0, 0, 0, 0};
        for (int w = 0; w < kStatBlock / 64; w++) {
            h.text_len += s_len[w];
            h.zero += s_cnt[w][0];
            h.one += s_cnt[w][1];
            h.two += s_cnt[w][2];
        }
        hdr[blockIdx.x] = h;
    }
}

// Grid: one workgroup per picked row; its lanes are the tile's kTextBlock samples.
__global__ __launch_bounds__(kTextBlock) void score_text_kernel(const DevTextRow *__restrict__ rows,
                                                                const uint32_t *__restrict__ toks,
                                                                const uint16_t *__restrict__ pidx, uint32_t n_samples,
                                                                uint8_t *__restrict__ out, uint64_t out_cap) {
    __shared__ uint4 s_text[(kTextBlock * 11 + 15) / 16 + 1];  // a tile's bytes from phase 0-15
    __shared__ uint32_t s_wsum[kTextBlock / 64];
    uint8_t *const text = reinterpret_cast<uint8_t *>(s_text);
    const DevTextRow R = rows[blockIdx.x];
    const uint16_t *pi = pidx + (size_t)R.region * n_samples;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t at = R.out_off;  // the tile's first byte (uniform)
    for (uint32_t s0 = 0; s0 < n_samples; s0 += kTextBlock) {
        const uint32_t s = s0 + tid;
        const bool valid = s < n_samples;
        const uint32_t tok = valid ? toks[R.tok_off + pi[s]] : 0u;
        const bool ext = (tok & (kTokLo | kTokHi)) != 0;
        const uint32_t len = valid ? (ext ? 8u : 11u) : 0u;
        uint32_t incl = len;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, m);
            incl += lane >= (uint32_t)m ? o : 0u;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kTextBlock / 64; w++) {
            before += w < wave ? s_wsum[w] : 0u;
            total += s_wsum[w];
        }
        const uint32_t phase = (uint32_t)(at & 15);
        if (valid) {
            uint8_t *f = text + phase + before + incl - len;
            const uint32_t cls = (tok >> 16) & 3u, t = tok & 0x7FFFu;
            f[0] = '\t';
            f[1] = cls == 2 ? '1' : '0';
            f[2] = '|';
            f[3] = cls == 0 ? '0' : '1';
            f[4] = ':';
            f[6] = '.';
            if (ext) {
                f[1] = f[3] = (tok & kTokHi) ? '1' : '0';
                f[5] = (tok & kTokHi) ? '2' : '0';
                f[7] = '0';
            } else {
                const uint32_t frac = t % 10000u;
                f[5] = (uint8_t)('0' + t / 10000u);
                f[7] = (uint8_t)('0' + frac / 1000u);
                f[8] = (uint8_t)('0' + frac / 100u % 10u);
                f[9] = (uint8_t)('0' + frac / 10u % 10u);
                f[10] = (uint8_t)('0' + frac % 10u);
            }
        }
        __syncthreads();
        // LDS byte j goes to byte g0 + j of the text, g0 a multiple of 16 (as the text's base is)
        const uint64_t g0 = at - phase;
        const uint32_t end = phase + total, npc = (end + 15) / 16;
        for (uint32_t i = tid; i < npc; i += kTextBlock) {
            const uint32_t b0 = max(16 * i, phase), b1 = min(16 * i + 16, end);
            if (g0 + b1 > out_cap) continue;  // (the host sized the text from the headers' lengths)
            if (b1 - b0 == 16) {
                *reinterpret_cast<uint4 *>(out + g0 + 16 * i) = s_text[i];
            } else {
                for (uint32_t b = b0; b < b1; b++) out[g0 + b] = text[b];
            }
        }
        at += total;
        __syncthreads();  // (the next tile writes s_text and s_wsum)
    }
}

}  // namespace

int launch_row_text(const DevTextRow *rows, uint32_t n, const uint32_t *toks, const uint16_t *pidx, uint32_t n_samples,
                    uint8_t *out, uint64_t out_cap, hipStream_t stream) {
    hipLaunchKernelGGL(score_text_kernel, dim3(n), dim3(kTextBlock), 0, stream, rows, toks, pidx, n_samples, out, out_cap);
    HIP_TRY(hipGetLastError());
    return TFBS_OK;
}

int scores_state_ensure(ScoresState **state, const Patterns &P, hipStream_t stream) {
    if (*state) return TFBS_OK;
    ScoresState *s = new ScoresState();
    if (int rc = s->F.init(P, stream)) {
        delete s;
        return rc;
    }
    *state = s;
    return TFBS_OK;
}

void scores_state_destroy(ScoresState *s) { delete s; }

void scores_last_ms(const ScoresState *s, double out[4]) {
    for (int k = 0; k < 4; k++) out[k] = s ? s->ms[k] : 0.0;
}

namespace {

struct ScoreKind {  // rows_run's kind (row_frame.hpp)
    typedef DevBestRec Rec;
    typedef int32_t Val;
    typedef DevScoreHdr Hdr;
    static constexpr const char *scratch_env = "TFBS_SCORES_SCRATCH_MB", *label = "best-site";
    ScoresState &S;
    BestState *best;
    int region_check(size_t, const RegionH &) { return TFBS_OK; }
    int launch_records(hipStream_t stream, const ScanImage &img, const uint32_t *ids, const uint64_t *hap_off, size_t nh,
                       uint64_t nrec, const uint64_t **d_hap_off, const Rec **recs, double *ms) {
        return best_launch_chunk(best, stream, img, ids, hap_off, nh, nrec, d_hap_off, recs, ms);
    }
    DevBuf<Val> &vals() { return S.vals; }
    DevBuf<Hdr> &hdr() { return S.hdr; }
    void fold(dim3 grid, hipStream_t stream, RowFrame &F, const uint64_t *d_hap_off, const Rec *recs, uint64_t nrec,
              uint32_t npid) {
        hipLaunchKernelGGL(score_fold_kernel, grid, dim3(kFoldBlock), 0, stream, F.regs.p, d_hap_off, recs, nrec, F.pid_off.p,
                           F.pid_strand.p, npid, S.vals.p, F.none.p);
    }
    void stats(uint32_t n, hipStream_t stream, RowFrame &F) {
        hipLaunchKernelGGL(score_stats_kernel, dim3(n), dim3(kStatBlock), 0, stream, F.cands.p, S.vals.p, F.none.p, F.pab.p,
                           F.pcnt.p, F.pair_n.p, S.hdr.p, F.toks.p);
    }
    bool pick(const Hdr &h, uint32_t, uint64_t min_spread, uint32_t min_maf, std::string &info) {
        const uint64_t spread = (uint64_t)(h.hi - h.lo);
        if (h.none || spread == 0 || spread < min_spread) return false;
        if (maf_of(h.zero, h.one, h.two) < min_maf) return false;
        info = score_info(h.lo, h.hi, h.zero, h.one, h.two);
        return true;
    }
    bool host_row(const Val *left, const Val *right, size_t n, uint32_t, uint64_t min_spread, uint32_t *maf,
                  std::string &info, std::string &gts) {
        return scores_as_genotypes(left, right, n, min_spread, maf, info, gts);
    }
};

}  // namespace

int scores_run(ScoresState **state, BestState **best, int device, void *stream_, const Patterns &P,
               const ScanImage &img, const Batch &B, size_t r0, size_t r1, const std::string &chrom, uint32_t min_maf,
               uint64_t min_spread, uint32_t *fake, std::string *out, uint64_t *n_rows) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(device));
    *n_rows = 0;
    uint32_t n_strands = 0;
    int rc;
    if ((rc = best_prepare(best, device, stream_, P, &n_strands)) || (rc = scores_state_ensure(state, P, stream))) return rc;
    ScoreKind kind{**state, *best};
    return rows_run((*state)->F, kind, (*state)->ms, device, stream, n_strands, img, B, r0, r1, chrom, min_maf, min_spread,
                    fake, out, n_rows);
}

}  // namespace tfbs
