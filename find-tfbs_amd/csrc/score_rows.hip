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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "hit_score.hpp"
#include "keys.hpp"
#include "scores.hpp"

namespace tfbs {
namespace {

constexpr int kFoldBlock = 256;
constexpr int kStatBlock = 256;
constexpr int kTextBlock = 512;  // samples per tile: one per thread
constexpr uint32_t kNotListed = 0xFFFFFFFFu;
// a token: t in bits 0-14, the class in 16-17, d == 0 in 18, d == spread in 19
constexpr uint32_t kTokLo = 1u << 18, kTokHi = 1u << 19;

struct DevFoldRegion {  // one region of a chunk
    uint32_t k0;        // its first haplotype among the chunk's
    uint32_t U, nr, pad;
    uint64_t val_off;   // its values: [(range * n_pids + q) * U + h]
};

struct DevCand {        // one candidate row whose region's pairs are listed
    uint64_t val_off;   // its U values
    uint64_t tok_off;   // its tokens, one per pair
    uint32_t region;    // of the chunk (the pair table's)
    uint32_t U;
};

struct DevScoreHdr {
    int64_t lo, hi;
    uint64_t text_len;  // of the genotype text
    uint32_t zero, one, two;
    uint32_t none;      // a carried haplotype without a value: no row
};

struct DevTextRow {
    uint64_t out_off;   // the genotype text's place in the group's text
    uint64_t tok_off;
    uint32_t region, pad;
};

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
        uint32_t cls, t;
        score_class(d, spread, &cls, &t);
        const bool ext = d == 0 || d == spread;
        cnt[0] += cls == 0 ? w : 0;
        cnt[1] += cls == 1 ? w : 0;
        cnt[2] += cls == 2 ? w : 0;
        len += (uint64_t)w * (ext ? 8u : 11u);
        toks[C.tok_off + i] = t | (cls << 16) | (d == 0 ? kTokLo : 0u) | (d == spread ? kTokHi : 0u);
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

struct ScoresState {
    DevBuf<uint32_t> pid_off, pid_strand;
    std::vector<uint16_t> pids;                 // ascending pattern ids
    DevBuf<uint64_t> rows;                         // membership rows' addresses
    DevBuf<uint16_t> memb, pidx;
    DevBuf<uint32_t> pab, pcnt, pair_n, toks;
    DevBuf<DevFoldRegion> regs;
    DevBuf<int32_t> vals;
    DevBuf<uint8_t> none, text;
    DevBuf<DevCand> cands;
    DevBuf<DevScoreHdr> hdr;
    DevBuf<DevTextRow> trows;
    PinnedBytes host;
    Event ev[2];
    double ms[4] = {0, 0, 0, 0};
    int init(const Patterns &P, hipStream_t stream) {
        std::map<uint16_t, std::vector<uint32_t>> by_pid;  // ascending pattern_id -> its strands in creation order
        for (uint32_t p = 0; p < P.pats.size(); p++) by_pid[P.pats[p].pattern_id].push_back(p);
        std::vector<uint32_t> off{0}, strands;
        for (const auto &ps : by_pid) {
            pids.push_back(ps.first);
            strands.insert(strands.end(), ps.second.begin(), ps.second.end());
            off.push_back((uint32_t)strands.size());
        }
        int rc;
        if ((rc = pid_off.ensure_exact(off.size())) || (rc = pid_strand.ensure_exact(std::max<size_t>(strands.size(), 1)))) return rc;
        HIP_TRY(hipMemcpyAsync(pid_off.p, off.data(), 4 * off.size(), hipMemcpyHostToDevice, stream));
        if (!strands.empty())
            HIP_TRY(hipMemcpyAsync(pid_strand.p, strands.data(), 4 * strands.size(), hipMemcpyHostToDevice, stream));
        for (Event &e : ev) HIP_TRY(e.create());
        HIP_TRY(hipStreamSynchronize(stream));  // (the vectors go out of scope)
        return TFBS_OK;
    }
};

void scores_state_destroy(ScoresState *s) { delete s; }

void scores_last_ms(const ScoresState *s, double out[4]) {
    for (int k = 0; k < 4; k++) out[k] = s ? s->ms[k] : 0.0;
}

namespace {

template <typename T>
int put(DevBuf<T> &b, const std::vector<T> &v, hipStream_t stream) {
    if (int rc = b.ensure_exact(std::max<size_t>(v.size(), 1))) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return TFBS_OK;
}

struct PickedRow {       // a row to write
    std::string head;    // "<chr>\t<POS>\t ... \tGT:DS"
    std::string geno;    // the genotype text of a row made on the host
    uint64_t geno_len;
    uint64_t tok_off;
    uint32_t region;     // of the chunk; kNotListed: geno holds the text
};

// The distinct index of every haplotype id of region R (the fallback's membership).
int region_locals(const Batch &B, const RegionH &R, std::vector<uint32_t> &local) {
    if (int rc = region_membership(B, R)) return rc;
    local.assign(2 * (size_t)B.n_samples, (uint32_t)(R.ref_local < 0 ? 0 : R.ref_local));
    for (size_t i = 0; i < R.nonref_id.size(); i++)
        if (R.nonref_id[i] < local.size()) local[R.nonref_id[i]] = R.nonref_local[i];
    return TFBS_OK;
}

}  // namespace

int scores_run(ScoresState **state, BestState **best, int device, void *stream_, const Patterns &P,
               const ScanImage &img, const Batch &B, size_t r0, size_t r1, const std::string &chrom, uint32_t min_maf,
               uint64_t min_spread, uint32_t *fake, std::string *out, uint64_t *n_rows) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(device));
    *n_rows = 0;
    uint32_t n_strands = 0;
    int rc;
    if ((rc = best_prepare(best, device, stream_, P, &n_strands))) return rc;
    if (!*state) {
        ScoresState *s = new ScoresState();
        if ((rc = s->init(P, stream))) {
            delete s;
            return rc;
        }
        *state = s;
    }
    ScoresState &S = **state;
    for (double &m : S.ms) m = 0;
    const uint64_t ns = n_strands, npid = S.pids.size();
    const uint32_t N = B.n_samples;
    // the regions that have candidate rows
    std::vector<size_t> todo;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        for (size_t k = 1; k < R.ranges.size(); k++)
            if (!(R.ranges[k - 1] < R.ranges[k])) return fail(TFBS_E_STATE, "inner ranges of a region not ascending");
        if (R.ranges.size() != B.regions[r].n_inner) return fail(TFBS_E_STATE, "inner ranges of a region not packed");
        if (!R.ranges.empty() && R.hap_count) todo.push_back(r);
    }
    if (todo.empty() || ns == 0 || npid == 0 || N == 0) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, "too many strands for the best-site kernel");
    const uint64_t budget = scratch_budget("TFBS_SCORES_SCRATCH_MB", 256.0);  // read at the call
    const size_t Hp = (2 * (size_t)N + 7) / 8 * 8;
    auto keys_of = [&](const RegionH &R) {
        uint64_t n = 0;
        for (const InnerKey &k : R.keys) n += k.slot >= 0;
        return n;
    };
    // a region's share of the scratch: records, values, tokens (at most a pair per sample), the pair table, its row
    auto cost_of = [&](const RegionH &R) {
        const uint64_t U = R.hap_count, nr = R.ranges.size();
        return U * ns * nr * sizeof(DevBestRec) + U * nr * npid * 5 +
               keys_of(R) * npid * std::min<uint64_t>(N, kEncMaxPairs) * 4 + (uint64_t)kEncMaxPairs * 8 + 2ull * N + 2 * Hp;
    };
    const std::string chr = chrom;
    std::vector<uint32_t> ids;
    std::vector<uint64_t> hap_off, rows;
    std::vector<DevFoldRegion> regs;
    std::vector<DevCand> cands;
    std::vector<DevTextRow> trows;
    std::vector<uint32_t> pair_n, local;
    std::vector<int32_t> left, right, hv;
    std::vector<uint8_t> hn;
    std::vector<PickedRow> picked;
    for (size_t start = 0; start < todo.size();) {
        // the chunk: whole regions whose scratch fits half the budget, one at least
        size_t nreg = 0;
        uint64_t cost = 0, nhap = 0, ncand_all = 0;
        while (start + nreg < todo.size() && nreg < 65535) {
            const RegionH &R = B.rh[todo[start + nreg]];
            const uint64_t add = cost_of(R), nc = keys_of(R) * npid;
            if (nreg && (cost + add > budget / 2 || (nhap + R.hap_count) * ns > kHitsMaxPairs || ncand_all + nc > (1u << 30)))
                break;
            cost += add;
            nhap += R.hap_count;
            ncand_all += nc;
            nreg++;
        }
        // the regions' membership rows on this device (a device-grouped region's own, the others'
        // filled here and uploaded), then their distinct pairs and each sample's pair
        rows.assign(nreg, 0);
        std::vector<size_t> hostr;
        for (size_t i = 0; i < nreg; i++) {
            const RegionH &R = B.rh[todo[start + i]];
            if (R.hap_count > kEncMaxHaps) continue;
            if (!R.memb_host && B.grouper && B.grouper->device() == device) rows[i] = R.memb_dev;
            else hostr.push_back(i);
        }
        if (!hostr.empty()) {
            if ((rc = S.host.reserve(hostr.size() * Hp * 2)) || (rc = S.memb.ensure_exact(hostr.size() * Hp))) return rc;
            uint16_t *m = reinterpret_cast<uint16_t *>(S.host.p);
            for (size_t k = 0; k < hostr.size(); k++) {
                const RegionH &R = B.rh[todo[start + hostr[k]]];
                if ((rc = region_membership(B, R))) return rc;
                uint16_t *row = m + k * Hp;
                std::fill(row, row + Hp, (uint16_t)(R.ref_local < 0 ? 0 : R.ref_local));
                for (size_t i = 0; i < R.nonref_id.size(); i++)
                    if (R.nonref_id[i] < 2 * (size_t)N) row[R.nonref_id[i]] = (uint16_t)R.nonref_local[i];
                rows[hostr[k]] = (uint64_t)(uintptr_t)(S.memb.p + k * Hp);
            }
            HIP_TRY(hipMemcpyAsync(S.memb.p, m, hostr.size() * Hp * 2, hipMemcpyHostToDevice, stream));
        }
        if ((rc = put(S.rows, rows, stream)) || (rc = S.pab.ensure_exact(nreg * (size_t)kEncMaxPairs)) ||
            (rc = S.pcnt.ensure_exact(nreg * (size_t)kEncMaxPairs)) || (rc = S.pair_n.ensure_exact(nreg)) ||
            (rc = S.pidx.ensure_exact(nreg * (size_t)N)))
            return rc;
        if ((rc = launch_pair_table(S.rows.p, (uint32_t)nreg, N, S.pab.p, S.pcnt.p, S.pair_n.p, S.pidx.p, stream)))
            return rc;
        // the best records of the chunk's haplotypes, left on the device
        ids.clear();
        hap_off.clear();
        regs.clear();
        uint64_t nrec = 0, nval = 0, max_vals = 0;
        for (size_t i = 0; i < nreg; i++) {
            const RegionH &R = B.rh[todo[start + i]];
            const uint32_t nr = (uint32_t)R.ranges.size();
            regs.push_back(DevFoldRegion{(uint32_t)ids.size(), R.hap_count, nr, 0, nval});
            for (uint32_t h = 0; h < R.hap_count; h++) {
                ids.push_back(R.hap_begin + h);
                hap_off.push_back(nrec);
                nrec += ns * nr;
            }
            const uint64_t nv = (uint64_t)nr * npid * R.hap_count;
            nval += nv;
            max_vals = std::max(max_vals, nv);
        }
        const uint64_t *d_hap_off;
        const DevBestRec *d_recs;
        if ((rc = best_launch_chunk(*best, stream_, img, ids.data(), hap_off.data(), ids.size(), nrec, &d_hap_off, &d_recs,
                                    &S.ms[0])))
            return rc;
        pair_n.resize(nreg);
        HIP_TRY(hipMemcpyAsync(pair_n.data(), S.pair_n.p, 4 * nreg, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // the candidate rows of the regions whose pairs are listed
        cands.clear();
        uint64_t ntok = 0;
        for (size_t i = 0; i < nreg; i++) {
            const RegionH &R = B.rh[todo[start + i]];
            if (pair_n[i] == kNotListed) continue;
            for (const InnerKey &k : R.keys) {  // sorted by (s, e, bed): the rows' order; each once
                if (k.slot < 0) continue;       // an empty inner range
                for (uint32_t q = 0; q < npid; q++) {
                    cands.push_back(DevCand{regs[i].val_off + ((uint64_t)k.slot * npid + q) * R.hap_count, ntok,
                                            (uint32_t)i, R.hap_count});
                    ntok += pair_n[i];
                }
            }
        }
        if ((rc = put(S.regs, regs, stream)) || (rc = S.vals.ensure_exact(nval)) || (rc = S.none.ensure_exact(nval)) ||
            (rc = put(S.cands, cands, stream)) || (rc = S.hdr.ensure_exact(std::max<size_t>(cands.size(), 1))) ||
            (rc = S.toks.ensure_exact(std::max<uint64_t>(ntok, 1))))
            return rc;
        HIP_TRY(hipEventRecord(S.ev[0], stream));
        hipLaunchKernelGGL(score_fold_kernel,
                           dim3((uint32_t)std::min<uint64_t>((max_vals + kFoldBlock - 1) / kFoldBlock, 1024), (uint32_t)nreg),
                           dim3(kFoldBlock), 0, stream, S.regs.p, d_hap_off, d_recs, nrec, S.pid_off.p, S.pid_strand.p,
                           (uint32_t)npid, S.vals.p, S.none.p);
        HIP_TRY(hipGetLastError());
        if (!cands.empty()) {
            hipLaunchKernelGGL(score_stats_kernel, dim3((uint32_t)cands.size()), dim3(kStatBlock), 0, stream, S.cands.p,
                               S.vals.p, S.none.p, S.pab.p, S.pcnt.p, S.pair_n.p, S.hdr.p, S.toks.p);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(S.ev[1], stream));
        HIP_TRY(hipEventSynchronize(S.ev[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        S.ms[1] += ms;
        double t0 = now_ms();
        if ((rc = S.host.reserve(std::max<size_t>(cands.size(), 1) * sizeof(DevScoreHdr)))) return rc;
        if (!cands.empty())
            HIP_TRY(hipMemcpyAsync(S.host.p, S.hdr.p, cands.size() * sizeof(DevScoreHdr), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // the rows: picked from the headers, or made on the host for a region whose pairs are not listed
        picked.clear();
        const DevScoreHdr *hd = reinterpret_cast<const DevScoreHdr *>(S.host.p);
        auto pick = [&](const InnerKey &k, uint32_t q, const std::string &info, PickedRow &&row) {
            (*n_rows)++;
            if (!out) return;
            char pos[24];
            snprintf(pos, sizeof pos, "\t%u\t", *fake);
            (*fake)++;
            row.head = chr + pos + score_row_head(B, k, S.pids[q], info);
            picked.push_back(std::move(row));
        };
        size_t c = 0;
        for (size_t i = 0; i < nreg; i++) {
            const RegionH &R = B.rh[todo[start + i]];
            const uint32_t U = R.hap_count;
            if (pair_n[i] != kNotListed) {
                for (const InnerKey &k : R.keys) {
                    if (k.slot < 0) continue;
                    for (uint32_t q = 0; q < npid; q++, c++) {
                        const DevScoreHdr &h = hd[c];
                        const uint64_t spread = (uint64_t)(h.hi - h.lo);
                        if (h.none || spread == 0 || spread < min_spread) continue;
                        if (maf_of(h.zero, h.one, h.two) < min_maf) continue;
                        pick(k, q, score_info(h.lo, h.hi, h.zero, h.one, h.two),
                             PickedRow{std::string(), std::string(), h.text_len, cands[c].tok_off, (uint32_t)i});
                    }
                }
                continue;
            }
            const uint64_t nv = (uint64_t)R.ranges.size() * npid * U;
            hv.resize(nv);
            hn.resize(nv);
            HIP_TRY(hipMemcpyAsync(hv.data(), S.vals.p + regs[i].val_off, 4 * nv, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(hn.data(), S.none.p + regs[i].val_off, nv, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if ((rc = region_locals(B, R, local))) return rc;
            left.resize(N);
            right.resize(N);
            for (const InnerKey &k : R.keys) {
                if (k.slot < 0) continue;
                for (uint32_t q = 0; q < npid; q++) {
                    const size_t base = ((size_t)k.slot * npid + q) * U;
                    bool none = false;
                    for (uint32_t s = 0; s < N && !none; s++) {
                        const uint32_t a = local[2 * s], b = local[2 * s + 1];
                        if (a >= U || b >= U) return fail(TFBS_E_STATE, "membership names a haplotype the region lacks");
                        none = hn[base + a] || hn[base + b];
                        left[s] = hv[base + a];
                        right[s] = hv[base + b];
                    }
                    if (none) continue;
                    uint32_t maf = 0;
                    std::string info, gts;
                    if (!scores_as_genotypes(left.data(), right.data(), N, min_spread, &maf, info, gts)) continue;
                    if (maf < min_maf) continue;
                    const uint64_t glen = gts.size();
                    pick(k, q, info, PickedRow{std::string(), out ? std::move(gts) : std::string(), glen, 0, kNotListed});
                }
            }
        }
        S.ms[3] += now_ms() - t0;
        // the text, in groups of rows that fit the other half of the budget, one row at least
        for (size_t g0 = 0; g0 < picked.size();) {
            size_t g1 = g0;
            uint64_t bytes = 0;
            trows.clear();
            while (g1 < picked.size()) {
                const PickedRow &r = picked[g1];
                const uint64_t add = r.head.size() + r.geno_len + 1;
                if (g1 > g0 && bytes + add > budget / 2) break;
                if (r.region != kNotListed) trows.push_back(DevTextRow{bytes + r.head.size(), r.tok_off, r.region, 0});
                bytes += add;
                g1++;
            }
            if ((rc = S.text.ensure_exact(bytes + 16)) || (rc = S.host.reserve(bytes + 16))) return rc;
            if (!trows.empty()) {
                if ((rc = put(S.trows, trows, stream))) return rc;
                HIP_TRY(hipEventRecord(S.ev[0], stream));
                hipLaunchKernelGGL(score_text_kernel, dim3((uint32_t)trows.size()), dim3(kTextBlock), 0, stream, S.trows.p,
                                   S.toks.p, S.pidx.p, N, S.text.p, bytes);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(S.ev[1], stream));
                HIP_TRY(hipEventSynchronize(S.ev[1]));
                HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
                S.ms[2] += ms;
                t0 = now_ms();
                HIP_TRY(hipMemcpyAsync(S.host.p, S.text.p, bytes, hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
            } else {
                t0 = now_ms();
            }
            const size_t at0 = out->size();
            out->append(reinterpret_cast<const char *>(S.host.p), bytes);
            size_t at = at0;
            for (size_t k = g0; k < g1; k++) {
                const PickedRow &r = picked[k];
                memcpy(&(*out)[at], r.head.data(), r.head.size());
                at += r.head.size();
                if (r.region == kNotListed) memcpy(&(*out)[at], r.geno.data(), r.geno_len);
                at += r.geno_len;
                (*out)[at++] = '\n';
            }
            S.ms[3] += now_ms() - t0;
            g0 = g1;
        }
        start += nreg;
    }
    return TFBS_OK;
}

}  // namespace tfbs
