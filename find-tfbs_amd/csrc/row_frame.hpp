// The frame of the two row kinds that write one VCF row per (key, pattern id) with one field per
// sample -- the score rows (score_rows.hip) and the affinity rows (affinity_rows.hip).  A HIP
// header: only .hip sources include it.
//
// Shared: the strands-per-id CSR, the regions' membership rows and pair tables, the candidate
// rows, the 4-byte token per (candidate row, pair), the picked rows, the text kernel
// (score_text_kernel in score_rows.hip, through launch_row_text: a token does not say where it
// came from) and the chunk / group loop under a scratch budget (rows_run).  What a kind keeps:
// its records' kernel, its fold and statistics kernels, its header and how a header or -- for a
// region whose pairs are not listed -- a candidate row's values on the host become a row.
//    K::Rec, K::Val, K::Hdr          the device record, a folded value, a candidate row's header
//    K::scratch_env                  the budget's name (MiB, read at the call)
//    k.region_check(r, R)            may refuse a region that has candidate rows (non-zero)
//    k.launch_records(...)           the records of a chunk's haplotypes, left on the device
//    k.vals(), k.hdr()               the kind's own buffers
//    k.fold(grid, stream, ...)       launches the fold kernel
//    k.stats(n, stream, F)           launches the statistics kernel over F.cands
//    k.pick(h, q, min_spread, min_maf, info)    a header's row: false for none, else its INFO value
//    k.host_row(left, right, n, q, min_spread, &maf, info, gts)   the definition on the host
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "hit_score.hpp"
#include "keys.hpp"
#include "scores.hpp"

namespace tfbs {

constexpr int kFoldBlock = 256;
constexpr int kStatBlock = 256;
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

struct DevTextRow {
    uint64_t out_off;   // the genotype text's place in the group's text
    uint64_t tok_off;
    uint32_t region, pad;
};

// A pair's token from d = its level - lo (0 <= d <= spread, spread > 0), and its share of the
// row's counts and text length: w samples carry the pair.
__device__ __forceinline__ uint32_t row_token(uint64_t d, uint64_t spread, uint32_t w, uint32_t (&cnt)[3], uint64_t &len) {
    uint32_t cls, t;
    score_class(d, spread, &cls, &t);
    const bool ext = d == 0 || d == spread;
    cnt[0] += cls == 0 ? w : 0;
    cnt[1] += cls == 1 ? w : 0;
    cnt[2] += cls == 2 ? w : 0;
    len += (uint64_t)w * (ext ? 8u : 11u);
    return t | (cls << 16) | (d == 0 ? kTokLo : 0u) | (d == spread ? kTokHi : 0u);
}

// What both kinds share on a ctx: made by the first call of either (scores_state_ensure).
struct RowFrame {
    DevBuf<uint32_t> pid_off, pid_strand;
    std::vector<uint16_t> pids;                 // ascending pattern ids
    std::vector<uint32_t> first_strand;         // per pattern id its first strand in creation order
    DevBuf<uint64_t> rows;                         // membership rows' addresses
    DevBuf<uint16_t> memb, pidx;
    DevBuf<uint32_t> pab, pcnt, pair_n, toks;
    DevBuf<DevFoldRegion> regs;
    DevBuf<uint8_t> none, text;
    DevBuf<DevCand> cands;
    DevBuf<DevTextRow> trows;
    PinnedBytes host;
    Event ev[2];
    int init(const Patterns &P, hipStream_t stream) {
        std::map<uint16_t, std::vector<uint32_t>> by_pid;  // ascending pattern_id -> its strands in creation order
        for (uint32_t p = 0; p < P.pats.size(); p++) by_pid[P.pats[p].pattern_id].push_back(p);
        std::vector<uint32_t> off{0}, strands;
        for (const auto &ps : by_pid) {
            pids.push_back(ps.first);
            first_strand.push_back(ps.second[0]);
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

struct DevScoreHdr {
    int64_t lo, hi;
    uint64_t text_len;  // of the genotype text
    uint32_t zero, one, two;
    uint32_t none;      // a carried haplotype without a value: no row
};

// The score rows' state: the frame, and the score kind's values, headers and timers.
struct ScoresState {
    RowFrame F;
    DevBuf<int32_t> vals;
    DevBuf<DevScoreHdr> hdr;
    double ms[4] = {0, 0, 0, 0};
};
// score_rows.hip: *state made when it is null (the frame's tables uploaded).
int scores_state_ensure(ScoresState **state, const Patterns &P, hipStream_t stream);
// score_rows.hip: score_text_kernel over n picked rows, one workgroup each.
int launch_row_text(const DevTextRow *rows, uint32_t n, const uint32_t *toks, const uint16_t *pidx, uint32_t n_samples,
                    uint8_t *out, uint64_t out_cap, hipStream_t stream);

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
inline int region_locals(const Batch &B, const RegionH &R, std::vector<uint32_t> &local) {
    if (int rc = region_membership(B, R)) return rc;
    local.assign(2 * (size_t)B.n_samples, (uint32_t)(R.ref_local < 0 ? 0 : R.ref_local));
    for (size_t i = 0; i < R.nonref_id.size(); i++)
        if (R.nonref_id[i] < local.size()) local[R.nonref_id[i]] = R.nonref_local[i];
    return TFBS_OK;
}

// The rows of kind K of regions [r0, r1) of B: their text appended to *out with POS from *fake
// (advanced per row), or -- out null -- counted only.  ns: the strands of K's records.  ms: the
// kind's four timers (zeroed here).  Synchronises `stream`.
template <typename K>
int rows_run(RowFrame &S, K &kind, double (&kms)[4], int device, hipStream_t stream, uint64_t ns, const ScanImage &img,
             const Batch &B, size_t r0, size_t r1, const std::string &chrom, uint32_t min_maf, uint64_t min_spread,
             uint32_t *fake, std::string *out, uint64_t *n_rows) {
    typedef typename K::Rec Rec;
    typedef typename K::Val Val;
    typedef typename K::Hdr Hdr;
    int rc;
    for (double &m : kms) m = 0;
    const uint64_t npid = S.pids.size();
    const uint32_t N = B.n_samples;
    // the regions that have candidate rows
    std::vector<size_t> todo;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        for (size_t k = 1; k < R.ranges.size(); k++)
            if (!(R.ranges[k - 1] < R.ranges[k])) return fail(TFBS_E_STATE, "inner ranges of a region not ascending");
        if (R.ranges.size() != B.regions[r].n_inner) return fail(TFBS_E_STATE, "inner ranges of a region not packed");
        if (R.ranges.empty()) continue;
        if ((rc = kind.region_check(r, R))) return rc;
        if (R.hap_count) todo.push_back(r);
    }
    if (todo.empty() || ns == 0 || npid == 0 || N == 0) return TFBS_OK;
    if (ns > kHitsMaxPairs) return fail(TFBS_E_ARG, std::string("too many strands for the ") + K::label + " kernel");
    const uint64_t budget = scratch_budget(K::scratch_env, 256.0);  // read at the call
    const size_t Hp = (2 * (size_t)N + 7) / 8 * 8;
    auto keys_of = [&](const RegionH &R) {
        uint64_t n = 0;
        for (const InnerKey &k : R.keys) n += k.slot >= 0;
        return n;
    };
    // a region's share of the scratch: records, values, tokens (at most a pair per sample), the pair table, its row
    auto cost_of = [&](const RegionH &R) {
        const uint64_t U = R.hap_count, nr = R.ranges.size();
        return U * ns * nr * sizeof(Rec) + U * nr * npid * (sizeof(Val) + 1) +
               keys_of(R) * npid * std::min<uint64_t>(N, kEncMaxPairs) * 4 + (uint64_t)kEncMaxPairs * 8 + 2ull * N + 2 * Hp;
    };
    const std::string chr = chrom;
    std::vector<uint32_t> ids;
    std::vector<uint64_t> hap_off, rows;
    std::vector<DevFoldRegion> regs;
    std::vector<DevCand> cands;
    std::vector<DevTextRow> trows;
    std::vector<uint32_t> pair_n, local;
    std::vector<Val> left, right, hv;
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
        // the kind's records of the chunk's haplotypes, left on the device
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
        const Rec *d_recs;
        if ((rc = kind.launch_records(stream, img, ids.data(), hap_off.data(), ids.size(), nrec, &d_hap_off, &d_recs, &kms[0])))
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
        if ((rc = put(S.regs, regs, stream)) || (rc = kind.vals().ensure_exact(nval)) || (rc = S.none.ensure_exact(nval)) ||
            (rc = put(S.cands, cands, stream)) || (rc = kind.hdr().ensure_exact(std::max<size_t>(cands.size(), 1))) ||
            (rc = S.toks.ensure_exact(std::max<uint64_t>(ntok, 1))))
            return rc;
        HIP_TRY(hipEventRecord(S.ev[0], stream));
        kind.fold(dim3((uint32_t)std::min<uint64_t>((max_vals + kFoldBlock - 1) / kFoldBlock, 1024), (uint32_t)nreg), stream,
                  S, d_hap_off, d_recs, nrec, (uint32_t)npid);
        HIP_TRY(hipGetLastError());
        if (!cands.empty()) {
            kind.stats((uint32_t)cands.size(), stream, S);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(S.ev[1], stream));
        HIP_TRY(hipEventSynchronize(S.ev[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        kms[1] += ms;
        double t0 = now_ms();
        if ((rc = S.host.reserve(std::max<size_t>(cands.size(), 1) * sizeof(Hdr)))) return rc;
        if (!cands.empty())
            HIP_TRY(hipMemcpyAsync(S.host.p, kind.hdr().p, cands.size() * sizeof(Hdr), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // the rows: picked from the headers, or made on the host for a region whose pairs are not listed
        picked.clear();
        const Hdr *hd = reinterpret_cast<const Hdr *>(S.host.p);
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
        std::string info;
        for (size_t i = 0; i < nreg; i++) {
            const RegionH &R = B.rh[todo[start + i]];
            const uint32_t U = R.hap_count;
            if (pair_n[i] != kNotListed) {
                for (const InnerKey &k : R.keys) {
                    if (k.slot < 0) continue;
                    for (uint32_t q = 0; q < npid; q++, c++) {
                        const Hdr &h = hd[c];
                        info.clear();
                        if (!kind.pick(h, q, min_spread, min_maf, info)) continue;
                        pick(k, q, info, PickedRow{std::string(), std::string(), h.text_len, cands[c].tok_off, (uint32_t)i});
                    }
                }
                continue;
            }
            const uint64_t nv = (uint64_t)R.ranges.size() * npid * U;
            hv.resize(nv);
            hn.resize(nv);
            HIP_TRY(hipMemcpyAsync(hv.data(), kind.vals().p + regs[i].val_off, sizeof(Val) * nv, hipMemcpyDeviceToHost, stream));
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
                    std::string hinfo, gts;
                    if (!kind.host_row(left.data(), right.data(), N, q, min_spread, &maf, hinfo, gts)) continue;
                    if (maf < min_maf) continue;
                    const uint64_t glen = gts.size();
                    pick(k, q, hinfo, PickedRow{std::string(), out ? std::move(gts) : std::string(), glen, 0, kNotListed});
                }
            }
        }
        kms[3] += now_ms() - t0;
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
                if ((rc = launch_row_text(S.trows.p, (uint32_t)trows.size(), S.toks.p, S.pidx.p, N, S.text.p, bytes, stream)))
                    return rc;
                HIP_TRY(hipEventRecord(S.ev[1], stream));
                HIP_TRY(hipEventSynchronize(S.ev[1]));
                HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
                kms[2] += ms;
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
            kms[3] += now_ms() - t0;
            g0 = g1;
        }
        start += nreg;
    }
    return TFBS_OK;
}

}  // namespace tfbs
