// Per-sample encoding on the device (tfbs_batch_encode).
#include "ctx.hpp"

using namespace tfbs;

extern "C" {

int tfbs_batch_encode(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1) {
    return tfbs_batch_encode_flags(ctx, b, r0, r1, 0);
}

int tfbs_batch_encode_flags(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, int flags) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not resident on this ctx");
    Batch &B = b->b;
    if (!B.reduced) return tfbs::fail(TFBS_E_STATE, "keys not reduced (tfbs_batch_reduce)");
    if (!B.keep_membership) return tfbs::fail(TFBS_E_STATE, "batch created without membership");
    {  // the varying counts the encode reads are this ctx's (var_counts, at the offsets of its reduction)
        std::lock_guard<std::mutex> g(B.var_mu);
        if (B.var_ctx != ctx) return tfbs::fail(TFBS_E_STATE, "batch last reduced on another ctx (tfbs_batch_reduce here)");
    }
    r1 = std::min(r1, B.rh.size());
    r0 = std::min(r0, r1);
    HIP_TRY(hipSetDevice(ctx->device));
    B.enc_r0 = B.enc_r1 = 0;
    B.enc_idx.assign(B.var_keys.size(), UINT32_MAX);
    B.enc_hdr.clear();
    B.enc_vals.clear();
    B.enc_hist.clear();
    B.enc_val_off.assign(1, 0);
    B.enc_code_off.assign(1, 0);
    const uint32_t N = B.n_samples, H = 2 * N;
    if (N == 0 || r0 == r1) {
        B.enc_r0 = (uint32_t)r0;
        B.enc_r1 = (uint32_t)r1;
        return TFBS_OK;
    }
    // every region's u16 membership row on this device -- a device-grouped region's
    // own, the others' made by the host threads in the ctx's pinned staging and
    // uploaded -- then its distinct (left, right) haplotype pairs and each sample's
    // pair on the device (launch_pair_table)
    const size_t nr = r1 - r0;
    int rc;
    std::vector<uint64_t> rows(nr, 0);
    std::vector<size_t> hostr;
    for (size_t r = r0; r < r1; r++) {
        const RegionH &R = B.rh[r];
        if (R.hap_count > kEncMaxHaps) continue;
        if (!R.memb_host && B.grouper && B.grouper->device() == ctx->device) rows[r - r0] = R.memb_dev;
        else hostr.push_back(r);
    }
    for (size_t r : hostr)
        if ((rc = region_membership(B, B.rh[r]))) return rc;
    const size_t Hp = ((size_t)H + 7) / 8 * 8;
    if (!hostr.empty()) {
        // their non-reference lists (haplotype id, distinct index) go up, the rows are
        // filled on the device (launch_memb_fill): a few MB instead of Hp u16 per region
        std::vector<uint32_t> meta(2 * (hostr.size() + 1), 0);
        uint64_t tot = 0;
        for (size_t k = 0; k < hostr.size(); k++) {
            const RegionH &R = B.rh[hostr[k]];
            meta[2 * k] = (uint32_t)tot;
            meta[2 * k + 1] = (uint32_t)(R.ref_local < 0 ? 0 : R.ref_local);
            tot += R.nonref_id.size();
        }
        if (tot >= UINT32_MAX) return tfbs::fail(TFBS_E_NOMEM, "too many non-reference haplotypes in one call");
        meta[2 * hostr.size()] = (uint32_t)tot;
        if ((rc = ctx->enc.enc_memb_host.reserve(std::max<uint64_t>(tot, 1) * 6)) ||
            (rc = ctx->enc.enc_memb.ensure(hostr.size() * Hp)) || (rc = ctx->enc.enc_nr_ids.ensure(std::max<uint64_t>(tot, 1))) ||
            (rc = ctx->enc.enc_nr_loc.ensure(std::max<uint64_t>(tot, 1))) || (rc = ctx->enc.enc_nr_meta.put(meta, ctx->stream)))
            return rc;
        uint32_t *const ids = reinterpret_cast<uint32_t *>(ctx->enc.enc_memb_host.p);
        uint16_t *const loc = reinterpret_cast<uint16_t *>(ctx->enc.enc_memb_host.p + 4 * std::max<uint64_t>(tot, 1));
        const uint32_t T = std::max(1u, std::min(ctx->enc.host_threads, (uint32_t)hostr.size()));
        std::atomic<size_t> next(0);
        auto work = [&]() {
            for (size_t k; (k = next.fetch_add(1)) < hostr.size();) {
                const RegionH &R = B.rh[hostr[k]];
                const size_t o = meta[2 * k];
                for (size_t i = 0; i < R.nonref_id.size(); i++) {
                    ids[o + i] = R.nonref_id[i];
                    loc[o + i] = (uint16_t)R.nonref_local[i];
                }
            }
        };
        std::vector<std::thread> ts;
        for (uint32_t t = 1; t < T; t++) ts.emplace_back(work);
        work();
        for (auto &t : ts) t.join();
        if (tot) {
            HIP_TRY(hipMemcpyAsync(ctx->enc.enc_nr_ids.p, ids, tot * 4, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(ctx->enc.enc_nr_loc.p, loc, tot * 2, hipMemcpyHostToDevice, ctx->stream));
        }
        if ((rc = launch_memb_fill(ctx->enc.enc_nr_meta.p, ctx->enc.enc_nr_ids.p, ctx->enc.enc_nr_loc.p, (uint32_t)hostr.size(),
                                   (uint32_t)Hp, ctx->enc.enc_memb.p, ctx->stream)))
            return rc;
    }
    for (size_t k = 0; k < hostr.size(); k++) rows[hostr[k] - r0] = (uint64_t)(uintptr_t)(ctx->enc.enc_memb.p + k * Hp);
    std::vector<uint32_t> pair_n(nr);
    if ((rc = ctx->enc.enc_rows.put(rows, ctx->stream)) || (rc = ctx->enc.enc_pab.ensure(nr * kEncMaxPairs)) ||
        (rc = ctx->enc.enc_pcnt.ensure(nr * kEncMaxPairs)) || (rc = ctx->enc.enc_pair_n.ensure(nr)) ||
        (rc = ctx->enc.enc_pidx.ensure(std::max<size_t>(nr * (size_t)N, 1))))
        return rc;
    if ((rc = launch_pair_table(ctx->enc.enc_rows.p, (uint32_t)nr, N, ctx->enc.enc_pab.p, ctx->enc.enc_pcnt.p,
                                ctx->enc.enc_pair_n.p, ctx->enc.enc_pidx.p, ctx->stream)))
        return rc;
    HIP_TRY(hipMemcpyAsync(pair_n.data(), ctx->enc.enc_pair_n.p, nr * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // the keys to encode: varying keys of [r0, r1) whose region's pairs were listed
    // (<= kEncMaxHaps distinct haplotypes, <= kEncMaxPairs pairs; the others keep the host path)
    std::vector<DevVarKey> ek;
    // (B.var_keys is in region order: tfbs_batch_reduce)
    auto region_lb = [&](size_t r) {
        return (uint32_t)(std::lower_bound(B.var_keys.begin(), B.var_keys.end(), r,
                                           [](const DevVarKey &k, size_t x) { return k.region < x; }) -
                          B.var_keys.begin());
    };
    for (uint32_t i = region_lb(r0), i1 = region_lb(r1); i < i1; i++) {
        const DevVarKey &k = B.var_keys[i];
        if (pair_n[k.region - r0] == UINT32_MAX) continue;
        B.enc_idx[i] = (uint32_t)ek.size();
        ek.push_back(k);
    }
    const size_t nk = ek.size();
    if ((rc = ctx->enc.enc_keys.put(ek, ctx->stream)) || (rc = ctx->enc.enc_hdr.ensure(std::max<size_t>(nk, 1))) ||
        (rc = ctx->enc.enc_vals.ensure(std::max<size_t>(nk, 1) * (kEncMaxVals + 1))) ||
        (rc = ctx->enc.enc_hist.ensure(std::max<size_t>(nk, 1) * (kEncMaxVals + 1))) ||
        (rc = ctx->enc.enc_codes.ensure(std::max<size_t>(nk, 1) * N)))
        return rc;
    if ((rc = launch_key_encode(ctx->asmb.var_counts.p, ctx->enc.enc_keys.p, (uint32_t)nk, ctx->enc.enc_pab.p, ctx->enc.enc_pcnt.p,
                                ctx->enc.enc_pair_n.p, ctx->enc.enc_pidx.p, (uint32_t)r0, N, ctx->enc.enc_hdr.p, ctx->enc.enc_vals.p,
                                ctx->enc.enc_hist.p, ctx->enc.enc_codes.p, ctx->stream)))
        return rc;
    B.enc_hdr.resize(nk);
    B.enc_val_off.assign(nk + 1, 0);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(B.enc_hdr.data(), ctx->enc.enc_hdr.p, nk * sizeof(EncHdr), hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        // the value tables and histograms, and the packed codes, back to back (a key's
        // number of values and code width are known only now)
        B.enc_code_off.resize(nk + 1);
        for (size_t k = 0; k < nk; k++) {
            const EncHdr &h = B.enc_hdr[k];
            const uint64_t bytes = h.status ? 0 : ((uint64_t)N * h.width + 7) / 8;
            B.enc_code_off[k + 1] = B.enc_code_off[k] + bytes;
            B.enc_val_off[k + 1] = B.enc_val_off[k] + (h.status ? 0u : h.n_vals);
        }
        const uint32_t nv_tot = B.enc_val_off[nk];
        if ((rc = ctx->enc.enc_val_off.put(B.enc_val_off, ctx->stream)) ||
            (rc = ctx->enc.enc_vals_c.ensure(std::max<uint32_t>(nv_tot, 1))) ||
            (rc = ctx->enc.enc_hist_c.ensure(std::max<uint32_t>(nv_tot, 1))))
            return rc;
        if ((rc = launch_val_compact(ctx->enc.enc_vals.p, ctx->enc.enc_hist.p, (uint32_t)nk, ctx->enc.enc_val_off.p,
                                     ctx->enc.enc_vals_c.p, ctx->enc.enc_hist_c.p, ctx->stream)))
            return rc;
        B.enc_vals.resize(nv_tot);
        B.enc_hist.resize(nv_tot);
        if (nv_tot) {
            HIP_TRY(hipMemcpyAsync(B.enc_vals.data(), ctx->enc.enc_vals_c.p, (size_t)nv_tot * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
            HIP_TRY(hipMemcpyAsync(B.enc_hist.data(), ctx->enc.enc_hist_c.p, (size_t)nv_tot * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
        }
        const uint64_t total = B.enc_code_off[nk];
        if ((rc = ctx->enc.enc_off.put(B.enc_code_off, ctx->stream)) ||
            (rc = ctx->enc.enc_packed.ensure(total + 16)) ||  // (the BGZF staging reads whole dwords)
            (!(flags & TFBS_ENC_DEVICE_CODES) && (rc = B.enc_codes.reserve(total))))
            return rc;
        if ((rc = launch_code_compact(ctx->enc.enc_codes.p, (uint32_t)nk, N, ctx->enc.enc_off.p, ctx->enc.enc_packed.p,
                                      ctx->stream)))
            return rc;
        if (total && !(flags & TFBS_ENC_DEVICE_CODES))
            HIP_TRY(hipMemcpyAsync(B.enc_codes.p, ctx->enc.enc_packed.p, total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    B.enc_r0 = (uint32_t)r0;
    B.enc_r1 = (uint32_t)r1;
    B.enc_codes_host = !(flags & TFBS_ENC_DEVICE_CODES);
    return TFBS_OK;
}

}  // extern "C"
