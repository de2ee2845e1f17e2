// The key assembly stage of the device context: the assembly's launches with their lean, rerun
// and post-scan decisions, the wait that checks its lists, the step graph (tfbs_step) and
// tfbs_batch_reduce.
#include "ctx.hpp"

using namespace tfbs;

AsmArgs tfbs::asm_args(tfbs_ctx *ctx, const Batch &B, int mode) {
    AsmArgs a{};
    a.haps = ctx->img.haps.p;
    a.druns = ctx->img.druns.p;
    a.regions = ctx->img.regions.p;
    a.hap_reuse = ctx->img.hap_reuse.p;
    a.region_asm = ctx->img.region_asm.p;
    a.inner = ctx->img.inner.p;
    a.mmeta = ctx->tabs.m_meta.p;
    a.slot_mfma = ctx->tabs.slot_mfma.p;
    a.any_dense = (!ctx->plan.fast_tiles.empty() || !ctx->plan.gen_tiles.empty() || !ctx->plan.di_tiles.empty()) ? 1 : 0;
    a.n_slots = B.n_slots;
    a.hpb = ctx->knobs.mfma_hpb;
    a.hitl = ctx->scan.hitl.p;
    a.hitn = ctx->scan.hitn.p;
    a.cand_cap = ctx->scan.scan_hit_cap;  // (the hit lists' geometry)
    a.mfma = ctx->plan.m_supers.empty() ? 0 : 1;
    a.ref_hits = ctx->scan.ref_hits.p;
    a.ref_count = ctx->scan.ref_count.p;
    a.spill_sorted = ctx->scan.spill_sorted.p;
    a.spill_off = ctx->scan.spill_boff.p;
    a.spill_cnt = ctx->scan.spill_cnt_ctr ? ctx->asmb.asm_ctr.p + kAsmCtrWords : ctx->scan.spill_bcnt.p;
    // (key_fast_kernel loads spill_cnt[r] and spill_off[r] with a region's first loads whenever
    // spill_count is not null, whatever the count: with matrix-core tiles launch_scan sizes
    // spill_bcnt and spill_boff for every region + 1, and asm_ctr holds the buckets behind its
    // counter words (enqueue_assembly); without tiles spill_count is null)
    a.spill_count = ctx->plan.m_supers.empty() ? nullptr : ctx->scan.over.p;
    a.spill_cap = ctx->scan.spill_cap;
    a.counts = ctx->img.counts_live ? ctx->img.counts.p : nullptr;
    a.dense_base = ctx->img.counts_live ? 1 : 0;
    a.scratch = ctx->asmb.asm_scratch.p;
    a.mode = mode;
    return a;
}

// The device half of the key reduction, enqueued on the ctx stream behind the scan
// with no host wait: the candidates past the waves' lists rescored and the spill
// records bucketed by region (post: once per scan -- the rescoring appends spill
// records), then the key assembly (launch_key_fast); the overflow and list
// counters are copied back for assembly_wait.  Buffers are sized from the batch
// (1/16 of its keys and dense counts for the varying lists: no regrowth at C3
// shapes; TFBS_VAR_CAP=n starts at n keys and 4 n counts -- the regrow path's test).
// asm_ctr's words: keys.hpp, AsmCtr.
static int enqueue_assembly(tfbs_ctx *ctx, Batch &B, bool post) {
    int rc;
    const uint64_t n_keys = (uint64_t)(B.inner.size() / 2) * B.n_slots;
    const uint32_t nr = (uint32_t)B.regions.size();
    if ((rc = ctx->asmb.key_first.ensure(std::max<uint64_t>(n_keys, 1))) ||
        (rc = ctx->asmb.key_flags.ensure(std::max<uint64_t>(n_keys, 1))) || (rc = ctx->asmb.asm_ctr.ensure(kAsmCtrWords + asm_bucket_words(nr))) ||
        (rc = ctx->asmb.asm_redo.ensure((size_t)nr + 1)) || (rc = ctx->asmb.cor_arena.ensure(ctx->asmb.cor_cap)))
        return rc;
    if (!ctx->asmb.asm_host) HIP_TRY(ctx->asmb.asm_host.alloc(kAsmCtrWords));
    if (const int vc = env_int("TFBS_VAR_CAP", 0); vc > 0) {
        if (!ctx->asmb.var_cap_forced) {
            ctx->asmb.var_keys_cap = (uint32_t)vc;
            ctx->asmb.var_cap = 4ull * (uint32_t)vc;
            ctx->asmb.var_cap_forced = true;
        }
    } else {
        ctx->asmb.var_keys_cap = std::max<uint32_t>(ctx->asmb.var_keys_cap, (uint32_t)std::min<uint64_t>(n_keys / 16, 1u << 26));
        ctx->asmb.var_cap = std::max<uint64_t>(ctx->asmb.var_cap, std::min<uint64_t>(B.n_counts / 16, 1ull << 28));
    }
    if ((rc = ctx->asmb.var_keys.ensure(ctx->asmb.var_keys_cap)) || (rc = ctx->asmb.var_counts.ensure(ctx->asmb.var_cap))) return rc;
    if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->asmb.asm_t0, ctx->stream));
    const bool mfma = !ctx->plan.m_supers.empty();
    // the assembly's counters and the spill buckets' (at asm_ctr + kAsmCtrWords): zeroed
    // by the scan for its first assembly, else one memset
    // (a reassembly without the stage -- the varying lists regrown -- leaves the buckets'
    // counts as they are: its readers need them)
    if (!(mfma && post && ctx->asmb.asm_ctr_zeroed && ctx->img.n_regions == nr))
        HIP_TRY(hipMemsetAsync(ctx->asmb.asm_ctr.p, 0, (kAsmCtrWords + (mfma && post ? asm_bucket_words(nr) : 0)) * 4,
                               ctx->stream));
    ctx->asmb.asm_ctr_zeroed = false;
    // lean (AsmStages, ctx.hpp): left out what the batch's last checked assembly did not need
    const bool lean = mfma && post && !ctx->asmb.asm_full && ctx->knobs.asm_lean_mode != 0;
    ctx->asmb.stages.wide = !(lean && (ctx->knobs.asm_lean_mode == 2 || ctx->asmb.prev_spill <= kPostSerial));
    ctx->asmb.stages.leftover = !(lean && (ctx->knobs.asm_lean_mode == 2 || ctx->asmb.prev_redo == 0));
    if (mfma && post) {  // overflow candidates rescored (once per scan: they append spill records) + spill buckets
        // (without the leftover pass post_scan_kernel copies the overflow counters to
        // asm_ctr + kCtrOver; asm_ctr[kCtrNeedWide]: set when the records needed the wide kernels)
        ctx->asmb.stages.post = true;
        ctx->asmb.stages.inplace = 0;
        ctx->asmb.stages.post_fused = ctx->scan.post_fused;
        if (ctx->scan.post_fused) {  // the scan's last workgroup did it (lean: no wide kernels)
            ctx->asmb.stages.wide = false;
        } else if (asm_skips_post(ctx)) {  // nothing for it last time, or a few records: no launch, no buckets
            ctx->asmb.stages.post = ctx->asmb.stages.wide = false;
            // (after an assembly without a record: none is read, as before -- the kernels then take
            // the path of a launch without a spill list, which is what C2's 50 us step is measured on --
            // and a record that does appear reruns the assembly in full)
            ctx->asmb.stages.inplace = ctx->knobs.asm_lean_mode != 2 && ctx->asmb.prev_spill == 0
                                           ? 0u : std::min(ctx->knobs.spill_inplace, ctx->scan.spill_cap);
        } else if ((rc = launch_post_fused(ctx->scan.last_margs, !ctx->scan.post_done, ctx->asmb.asm_ctr.p + kCtrWgDone,
                                           std::max<uint32_t>(1, nr), ctx->asmb.asm_ctr.p + kAsmCtrWords, ctx->scan.spill_boff.p,
                                           ctx->scan.spill_sorted.p, ctx->stream, ctx->asmb.stages.wide, ctx->asmb.asm_ctr.p,
                                           ctx->asmb.asm_ctr.p + kCtrNeedWide, lean && ctx->asmb.prev_cand == 0 ? 1u : 256u))) {
            return rc;
        }
        if (ctx->asmb.stages.post) {
            ctx->scan.post_done = true;
            ctx->scan.spill_cnt_ctr = true;
        }
    }
    ctx->scan.post_fused = false;
    AsmArgs a = asm_args(ctx, B, 0);
    // (no stage: no bucket is read -- stale ones least of all -- and key_fast_kernel
    // reports the scan's overflow counters, whatever they are, for assembly_wait; the records
    // are read in place up to stages.inplace, by this scan's count: ScanArgs::over[0])
    if (mfma && !ctx->asmb.stages.post) {
        if (ctx->asmb.stages.inplace) {
            a.spill_raw = ctx->scan.spill.p;
            a.spill_inplace = ctx->asmb.stages.inplace;
        } else {
            a.spill_count = nullptr;
        }
    }
    a.report_fast = mfma && !ctx->asmb.stages.post ? 1u : 0u;
    a.key_first = ctx->asmb.key_first.p;
    a.key_flags = ctx->asmb.key_flags.p;
    a.var_keys = ctx->asmb.var_keys.p;
    a.var_keys_cap = ctx->asmb.var_keys_cap;
    a.var_counts = ctx->asmb.var_counts.p;
    a.var_cap = ctx->asmb.var_cap;
    a.var_tot = reinterpret_cast<unsigned long long *>(ctx->asmb.asm_ctr.p + kCtrVarTot);
    a.redo = ctx->asmb.asm_redo.p;
    a.redo_n = ctx->asmb.asm_ctr.p + kCtrRedoN;
    a.fast_max_u = ctx->knobs.key_fast_max_u;
    a.cor_arena = ctx->asmb.cor_arena.p;
    a.cor_cap = ctx->asmb.cor_cap;
    a.cor_used = ctx->asmb.asm_ctr.p + kCtrCorUsed;
    a.cor_lds = ctx->knobs.key_cor_lds;
    a.why = ctx->knobs.debug_over ? ctx->asmb.asm_ctr.p + kCtrWhy : nullptr;
    a.report_src = mfma ? ctx->scan.over.p : nullptr;  // (copied by the list pass: no report launch)
    a.report = ctx->asmb.asm_ctr.p;
    a.order = ctx->asmb.asm_order_n == nr ? ctx->asmb.asm_order.p : nullptr;
    a.persist = ctx->knobs.kf_persistent ? 1u : 0u;
    a.next = ctx->asmb.asm_ctr.p + kCtrNext;
    a.grid_cap = ctx->knobs.kf_grid;
    ctx->asmb.asm_traced = ctx->asmb.asm_trace;
    if (ctx->asmb.asm_trace && nr) {
        if ((rc = ctx->asmb.asm_path.ensure(nr))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->asmb.asm_path.p, 0, (size_t)nr * 4, ctx->stream));
        a.path = ctx->asmb.asm_path.p;
    }
    if (ctx->knobs.kf_prof_on && nr) {
        if ((rc = ctx->asmb.kf_prof.ensure((size_t)nr * kKfProfWords))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->asmb.kf_prof.p, 0, (size_t)nr * kKfProfWords * 8, ctx->stream));
        a.prof = ctx->asmb.kf_prof.p;
    }
    if ((rc = launch_key_fast(a, nr, a.order ? ctx->asmb.asm_order_big : 0, ctx->stream, ctx->asmb.side, ctx->asmb.kf_fork,
                              ctx->asmb.kf_join, ctx->asmb.stages.leftover)) ||
        (nr == 0 && (rc = launch_asm_report(a.report_src, ctx->asmb.asm_ctr.p, ctx->stream))))
        return rc;
    if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->asmb.asm_t1, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->asmb.asm_host.p, ctx->asmb.asm_ctr.p, 4 * kAsmCtrWords, hipMemcpyDeviceToHost, ctx->stream));
    if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->asmb.asm_ev, ctx->stream));
    ctx->scan.over_pending = false;  // the assembly's check covers this scan's overflow lists
    ctx->asmb.asm_batch = &B;
    ctx->asmb.asm_state = 1;
    ctx->asmb.asm_timed = true;
    return TFBS_OK;
}

// TFBS_KF_PROF: key_fast_kernel's mean phase cycles and sizes over the regions it
// finished (debug; synchronises).
static int kf_prof_report(tfbs_ctx *ctx, uint32_t nr) {
    std::vector<uint64_t> h((size_t)nr * kKfProfWords);
    HIP_TRY(hipMemcpy(h.data(), ctx->asmb.kf_prof.p, h.size() * 8, hipMemcpyDeviceToHost));
    double ph[6] = {0, 0, 0, 0, 0, 0}, sz[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx = 0, at = 0;
    double fr[5] = {0, 0, 0, 0, 0};  // the front: 0 -> 16 -> 17 -> 1 -> 18 -> 19 (-> 2: the hits' sort)
    double tkt = 0;                  // in front of stamp 0: the ticket atomic to the order entry (word 20)
    uint32_t n = 0;
    for (uint32_t r = 0; r < nr; r++) {
        const uint64_t *p = &h[(size_t)r * kKfProfWords];
        if (!p[6]) continue;  // empty, or left to key_asm_kernel
        n++;
        for (int k = 0; k < 6; k++) ph[k] += (double)(p[k + 1] - p[k]);
        const uint64_t f[6] = {p[0], p[16], p[17], p[1], p[18], p[19]};
        for (int k = 0; k < 5; k++) fr[k] += (double)(f[k + 1] - f[k]);
        tkt += (double)p[20];
        mx = std::max(mx, (double)(p[6] - p[0]));
        at += (double)p[7];
        for (int k = 0; k < 8; k++) sz[k] += (double)p[8 + k];
    }
    std::vector<std::pair<double, uint32_t>> tot;  // (cycles, region)
    for (uint32_t r = 0; r < nr; r++)
        if (h[(size_t)r * kKfProfWords + 6]) tot.push_back({(double)(h[(size_t)r * kKfProfWords + 6] - h[(size_t)r * kKfProfWords]), r});
    std::sort(tot.begin(), tot.end());
    if (!tot.empty()) {
        auto pct = [&](double f) { return tot[std::min(tot.size() - 1, (size_t)(f * tot.size()))].first; };
        fprintf(stderr, "[kf prof] total ticks p50 %.0f p90 %.0f p99 %.0f max %.0f; slowest regions (ticks U rows chunks "
                        "corrections refs):", pct(0.5), pct(0.9), pct(0.99), tot.back().first);
        for (size_t i = tot.size(); i-- > 0 && i + 6 > tot.size();) {
            const uint64_t *p = &h[(size_t)tot[i].second * kKfProfWords];
            fprintf(stderr, " [%.0f %llu %llu %llu %llu %llu]", tot[i].first, (unsigned long long)p[8],
                    (unsigned long long)p[12], (unsigned long long)p[13], (unsigned long long)p[11],
                    (unsigned long long)p[15]);
        }
        fprintf(stderr, "\n");
    }
    uint64_t t_lo = UINT64_MAX, t_hi = 0;
    double busy = 0;
    for (uint32_t r = 0; r < nr; r++) {
        const uint64_t *p = &h[(size_t)r * kKfProfWords];
        if (!p[6]) continue;
        t_lo = std::min(t_lo, p[0]);
        t_hi = std::max(t_hi, p[6]);
        busy += (double)(p[6] - p[0]);
    }
    {  // per workgroup: its regions in start order -> gaps between them, late start, early end
        std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint32_t>> ev;  // ((workgroup, start), region)
        for (uint32_t r = 0; r < nr; r++)
            if (h[(size_t)r * kKfProfWords + 6]) ev.push_back({{h[(size_t)r * kKfProfWords + 14], h[(size_t)r * kKfProfWords]}, r});
        std::sort(ev.begin(), ev.end());
        double gap = 0, late = 0, early_end = 0;
        uint32_t n_gap = 0, n_groups = 0;
        for (size_t i = 0; i < ev.size(); i++) {
            const uint64_t *p = &h[(size_t)ev[i].second * kKfProfWords];
            const bool first = i == 0 || ev[i - 1].first.first != ev[i].first.first;
            const bool last = i + 1 == ev.size() || ev[i + 1].first.first != ev[i].first.first;
            if (first) {
                n_groups++;
                late += (double)(p[0] - t_lo);
            } else {
                gap += (double)(p[0] - h[(size_t)ev[i - 1].second * kKfProfWords + 6]);
                n_gap++;
            }
            if (last) early_end += (double)(t_hi - p[6]);
        }
        if (n_groups)
            fprintf(stderr, "[kf prof] %u workgroups: mean gap between a workgroup's regions %.1f us (%u gaps), first "
                            "region start after the kernel's first %.1f us, last end before the kernel's last %.1f us\n",
                    n_groups, n_gap ? gap / n_gap / 100.0 : 0.0, n_gap, late / n_groups / 100.0, early_end / n_groups / 100.0);
    }
    uint32_t early = 0;  // regions started in the first 10 us: the workgroups resident at the start
    for (uint32_t r = 0; r < nr; r++)
        if (h[(size_t)r * kKfProfWords + 6] && h[(size_t)r * kKfProfWords] < t_lo + 1000) early++;
    if (t_hi > t_lo)
        fprintf(stderr, "[kf prof] span %.1f us (first region start to last end, 100 MHz ticks), region-time %.1f us: "
                        "%.0f regions in flight on average; %u regions started in the first 10 us\n",
                (t_hi - t_lo) / 100.0, busy / 100.0, busy / (double)(t_hi - t_lo), early);
    const double d = n ? n : 1;
    fprintf(stderr,
            "[kf prof] front ticks/region: region record + reference hit list (round 1) %.0f, descriptors + hitn + "
            "first runs + meta (round 2) %.0f, hitn scan %.0f, runs staged %.0f, reference hits + barrier %.0f; in front of "
            "a region, ticket atomic to order entry %.0f\n",
            fr[0] / d, fr[1] / d, fr[2] / d, fr[3] / d, fr[4] / d, tkt / d);
    fprintf(stderr,
            "[kf prof] regions %u of %u ticks/region: descr+hitn %.0f refs %.0f dirty %.0f lists %.0f keys %.0f "
            "chunks %.0f (of which var-list atomics %.0f) (max total %.0f); per region: U %.1f entries %.1f dirty-refs %.1f corrections %.1f rows "
            "%.1f chunks %.2f in-LDS %.2f refs %.1f\n",
            n, nr, ph[0] / d, ph[1] / d, ph[2] / d, ph[3] / d, ph[4] / d, ph[5] / d, at / d, mx, sz[0] / d, sz[1] / d,
            sz[2] / d, sz[3] / d, sz[4] / d, sz[5] / d, sz[6] / d, sz[7] / d);
    double fine[kKfProfFineN] = {}, fine_sum = 0;  // (a kernel built with TFBS_KF_FINE: thread 0's own times)
    for (uint32_t r = 0; r < nr; r++) {
        const uint64_t *p = &h[(size_t)r * kKfProfWords];
        if (!p[6]) continue;
        for (uint32_t k = 0; k < kKfProfFineN; k++) fine[k] += (double)p[kKfProfFine + k], fine_sum += (double)p[kKfProfFine + k];
    }
    if (fine_sum != 0)
        fprintf(stderr,
                "[kf prof] fine ticks/region: dirty: pair loop %.0f listing %.0f scan %.0f; chunks: remap %.0f row keys + R "
                "%.0f base fill %.0f corrections %.0f classification %.0f var atomics %.0f varying rows %.0f\n",
                fine[0] / d, fine[1] / d, fine[2] / d, fine[3] / d, fine[4] / d, fine[5] / d, fine[6] / d, fine[7] / d,
                fine[8] / d, fine[9] / d);
    return TFBS_OK;
}

// Waits for the enqueued assembly and checks its lists: a scan overflow list that
// dropped entries means a rescan with larger lists (and a new assembly), a full
// varying-key list a new assembly with larger ones.
int tfbs::assembly_wait(tfbs_ctx *ctx, Batch &B) {
    for (int round = 0; ctx->asmb.asm_state == 1; round++) {
        if (round == 8) return tfbs::fail(TFBS_E_NOMEM, "scan / key lists still full after 8 reruns");
        HIP_TRY(hipEventSynchronize(ctx->asmb.asm_ev));
        const uint32_t nspill = ctx->asmb.asm_host[kCtrOver], ncand = ctx->asmb.asm_host[kCtrOver + 1];
        const uint64_t *vt = reinterpret_cast<const uint64_t *>(ctx->asmb.asm_host.p + kCtrVarTot);
        const uint64_t nk = vt[0], nc = vt[1];
        if (ctx->knobs.debug_over && ctx->asmb.asm_host[kCtrRedoN]) {  // the regions left to key_asm_kernel: their shapes
            std::vector<uint32_t> redo(ctx->asmb.asm_host[kCtrRedoN]);
            HIP_TRY(hipMemcpy(redo.data(), ctx->asmb.asm_redo.p, redo.size() * 4, hipMemcpyDeviceToHost));
            uint64_t su = 0, sr = 0;
            uint32_t mu = 0, mi = 0;
            for (uint32_t r : redo) {
                const DevRegion &rg = B.regions[r];
                su += rg.hap_count;
                mu = std::max(mu, rg.hap_count);
                mi = std::max(mi, rg.n_inner);
                for (uint32_t l = 0; l < rg.hap_count; l++) sr += B.haps[rg.hap_begin + l].n_druns;
            }
            const uint32_t *why = ctx->asmb.asm_host.p + kCtrWhy;
            fprintf(stderr, "tfbs assembly: %zu regions left to key_asm: mean haplotypes %.1f (max %u), max inner %u, "
                            "mean diff runs %.1f; reasons: shape %u lists %u runs %u refs %u arena(cor) %u arena(cnt) %u\n",
                    redo.size(), (double)su / redo.size(), mu, mi, (double)sr / redo.size(), why[0], why[1], why[2],
                    why[3], why[4], why[5]);
        }
        if (ctx->knobs.debug_over)
            fprintf(stderr, "tfbs assembly: spill %u/%u candidates %u/%u left to key_asm %u arena %u/%u varying keys "
                            "%llu/%u counts %llu/%llu\n", nspill, ctx->scan.spill_cap, ncand, ctx->scan.cand_over_cap,
                    ctx->asmb.asm_host[kCtrRedoN], ctx->asmb.asm_host[kCtrCorUsed], ctx->asmb.cor_cap,
                    (unsigned long long)nk, ctx->asmb.var_keys_cap, (unsigned long long)nc,
                    (unsigned long long)ctx->asmb.var_cap);
        int rc;
        // a lean assembly that needed what it left out (more spill records than post_scan_kernel
        // buckets, or regions key_fast_kernel gave up): again with everything
        // (or a record or a candidate with the post-scan stage left out: whether that one needed
        // the wide kernels too shows when the rerun has rescored the candidates)
        // (or more records than it read in place)
        const bool need_post = !ctx->asmb.stages.post && (nspill > ctx->asmb.stages.inplace || ncand);
        const bool need_wide = !ctx->asmb.stages.wide && ctx->asmb.asm_host[kCtrNeedWide], need_left = !ctx->asmb.stages.leftover && ctx->asmb.asm_host[kCtrRedoN];
        if (need_post || need_wide || need_left) {
            ctx->asmb.asm_full = true;
            ctx->asmb.asm_reruns++;
            ctx->asmb.asm_reruns_post += need_post ? 1 : 0;
            ctx->asmb.asm_post_rerun = need_post;
            ctx->asmb.asm_reruns_wide += need_wide ? 1 : 0;
            ctx->asmb.asm_reruns_left += need_left ? 1 : 0;
            rc = enqueue_assembly(ctx, B, true);
            ctx->asmb.asm_full = false;
            if (rc) return rc;
            continue;
        }
        if (ctx->asmb.asm_host[kCtrCorUsed] > ctx->asmb.cor_cap)  // regions that found the arena full went to key_asm_kernel: larger next time
            ctx->asmb.cor_cap = (uint32_t)std::min<uint64_t>((uint64_t)ctx->asmb.asm_host[kCtrCorUsed] * 5 / 4, 1u << 30);
        if (nspill > ctx->scan.spill_cap || ncand > ctx->scan.cand_over_cap) {
            grow_cap(ctx->scan.spill_cap, ncand > ctx->scan.cand_over_cap ? 2 * std::max(nspill, 1024u) : nspill, UINT32_MAX / 4);
            grow_cap(ctx->scan.cand_over_cap, ncand, UINT32_MAX / 4);
            const int n = launch_scan(ctx, (uint32_t)B.haps.size(), nullptr, 0);
            if (n < 0) return n;
            if ((rc = enqueue_assembly(ctx, B, true))) return rc;
            continue;
        }
        if (nk > ctx->asmb.var_keys_cap || nc > ctx->asmb.var_cap) {
            if (nk >= (1ull << 32) || nc >= (1ull << 40)) return tfbs::fail(TFBS_E_NOMEM, "too many varying counts");
            ctx->asmb.var_keys_cap = (uint32_t)std::max<uint64_t>(ctx->asmb.var_keys_cap, std::min<uint64_t>(nk + nk / 4 + 1024, UINT32_MAX));
            ctx->asmb.var_cap = std::max<uint64_t>(ctx->asmb.var_cap, nc + nc / 4 + 4096);
            if ((rc = enqueue_assembly(ctx, B, false))) return rc;
            continue;
        }
        ctx->asmb.asm_state = 2;
        ctx->asmb.asm_reruns_wide += ctx->asmb.asm_post_rerun && nspill > kPostSerial ? 1 : 0;
        ctx->asmb.asm_post_rerun = false;
        ctx->asmb.prev_spill = nspill;
        ctx->asmb.prev_redo = ctx->asmb.asm_host[kCtrRedoN];
        ctx->asmb.prev_cand = ncand;
        if (ctx->knobs.kf_prof_on && (rc = kf_prof_report(ctx, (uint32_t)B.regions.size()))) return rc;
    }
    return TFBS_OK;
}

extern "C" {

int tfbs_batch_assemble(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not resident on this ctx");
    if (!ctx->scan.scanned) return tfbs::fail(TFBS_E_STATE, "batch not scanned (tfbs_scan)");
    HIP_TRY(hipSetDevice(ctx->device));
    Batch &B = b->b;
    if (ctx->asmb.asm_state != 0 && ctx->asmb.asm_batch == &B) return TFBS_OK;  // this scan's assembly is on its way
    // another batch's varying counts live in var_counts: to its host copy first
    if (ctx->asmb.var_owner && ctx->asmb.var_owner != &B) {
        int rc;
        if ((rc = tfbs::ensure_host_var_counts(*ctx->asmb.var_owner))) return rc;
        std::lock_guard<std::mutex> g(ctx->asmb.var_owner->var_mu);
        if (ctx->asmb.var_owner->var_ctx == ctx) ctx->asmb.var_owner->var_ctx = nullptr;
        ctx->asmb.var_owner = nullptr;
    }
    return enqueue_assembly(ctx, B, true);
}

}  // extern "C"

// What a step's launches depend on besides the batch image: the resident batch and
// its upload, every buffer's address and every list capacity the scan and the
// assembly pass to their kernels.  A step whose signature equals the captured
// graph's replays it.
static uint64_t step_signature(const tfbs_ctx *ctx, const tfbs_batch *b) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    auto mix = [&](uint64_t v) {
        h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xBF58476D1CE4E5B9ull;
    };
    auto buf = [&](const auto &d) {
        mix((uint64_t)(uintptr_t)d.p);
        mix(d.n);
    };
    mix((uint64_t)(uintptr_t)b);
    mix((uint64_t)(uintptr_t)ctx->img.resident);
    mix(ctx->img.upload_gen);
    // every buffer a captured step passes to a kernel: each stage lists its own (ctx.hpp)
    ctx->tabs.each_buf(buf), ctx->img.each_buf(buf), ctx->lists.each_buf(buf), ctx->scan.each_buf(buf);
    ctx->asmb.each_buf(buf);
    for (int c = 0; c < 2; c++) mix(ctx->lists.sh_entries[c]);
    mix((uint64_t)ctx->lists.wl_share);
    for (uint64_t v : {(uint64_t)ctx->scan.spill_cap, (uint64_t)ctx->scan.cand_over_cap, (uint64_t)ctx->knobs.cand_cap,
                       (uint64_t)ctx->scan.scan_cand_cap, (uint64_t)ctx->scan.scan_hit_cap, (uint64_t)ctx->asmb.var_keys_cap, ctx->asmb.var_cap,
                       (uint64_t)ctx->asmb.cor_cap, (uint64_t)ctx->img.n_regions, (uint64_t)ctx->asmb.asm_order_n,
                       (uint64_t)ctx->asmb.asm_order_big,
                       (uint64_t)ctx->img.counts_live, (uint64_t)ctx->img.mfma_group_words,
                       (uint64_t)(uintptr_t)ctx->asmb.var_owner, (uint64_t)ctx->knobs.asm_lean_mode,
                       (uint64_t)(ctx->asmb.prev_spill <= kPostSerial), (uint64_t)(ctx->asmb.prev_redo == 0),
                       (uint64_t)(ctx->asmb.prev_cand == 0), (uint64_t)(ctx->asmb.prev_spill == 0),
                       (uint64_t)(ctx->asmb.prev_spill <= ctx->knobs.spill_inplace)})
        mix(v);
    return h;
}

// The host state a step leaves (tfbs_scan + tfbs_batch_assemble), set after a replay.
static void step_state(tfbs_ctx *ctx, Batch &B) {
    ctx->scan.scanned = true;
    ctx->scan.kernel_timed = false;  // (no timing events in a graph: the timing queries keep the last plain step's)
    ctx->scan.timing_pending = false;
    ctx->asmb.asm_timed = false;
    ctx->asmb.asm_ctr_zeroed = false;
    ctx->scan.post_done = true;
    ctx->scan.over_pending = false;
    ctx->scan.over_copied = false;
    ctx->asmb.asm_batch = &B;
    ctx->asmb.asm_state = 1;
    // what the captured assembly left out (a rerun in full since then changed the flags)
    ctx->asmb.stages = ctx->step.step_asm;
    if (ctx->asmb.stages.post) ctx->scan.spill_cnt_ctr = true;
    ctx->scan.post_done = ctx->asmb.stages.post;  // (left out: a rerun in full rescores the candidates)
    B.counts_valid = B.reduced = false;
    B.enc_r0 = B.enc_r1 = 0;
}

extern "C" {

int tfbs_step(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not uploaded to this ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    Batch &B = b->b;
    auto plain = [&]() -> int {
        int rc;
        ctx->scan.post_fuse_ok = true;  // (the assembly follows the scan at once)
        rc = tfbs_scan(ctx, b);
        ctx->scan.post_fuse_ok = false;
        if (rc || (rc = tfbs_batch_assemble(ctx, b))) return rc;
        return TFBS_OK;
    };
    // (another batch's varying counts in var_counts: tfbs_batch_assemble hands them over first)
    const bool eligible = ctx->knobs.step_graphs && !ctx->asmb.asm_trace && (!ctx->asmb.var_owner || ctx->asmb.var_owner == &B);
    const uint64_t sig = step_signature(ctx, b);
    int rc;
    auto replay = [&]() -> int {
        HIP_TRY(hipGraphLaunch(ctx->step.step_exec, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->asmb.asm_ev, ctx->stream));
        step_state(ctx, B);
        ctx->scan.last_launches = 1;
        return assembly_wait(ctx, B);
    };
    if (eligible && ctx->step.step_exec && sig == ctx->step.step_sig) return replay();
    ctx->step.drop();
    if (eligible && ctx->step.step_sig_seen && sig == ctx->step.step_sig) {  // the second step alike: capture it
        hipGraph_t g = nullptr;
        HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
        ctx->step.capturing = true;
        rc = plain();
        ctx->step.capturing = false;
        const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
        hipGraphExec_t x = nullptr;
        const bool ok = !rc && e == hipSuccess && g && hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess;
        const uint64_t after = step_signature(ctx, b);  // (a buffer that moved while capturing: no graph)
        if (ok && after == sig) {
            ctx->step.step_graph = g;
            ctx->step.step_exec = x;
            ctx->step.step_sig = sig;
            ctx->step.step_asm = ctx->asmb.stages;
            return replay();
        }
        (void)hipGetLastError();
        if (x) (void)hipGraphExecDestroy(x);
        if (g) (void)hipGraphDestroy(g);
        ctx->step.step_sig_seen = false;  // nothing ran: the step again, plainly
        if ((rc = plain())) return rc;
        return assembly_wait(ctx, B);
    }
    if ((rc = plain())) return rc;
    rc = assembly_wait(ctx, B);
    ctx->step.step_sig = step_signature(ctx, b);  // (after the wait: a rescan's regrown lists count)
    ctx->step.step_sig_seen = ctx->step.step_sig == sig;
    return rc;
}

int tfbs_batch_assemble_wait(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b || ctx->asmb.asm_state == 0 || ctx->asmb.asm_batch != &b->b)
        return tfbs::fail(TFBS_E_STATE, "no assembly of this batch on this ctx (tfbs_batch_assemble)");
    HIP_TRY(hipSetDevice(ctx->device));
    return assembly_wait(ctx, b->b);
}

int tfbs_ctx_assembly_trace(tfbs_ctx *ctx, int on) {
    if (!ctx) return tfbs::fail(TFBS_E_ARG, "null argument");
    ctx->asmb.asm_trace = on != 0;
    return TFBS_OK;
}

int tfbs_batch_assembly_paths(tfbs_ctx *ctx, const tfbs_batch *b, uint32_t *mask, uint32_t n) {
    if (!ctx || !b || (!mask && n)) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (!ctx->asmb.asm_trace) return tfbs::fail(TFBS_E_STATE, "the assembly trace is off (tfbs_ctx_assembly_trace)");
    if (!ctx->asmb.asm_traced) return tfbs::fail(TFBS_E_STATE, "the last assembly ran before the assembly trace was turned on");
    if (ctx->img.resident != b || ctx->asmb.asm_state != 2 || ctx->asmb.asm_batch != &b->b)
        return tfbs::fail(TFBS_E_STATE, "no checked assembly of this batch on this ctx");
    if (n != b->b.regions.size() || ctx->asmb.asm_path.n < n) return tfbs::fail(TFBS_E_ARG, "n is not the batch's regions");
    HIP_TRY(hipSetDevice(ctx->device));
    if (n) HIP_TRY(hipMemcpyAsync(mask, ctx->asmb.asm_path.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TFBS_OK;
}

int tfbs_ctx_assembly_figures(tfbs_ctx *ctx, uint64_t out[8]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->asmb.asm_state != 2 || !ctx->asmb.asm_host) return tfbs::fail(TFBS_E_STATE, "no checked assembly on this ctx");
    out[0] = ctx->asmb.asm_host[kCtrRedoN];
    out[1] = ctx->asmb.asm_host[kCtrCorUsed];
    out[2] = ctx->asmb.asm_host[kCtrOver];
    out[3] = ctx->asmb.stages.wide ? 1 : 0;
    out[4] = ctx->asmb.stages.leftover ? 1 : 0;
    out[5] = ctx->asmb.asm_reruns;
    out[6] = ctx->asmb.asm_reruns_wide;
    out[7] = ctx->asmb.asm_reruns_left;
    return TFBS_OK;
}

int tfbs_ctx_post_figures(tfbs_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->asmb.asm_state != 2 || !ctx->asmb.asm_host) return tfbs::fail(TFBS_E_STATE, "no checked assembly on this ctx");
    out[0] = ctx->asmb.stages.post ? 0 : 1;
    out[1] = ctx->asmb.asm_reruns_post;
    out[2] = ctx->asmb.stages.post ? (ctx->asmb.stages.post_fused ? 1 : 0) : ctx->asmb.stages.inplace ? 2 : 0;
    out[3] = ctx->asmb.asm_host[kCtrOver + 1];
    return TFBS_OK;
}

float tfbs_ctx_last_assemble_ms(const tfbs_ctx *ctx) {
    if (!ctx || !ctx->asmb.asm_timed) return -1.f;
    auto *c = const_cast<tfbs_ctx *>(ctx);
    float ms = -1.f;
    if (hipEventSynchronize(c->asmb.asm_t1) == hipSuccess && hipEventElapsedTime(&ms, c->asmb.asm_t0, c->asmb.asm_t1) == hipSuccess)
        c->asmb.last_asm_ms = ms;
    return c->asmb.last_asm_ms;
}

int tfbs_batch_reduce(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not resident on this ctx");
    if (!ctx->scan.scanned) return tfbs::fail(TFBS_E_STATE, "batch not scanned (tfbs_scan)");
    HIP_TRY(hipSetDevice(ctx->device));
    Batch &B = b->b;
    int rc;
    if ((rc = tfbs_batch_assemble(ctx, b)) || (rc = assembly_wait(ctx, B))) return rc;
    const uint64_t n_keys = (uint64_t)(B.inner.size() / 2) * B.n_slots;
    const uint64_t *vt = reinterpret_cast<const uint64_t *>(ctx->asmb.asm_host.p + kCtrVarTot);
    const uint32_t nk = (uint32_t)vt[0];
    const uint64_t nc = vt[1];
    if (nc >= UINT32_MAX) return tfbs::fail(TFBS_E_NOMEM, "too many varying counts (u32 offsets)");
    B.key_first.resize(n_keys);
    B.key_flags.resize(n_keys);
    std::vector<DevVarKey> vk(nk);
    if (n_keys) {
        HIP_TRY(hipMemcpyAsync(B.key_first.data(), ctx->asmb.key_first.p, n_keys * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(B.key_flags.data(), ctx->asmb.key_flags.p, n_keys, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (nk) HIP_TRY(hipMemcpyAsync(vk.data(), ctx->asmb.var_keys.p, nk * sizeof(DevVarKey), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // the varying keys in (region, key) order -- a counting sort by region, then each
    // region's few keys by key; their counts stay where the device put them
    {
        std::vector<uint32_t> at(B.regions.size() + 1, 0);
        for (const DevVarKey &k : vk) at[k.region + 1]++;
        for (size_t r = 0; r < B.regions.size(); r++) at[r + 1] += at[r];
        std::vector<DevVarKey> by(nk);
        {
            std::vector<uint32_t> put(at.begin(), at.end() - 1);
            for (const DevVarKey &k : vk) by[put[k.region]++] = k;
        }
        for (size_t r = 0; r < B.regions.size(); r++)
            std::sort(by.begin() + at[r], by.begin() + at[r + 1],
                      [](const DevVarKey &x, const DevVarKey &y) { return x.j < y.j; });
        vk.swap(by);
    }
    B.var_off.assign(n_keys, UINT32_MAX);
    B.var_idx.assign(n_keys, UINT32_MAX);
    for (uint32_t i = 0; i < nk; i++) {
        const uint64_t k = (uint64_t)B.regions[vk[i].region].inner_off * B.n_slots + vk[i].j;
        B.var_off[k] = (uint32_t)vk[i].out_off;
        B.var_idx[k] = i;
    }
    B.var_keys = std::move(vk);
    // (a batch reduced before on another ctx: B.var_ctx moves here; that ctx drops B
    // as its owner when it next looks -- it checks B.var_ctx under B.var_mu)
    {  // the varying counts stay on the device until a host reader needs them
        std::lock_guard<std::mutex> g(B.var_mu);
        B.var_dev = ctx->asmb.var_counts.p;
        B.var_n = nc;
        B.var_device = ctx->device;
        B.var_ctx = ctx;
        B.var_host = false;
        B.var_err = 0;
    }
    ctx->asmb.var_owner = &B;
    B.enc_r0 = B.enc_r1 = 0;
    B.enc_idx.clear();
    B.reduced = true;
    return TFBS_OK;
}

}  // extern "C"

namespace tfbs {

int ensure_host_var_counts(const Batch &B) {
    std::lock_guard<std::mutex> g(B.var_mu);
    if (B.var_host) return B.var_err;
    Batch &M = const_cast<Batch &>(B);
    int rc = M.var_counts.reserve(std::max<size_t>(B.var_n * 4, 1));
    if (!rc && B.var_n) {
        int dev = -1;
        (void)hipGetDevice(&dev);
        const hipError_t e = hipSetDevice(B.var_device);
        const hipError_t c = e == hipSuccess ? hipMemcpy(M.var_counts.p, B.var_dev, B.var_n * 4, hipMemcpyDeviceToHost) : e;
        if (dev >= 0) (void)hipSetDevice(dev);
        if (c != hipSuccess) rc = fail(TFBS_E_HIP, std::string("varying counts download: ") + hipGetErrorString(c));
    }
    M.var_host = true;
    M.var_err = rc;
    M.var_dev = nullptr;
    return rc;
}

void forget_var_counts(Batch &B) {
    if (B.var_ctx && B.var_ctx->asmb.var_owner == &B) B.var_ctx->asmb.var_owner = nullptr;
    B.var_ctx = nullptr;
}

}  // namespace tfbs
