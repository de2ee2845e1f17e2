// The scan stage of the device context: the window-list build, the scan launch and its
// overflow loop, tfbs_batch_upload, tfbs_scan, tfbs_batch_download and tfbs_matches.
#include "ctx.hpp"

using namespace tfbs;

// The scan's counters (reference hits per region, the overflow pair) and the
// assembly's (asm_ctr) zeroed in one launch at the scan's start, instead of three
// memsets on either side of it (C2 is launch-bound).
__global__ void zero3_kernel(uint32_t *__restrict__ a, uint32_t na, uint32_t *__restrict__ b, uint32_t nb,
                             uint32_t *__restrict__ c, uint32_t nc) {
    const uint32_t s = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < na || k < nb || k < nc; k += s) {
        if (k < na) a[k] = 0;
        if (k < nb) b[k] = 0;
        if (k < nc) c[k] = 0;
    }
}

// The scan's unit for a batch of n_groups haplotype groups (ScanArgs::unit): a
// unit pays a super tile image's staging once for its G groups and hands their window
// pairs to its waves from one pool, but G times fewer workgroups fill the chip worse --
// the largest G of 4, 2, 1 whose units still give the chip's workgroup slots (two per
// CU) one and a half workgroups each in turn ("Units": the sweep behind the
// number -- units paid from 1.85 rounds up and not at 0.96 or below).  And only where a
// group's list is short: a group's list of either depth class holds at most kUnitPairs
// pairs of window tiles on average, two per wave (C5's groups hold 38: their waves scan
// for longer than an image takes to stage and are balanced without the pool; units of two
// or four neither gained nor lost there beyond the runs' spread).
constexpr uint32_t kUnitPairs = 2 * kMBlockWaves;
static uint32_t scan_unit_for(const tfbs_ctx *ctx, uint32_t n_groups) {
    if (ctx->knobs.scan_unit_env) return ctx->knobs.scan_unit_env;
    for (int c = 0; c < 2; c++)
        if (ctx->lists.wl_entries[c] > (uint64_t)kUnitPairs * 64 * n_groups) return 1;
    for (uint32_t G = kMMaxUnit; G > 1; G /= 2)
        if (2 * (uint64_t)((n_groups + G - 1) / G) >= 3 * (uint64_t)(2 * ctx->n_cus)) return G;
    return 1;
}

// The matrix-core window lists of the haplotypes just put on the device (one
// per depth class the plan has; scan.hpp build_window_lists).
// B: the batch whose haplotypes they are -- its windows are shared among the region's
// haplotypes (window_lists.hip "Shared windows") unless TFBS_SHARE=0, read here --, or
// null (a single haplotype: nothing to share).
int tfbs::build_lists(tfbs_ctx *ctx, uint32_t n_haps, const std::vector<uint8_t> &narrow, Batch *B) {
    const Plan &P = ctx->plan;
    ctx->lists.wl_share = false;
    ctx->lists.wl_n_haps = n_haps;
    for (int c = 0; c < 2; c++) ctx->lists.sh_entries[c] = ctx->lists.sh_listed[c][0] = ctx->lists.sh_listed[c][1] = 0;
    if (B) B->lists_counted = false;
    int rc;
    {  // key_fast_kernel's static records of the haplotypes and regions just put on the device
        const uint32_t nr = B ? (uint32_t)B->regions.size() : 1u;
        if ((rc = ctx->img.hap_reuse.ensure(std::max<uint32_t>(n_haps, 1))) ||
            (rc = ctx->img.region_asm.ensure(std::max<uint32_t>(nr, 1))) ||
            (rc = launch_region_asm(ctx->img.haps.p, n_haps, ctx->img.regions.p, nr, ctx->img.hap_reuse.p,
                                    ctx->img.region_asm.p, ctx->stream)))
            return rc;
    }
    if (P.m_supers.empty()) return TFBS_OK;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t lmin[2] = {0, 0}, span[2] = {0, 0};  // per depth class: shortest and longest strand
    for (const DevMSuper &S : P.m_supers) {
        uint32_t &l = lmin[S.nk > 2 ? 1 : 0];
        l = l ? std::min(l, S.lmin) : S.lmin;
        span[S.nk > 2 ? 1 : 0] = std::max(span[S.nk > 2 ? 1 : 0], S.lmax);
    }
    for (int c = 0; c < 2; c++)
        if (lmin[c] && (rc = ctx->lists.wl_off[c].ensure((size_t)n_haps + 1))) return rc;
    if ((rc = ctx->lists.wl_tmp.ensure(scan_tmp_words((size_t)n_haps + 1))) ||
        (rc = ctx->img.druns.ensure(std::max<size_t>(ctx->img.druns.n, 1))))
        return rc;
    if ((rc = ctx->lists.gnarrow.put(narrow, ctx->stream))) return rc;
    WindowListBufs bufs{};
    for (int c = 0; c < 2; c++) {
        bufs.off[c] = lmin[c] ? ctx->lists.wl_off[c].p : nullptr;
        bufs.list[c] = nullptr;
        bufs.list16[c] = nullptr;
    }
    bufs.gnarrow = narrow.empty() ? nullptr : ctx->lists.gnarrow.p;
    if ((rc = ctx->lists.hd.ensure(std::max<uint32_t>(n_haps, 1))) || (rc = ctx->lists.hd2.ensure(std::max<uint32_t>(n_haps, 1))))
        return rc;
    bufs.hd = ctx->lists.hd.p;
    bufs.hd2 = ctx->lists.hd2.p;
    bufs.scan_tmp = ctx->lists.wl_tmp.p;
    // a group's entries are all in one of the two lists (16-bit: a narrow group), both
    // indexed by the same offsets: a list no group uses gets no room
    ctx->lists.wl_any_narrow = ctx->lists.wl_any_wide = false;
    for (uint8_t g : narrow) (g ? ctx->lists.wl_any_narrow : ctx->lists.wl_any_wide) = true;
    if (narrow.empty()) ctx->lists.wl_any_wide = true;
    auto ensure = [](void *x, int c, uint64_t n, uint32_t **p, uint16_t **p16) {
        tfbs_ctx *cx = static_cast<tfbs_ctx *>(x);
        if (int e = cx->lists.wl[c].ensure(cx->lists.wl_any_wide ? n : 1)) return e;
        if (int e = cx->lists.wl16[c].ensure(cx->lists.wl_any_narrow ? n : 1)) return e;
        *p = cx->lists.wl[c].p;
        *p16 = cx->lists.wl16[c].p;
        return TFBS_OK;
    };
    const bool share = B && B->dedup && n_haps && env_int("TFBS_SHARE", 1) != 0;
    std::vector<std::pair<uint32_t, uint32_t>> rest;  // (length, strands) the matrix cores do not score
    if (share) {
        // the strand lengths of each depth class (a tile's class is its longest strand's):
        // per columns left, the strands a listed window is scored for and their cells
        std::vector<ClassTab> tab(2, ClassTab{});
        rest = B->pwm_len_hist;
        for (size_t t = 0; t * kGMetaInts < P.m_meta.size(); t++) {
            const int32_t *gm = &P.m_meta[t * kGMetaInts];
            ClassTab &ct = tab[gm[kGDepth] > 2];
            for (int sn = 0; sn < kMStrands; sn++) {
                if (gm[kGOrig + sn] < 0) continue;  // tile padding
                const uint32_t L = (uint32_t)gm[kGStrandInts * sn + kGLen];
                for (uint32_t r = L; r <= 32; r++) ct.w[r] += 1, ct.c[r] += L;
                for (auto &lc : rest)
                    if (lc.first == L && lc.second) lc.second--;
            }
        }
        if ((rc = ctx->lists.sh_tab.put(tab, ctx->stream)) || (rc = ctx->lists.sh_stat.ensure(4)) ||
            (rc = ctx->lists.sh_cur.ensure(2 * (size_t)n_haps)))
            return rc;
        for (int c = 0; c < 2; c++)
            if (lmin[c] && (rc = ctx->lists.sh_off[c].ensure((size_t)n_haps + 1))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // (tab is copied from this scope)
        for (int c = 0; c < 2; c++) bufs.soff[c] = lmin[c] ? ctx->lists.sh_off[c].p : nullptr;
        bufs.scur = ctx->lists.sh_cur.p;
        bufs.stat = ctx->lists.sh_stat.p;
    }
    auto ensure_share = [](void *x, int c, uint64_t n, uint2 **p) {
        tfbs_ctx *cx = static_cast<tfbs_ctx *>(x);
        if (int e = cx->lists.sh[c].ensure(n)) return e;
        *p = cx->lists.sh[c].p;
        return TFBS_OK;
    };
    if ((rc = build_window_lists(ctx->img.haps.p, n_haps, ctx->img.druns.p, lmin, span, ctx->knobs.mfma_hpb, 1, bufs, ctx->lists.wl_entries,
                                 ctx->stream, ensure, ctx, share ? 1u : 0u, ctx->img.regions.p, ctx->img.words.p, ctx->lists.sh_tab.p,
                                 ensure_share, ctx->lists.sh_entries, ctx->lists.sh_listed)))
        return rc;
    ctx->lists.wl_share = share;
    if (share) {  // the scan statistics from what the lists hold (+ the other kernels' strands: every window)
        B->list_windows = ctx->lists.sh_listed[0][0] + ctx->lists.sh_listed[1][0];
        B->list_cell_ops = ctx->lists.sh_listed[0][1] + ctx->lists.sh_listed[1][1];
        for (const auto &lc : rest) {
            if (!lc.second) continue;
            uint64_t nw = 0;
            for (const DevHap &h : B->haps) nw += h.len >= lc.first ? h.len - lc.first + 1 : 0;
            B->list_windows += nw * lc.second;
            B->list_cell_ops += nw * lc.second * lc.first;
        }
        B->lists_counted = true;
    }
    for (int c = 0; c < 2; c++)
        if (!lmin[c]) ctx->lists.wl_off[c].release(), ctx->lists.wl[c].release(), ctx->lists.wl16[c].release();
    // The scan's workgroup order: groups by descending work (window pairs x the
    // per-pair MFMAs + rounds of each depth class's super tiles), so that the launch
    // ends on its smallest groups instead of a late large one (LPT).
    ctx->lists.gorder.release();
    ctx->lists.scan_unit = scan_unit_for(ctx, (n_haps + ctx->knobs.mfma_hpb - 1) / ctx->knobs.mfma_hpb);
    if (env_int("TFBS_SCAN_LPT", 1) && n_haps) {
        uint32_t w[2] = {0, 0};
        for (const DevMSuper &S : P.m_supers) {
            uint32_t prev = 0;
            for (uint32_t d = 1; d <= 4; d++) {
                const uint32_t e = (S.seg >> (8 * (d - 1))) & 255u;
                if (e > prev) w[S.nk > 2 ? 1 : 0] += (e - prev) * (2 * d + 1);
                prev = std::max(prev, e);
            }
        }
        const uint32_t hpb = ctx->knobs.mfma_hpb, ng = (n_haps + hpb - 1) / hpb;
        if ((rc = ctx->lists.gcost.ensure(ng)) ||
            (rc = group_costs(lmin[0] ? ctx->lists.wl_off[0].p : nullptr, lmin[1] ? ctx->lists.wl_off[1].p : nullptr, n_haps, hpb,
                              w[0], w[1], ctx->lists.gcost.p, ctx->stream)))
            return rc;
        // (the order holds units: a unit's cost is the sum of its groups')
        const uint32_t G = ctx->lists.scan_unit, nu = (ng + G - 1) / G;
        std::vector<uint32_t> cost(ng), order(nu);
        HIP_TRY(hipMemcpyAsync(cost.data(), ctx->lists.gcost.p, (size_t)ng * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        std::vector<uint64_t> ucost(nu, 0);
        for (uint32_t g = 0; g < ng; g++) ucost[g / G] += cost[g];
        for (uint32_t u = 0; u < nu; u++) order[u] = u;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ucost[a] > ucost[b]; });
        if ((rc = ctx->lists.gorder.put(order, ctx->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // (order is copied from the host's stack)
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->lists.wl_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return TFBS_OK;
}

int tfbs::launch_scan(tfbs_ctx *ctx, uint32_t n_haps, unsigned long long *hits, uint32_t hits_wpp) {
    const Plan &P = ctx->plan;
    if (n_haps == 0) return 0;
    ScanArgs a{};
    a.haps = ctx->img.haps.p;
    a.n_haps = n_haps;
    a.hap_base = 0;
    a.regions = ctx->img.regions.p;
    a.inner = ctx->img.inner.p;
    a.words = ctx->img.words.p;
    a.nmask = ctx->img.nmask.p;
    a.posrel = ctx->img.posrel.p;
    a.counts = ctx->img.counts_live ? ctx->img.counts.p : nullptr;
    a.haps_per_block = ctx->knobs.haps_per_block;
    a.hits = hits;
    a.hits_wpp = hits_wpp;
    a.n_patterns_total = (uint32_t)ctx->pats->pats.size();
    int launches = 0;
    if (!P.m_supers.empty()) {  // sparse hits: no count matrix to zero
        ScanArgs m = a;
        m.msupers = ctx->tabs.m_supers.p;
        m.n_msupers = (uint32_t)P.m_supers.size();
        m.mimage = ctx->tabs.m_image.p;
        m.mweights = ctx->tabs.m_weights.p;
        m.mmeta = ctx->tabs.m_meta.p;
        m.haps_per_block = ctx->knobs.mfma_hpb;
        // one candidate list and one hit list per haplotype group (a workgroup scans its
        // groups against every super tile: their lists hold the candidates of all of them)
        const uint64_t n_groups = (n_haps + ctx->knobs.mfma_hpb - 1) / ctx->knobs.mfma_hpb;
        const uint32_t cand_cap = (uint32_t)std::min<uint64_t>(1u << 16, (uint64_t)ctx->knobs.cand_cap * P.m_supers.size());
        // (shared windows: a donor's wave lists its sharers' pairs too -- at C3 a per-wave share
        // of cand_cap / 8 sent 152 000 of 4.27 M pairs to the spill list)
        const uint32_t hit_cap = (uint32_t)std::min<uint64_t>(1u << 16, (uint64_t)cand_cap * (ctx->lists.wl_share ? 4 : 1));
        int rc;
        if ((rc = ctx->scan.cands.ensure(n_groups * cand_cap * kCandWords)) || (rc = ctx->scan.hitl.ensure(n_groups * hit_cap * 2)) ||
            (rc = ctx->scan.hitn.ensure(n_groups * (kMBlockWaves))) || (rc = ctx->scan.candn.ensure(n_groups * (kMBlockWaves))))
            return rc;
        m.cands = ctx->scan.cands.p;
        m.cand_cap = cand_cap;
        ctx->scan.scan_cand_cap = cand_cap;
        ctx->scan.scan_hit_cap = hit_cap;
        m.hit_cap = hit_cap;
        m.hitl = ctx->scan.hitl.p;
        m.hitn = ctx->scan.hitn.p;
        m.candn = ctx->scan.candn.p;
        const uint32_t nr = std::max<uint32_t>(1, ctx->img.n_regions);
        if ((rc = ctx->scan.ref_count.ensure(nr)) || (rc = ctx->scan.ref_hits.ensure((size_t)nr * kRefPerRegion * 2)) ||
            (rc = ctx->scan.over.ensure(2)) || (rc = ctx->scan.spill.ensure((size_t)ctx->scan.spill_cap * 3)) ||
            (rc = ctx->scan.cand_over.ensure((size_t)ctx->scan.cand_over_cap * 3)) ||
            (rc = ctx->scan.spill_sorted.ensure((size_t)ctx->scan.spill_cap * 3)) || (rc = ctx->scan.spill_bcnt.ensure(nr + 1)) ||
            (rc = ctx->scan.spill_boff.ensure(nr + 1)))
            return rc;
        m.dedup = 1;
        m.gnarrow = ctx->lists.gnarrow.n ? ctx->lists.gnarrow.p : nullptr;
        m.gorder = ctx->lists.gorder.n ? ctx->lists.gorder.p : nullptr;
        m.unit = ctx->lists.scan_unit;  // (gorder holds units of as many groups)
        m.unit_words = ctx->knobs.scan_unit_words_env;
        m.hd = ctx->lists.hd.p;
        m.hd2 = ctx->lists.hd2.p;
        m.druns = ctx->img.druns.p;
        m.n_regions = ctx->img.n_regions;
        m.ref_hits = ctx->scan.ref_hits.p;
        m.ref_count = ctx->scan.ref_count.p;
        m.spill = ctx->scan.spill.p;
        m.over = ctx->scan.over.p;
        m.spill_cap = ctx->scan.spill_cap;
        m.cand_over = ctx->scan.cand_over.p;
        m.cand_over_cap = ctx->scan.cand_over_cap;
        static const char *prof_path = getenv("TFBS_SCAN_PROF");
        if (prof_path && *prof_path) {
            if ((rc = ctx->scan.scan_prof.ensure(n_groups * kMBlockWaves * kScanProfWords))) return rc;
            HIP_TRY(hipMemsetAsync(ctx->scan.scan_prof.p, 0, ctx->scan.scan_prof.n * 8, ctx->stream));
            m.prof = ctx->scan.scan_prof.p;
        }
        for (int c = 0; c < 2; c++) {
            m.wlist[c] = ctx->lists.wl[c].p;
            m.wlist16[c] = ctx->lists.wl16[c].p;
            m.wlist_off[c] = ctx->lists.wl_off[c].p;
            const bool sh = ctx->lists.wl_share && ctx->lists.wl_off[c].p && ctx->lists.sh_entries[c];
            m.share_off[c] = sh ? ctx->lists.sh_off[c].p : nullptr;
            m.share[c] = sh ? ctx->lists.sh[c].p : nullptr;
        }
        {
            const uint32_t na = (uint32_t)(kAsmCtrWords + asm_bucket_words(nr));
            if ((rc = ctx->asmb.asm_ctr.ensure(na))) return rc;
            hipLaunchKernelGGL(zero3_kernel, dim3(std::min<uint32_t>(256, (std::max(na, nr) + 255) / 256)), dim3(256), 0,
                               ctx->stream, ctx->scan.ref_count.p, nr, ctx->scan.over.p, 2u, ctx->asmb.asm_ctr.p, na);
            HIP_TRY(hipGetLastError());
            ctx->asmb.asm_ctr_zeroed = true;  // (for this scan's first assembly)
        }
        // the post-scan work in the scan's last workgroup when the assembly that follows
        // (tfbs_step) would launch it lean: neither the grid-wide bucketing nor overflow
        // candidates last time (it handles both anyway: too many spill records set
        // need_wide, and the assembly reruns with the wide kernels) -- unless that assembly
        // leaves the stage out altogether
        ctx->scan.post_fused = ctx->scan.post_fuse_ok && ctx->knobs.post_fuse_env && ctx->knobs.asm_lean_mode != 0 &&
                          !ctx->asmb.asm_full && (ctx->knobs.asm_lean_mode == 2 || ctx->asmb.prev_spill <= kPostSerial) &&
                          ctx->asmb.prev_cand == 0 && !asm_skips_post(ctx);
        if (ctx->scan.post_fused) {
            m.post_done = ctx->asmb.asm_ctr.p + kCtrPostDone;
            m.post_regions = nr;
            m.post_bcnt = ctx->asmb.asm_ctr.p + kAsmCtrWords;
            m.post_boff = ctx->scan.spill_boff.p;
            m.post_sorted = ctx->scan.spill_sorted.p;
            m.post_report = ctx->asmb.asm_ctr.p;
            m.post_need_wide = ctx->asmb.asm_ctr.p + kCtrNeedWide;
        }
        if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->scan.evk0, ctx->stream));
        const int n = launch_mfma_all(m, P.m_supers.data(), (uint32_t)P.m_supers.size(), ctx->img.mfma_group_words, n_haps,
                                      ctx->stream);
        if (n < 0) return n;
        if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->scan.evk1, ctx->stream));
        ctx->scan.kernel_timed = true;
        launches += n;
        if (m.prof) {  // (profiling runs only) the stamps, appended to the file: launches, then the waves
            std::vector<unsigned long long> h(ctx->scan.scan_prof.n);
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipMemcpy(h.data(), ctx->scan.scan_prof.p, h.size() * 8, hipMemcpyDeviceToHost));
            if (FILE *f = fopen(prof_path, "ab")) {
                unsigned long long hdr[2] = {(unsigned long long)n, h.size()};
                fwrite(hdr, 8, 2, f);
                for (uint64_t i = 0, g0 = 0; g0 < n_groups; i++, g0 += kMLaunchGroups) {
                    // one row per launch: its first list slot, lists per group, first group, groups
                    unsigned long long v[5] = {g0, 1, g0, std::min<uint64_t>(kMLaunchGroups, n_groups - g0), i};
                    fwrite(v, 8, 5, f);
                }
                fwrite(h.data(), 8, h.size(), f);
                fclose(f);
            }
        }
        ctx->scan.last_margs = m;  // the overflow candidates are rescored when the results are read (check_overflow)
        ctx->scan.post_done = false;
        // the overflow counters are checked before the results are read: by the
        // assembly's list pass, or by check_overflow (which copies them back first)
        ctx->scan.over_pending = true;
        ctx->scan.over_copied = false;
    }
    if (!P.fast_tiles.empty()) {
        ScanArgs f = a;
        f.tiles = ctx->tabs.fast_tiles.p;
        f.n_tiles = (uint32_t)P.fast_tiles.size();
        f.units = ctx->tabs.fast_units.p;
        f.lut = ctx->tabs.lut.p;
        f.wfull = ctx->tabs.wfull.p;
        const int n = launch_fast(f, ctx->cfg, n_haps, ctx->stream);
        if (n < 0) return n;
        launches += n;
    }
    if (!P.gen_tiles.empty()) {
        ScanArgs g = a;
        g.tiles = ctx->tabs.gen_tiles.p;
        g.n_tiles = (uint32_t)P.gen_tiles.size();
        g.gpats = ctx->tabs.gen_pats.p;
        g.gw = ctx->tabs.gen_w.p;
        const int n = launch_generic(g, n_haps, ctx->stream);
        if (n < 0) return n;
        launches += n;
    }
    if (!P.di_tiles.empty()) {
        ScanArgs d = a;
        d.tiles = ctx->tabs.di_tiles.p;
        d.n_tiles = (uint32_t)P.di_tiles.size();
        d.units = ctx->tabs.di_units.p;
        d.lut = ctx->tabs.di_lut.p;
        d.wfull = ctx->tabs.di_w.p;
        const int n = launch_dinuc(d, (size_t)P.max_di_tile_blocks * kDiBlockBytes, n_haps, ctx->stream);
        if (n < 0) return n;
        launches += n;
    }
    return launches;
}

// The last scan's overflow lists must have held every entry (a dropped
// candidate may hide a hit, a dropped spill record is a lost count): read the
// counters copied back after it and, if one overflowed, grow the lists and scan
// again.  Then the candidates past the waves' lists are rescored (their hits
// join the spill list) and the spill records bucketed by region -- work only
// when there is any.  Runs before anything reads the scan's results.
int tfbs::check_overflow(tfbs_ctx *ctx, uint32_t n_haps, unsigned long long *hits, uint32_t wpp) {
    for (int round = 0; ctx->scan.over_pending; round++) {
        if (round == 8) return tfbs::fail(TFBS_E_NOMEM, "scan overflow lists still full after 8 rescans");
        if (!ctx->scan.over_copied) {  // (the scan's counters: nothing after it on the stream changes them)
            if (!ctx->scan.over_host) HIP_TRY(ctx->scan.over_host.alloc(2));
            HIP_TRY(hipMemcpyAsync(ctx->scan.over_host.p, ctx->scan.over.p, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipEventRecord(ctx->scan.over_ev, ctx->stream));
            ctx->scan.over_copied = true;
        }
        HIP_TRY(hipEventSynchronize(ctx->scan.over_ev));
        uint32_t nspill = ctx->scan.over_host[0];
        const uint32_t ncand = ctx->scan.over_host[1];
        if (ncand > 0 && ncand <= ctx->scan.cand_over_cap && !ctx->scan.post_done) {  // rescore them: their hits add spill records
            const int f = launch_post_scan(ctx->scan.last_margs, ctx->stream);
            if (f < 0) return f;
            HIP_TRY(hipMemcpyAsync(ctx->scan.over_host.p, ctx->scan.over.p, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            nspill = ctx->scan.over_host[0];
        }
        if (ctx->knobs.debug_over) {
            fprintf(stderr, "tfbs_scan overflow lists: spill %u/%u candidates %u/%u\n", nspill, ctx->scan.spill_cap, ncand,
                    ctx->scan.cand_over_cap);
            // the hits of the scan workgroups' lists
            const size_t nw = ctx->scan.hitn.n;
            std::vector<uint32_t> hn(nw);
            HIP_TRY(hipMemcpy(hn.data(), ctx->scan.hitn.p, nw * 4, hipMemcpyDeviceToHost));
            uint64_t sh = 0, mh = 0;
            for (size_t i = 0; i < nw; i++) sh += hn[i], mh = std::max<uint64_t>(mh, hn[i]);
            fprintf(stderr, "tfbs_scan hit pairs %llu (max per wave %llu) over %zu waves\n", (unsigned long long)sh,
                    (unsigned long long)mh, nw);
        }
        if (nspill <= ctx->scan.spill_cap && ncand <= ctx->scan.cand_over_cap) {
            ctx->scan.over_pending = false;
            ctx->scan.post_done = true;
            if (nspill) {
                const uint32_t nr = std::max<uint32_t>(1, ctx->img.n_regions);
                const int rc = launch_spill_buckets(ctx->scan.over.p, ctx->scan.spill_cap, ctx->scan.spill.p, nr, ctx->scan.spill_bcnt.p,
                                                    ctx->scan.spill_boff.p, ctx->scan.spill_sorted.p, ctx->stream);
                if (rc) return rc;
                ctx->scan.spill_cnt_ctr = false;  // (spill_bcnt: its fill counters end at the counts)
            }
            return TFBS_OK;
        }
        grow_cap(ctx->scan.spill_cap, ncand > ctx->scan.cand_over_cap ? 2 * std::max(nspill, 1024u) : nspill, UINT32_MAX / 4);
        grow_cap(ctx->scan.cand_over_cap, ncand, UINT32_MAX / 4);
        const int n = launch_scan(ctx, n_haps, hits, wpp);
        if (n < 0) return n;
    }
    return TFBS_OK;
}

extern "C" {

int tfbs_ctx_group_pairs(tfbs_ctx *ctx, int cls, uint32_t *pairs, size_t cap, size_t *n_groups) {
    if (!ctx || !n_groups || cls < 0 || cls > 1 || (cap && !pairs)) return tfbs::fail(TFBS_E_ARG, "bad argument");
    const uint32_t n = ctx->lists.wl_n_haps, hpb = ctx->knobs.mfma_hpb;
    *n_groups = ((size_t)n + hpb - 1) / hpb;
    if (*n_groups > cap) return cap ? tfbs::fail(TFBS_E_ARG, "group pairs: the array is too small") : TFBS_OK;
    if (!ctx->lists.wl_off[cls].p) {  // no super tile of the class: no list
        for (size_t g = 0; g < *n_groups; g++) pairs[g] = 0;
        return TFBS_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint64_t> off((size_t)n + 1);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(off.data(), ctx->lists.wl_off[cls].p, off.size() * 8, hipMemcpyDeviceToHost));
    for (size_t g = 0; g < *n_groups; g++) {
        const uint64_t nw = off[std::min<size_t>((g + 1) * hpb, n)] - off[g * hpb];
        pairs[g] = (uint32_t)(((nw + 31) / 32 + 1) / 2);
    }
    return TFBS_OK;
}

int tfbs_ctx_share_entries(tfbs_ctx *ctx, int cls, uint32_t *entries, size_t cap, size_t *n_haps) {
    if (!ctx || !n_haps || cls < 0 || cls > 1 || (cap && !entries)) return tfbs::fail(TFBS_E_ARG, "bad argument");
    const uint32_t n = ctx->lists.wl_n_haps;
    *n_haps = n;
    if (n > cap) return cap ? tfbs::fail(TFBS_E_ARG, "share entries: the array is too small") : TFBS_OK;
    // (as the scan takes them, launch_scan: shared lists, a list of the class, an entry in it)
    if (!ctx->lists.wl_share || !ctx->lists.wl_off[cls].p || !ctx->lists.sh_entries[cls]) {
        for (size_t h = 0; h < n; h++) entries[h] = 0;
        return TFBS_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint64_t> off((size_t)n + 1);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(off.data(), ctx->lists.sh_off[cls].p, off.size() * 8, hipMemcpyDeviceToHost));
    for (size_t h = 0; h < n; h++) entries[h] = (uint32_t)(off[h + 1] - off[h]);
    return TFBS_OK;
}

int tfbs_ctx_region_asm(tfbs_ctx *ctx, uint32_t *region_asm, size_t cap_regions, uint32_t *hap_reuse, size_t cap_haps,
                        size_t *n_regions, size_t *n_haps) {
    if (!ctx || !n_regions || !n_haps || (cap_regions && !region_asm) || (cap_haps && !hap_reuse))
        return tfbs::fail(TFBS_E_ARG, "bad argument");
    *n_regions = ctx->img.n_regions;
    *n_haps = ctx->lists.wl_n_haps;
    if (!cap_regions && !cap_haps) return TFBS_OK;
    if (*n_regions > cap_regions || *n_haps > cap_haps) return tfbs::fail(TFBS_E_ARG, "region asm: the arrays are too small");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (*n_regions) HIP_TRY(hipMemcpy(region_asm, ctx->img.region_asm.p, *n_regions * 16, hipMemcpyDeviceToHost));
    if (*n_haps) HIP_TRY(hipMemcpy(hap_reuse, ctx->img.hap_reuse.p, *n_haps * 4, hipMemcpyDeviceToHost));
    return TFBS_OK;
}

int tfbs_batch_upload(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    Batch &B = b->b;
    if (B.pats != ctx->pats) return tfbs::fail(TFBS_E_ARG, "batch and ctx use different pattern sets");
    if (B.open) return tfbs::fail(TFBS_E_STATE, "region still open");
    if (B.slot_pid != ctx->plan.slot_pid) return tfbs::fail(TFBS_E_STATE, "batch slot order differs from the ctx plan");
    HIP_TRY(hipSetDevice(ctx->device));
    // key assembly scratch for regions of more distinct haplotypes than its LDS block holds
    uint64_t big = 0;
    for (DevRegion &rg : B.regions) {
        rg.big_off = big;
        if (rg.hap_count > key_asm_lds_counters()) big += rg.hap_count;
    }
    // dense counts only for the LUT / generic kernels' slots (they store theirs)
    const bool dense = !ctx->plan.fast_tiles.empty() || !ctx->plan.gen_tiles.empty() || !ctx->plan.di_tiles.empty();
    int rc;
    if ((rc = ctx->img.words.put(B.words, ctx->stream)) || (rc = ctx->img.nmask.put(B.nmask, ctx->stream)) ||
        (rc = ctx->img.posrel.put(B.posrel, ctx->stream)) || (rc = ctx->img.haps.put(B.haps, ctx->stream)) ||
        (rc = ctx->img.druns.put(B.druns, ctx->stream)) ||
        (rc = ctx->img.regions.put(B.regions, ctx->stream)) || (rc = ctx->img.inner.put(B.inner, ctx->stream)) ||
        (rc = ctx->asmb.asm_scratch.ensure(std::max<uint64_t>(big, 1))) ||
        (dense && (rc = ctx->img.counts.ensure(std::max<uint64_t>(B.n_counts, 1)))))
        return rc;
    std::vector<uint32_t> order(B.regions.size());  // (alive until the stream sync below)
    {  // key_fast_kernel's region order: most distinct haplotypes first (their workgroups run longest)
        for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            return B.regions[x].hap_count > B.regions[y].hap_count;
        });
        if ((rc = ctx->asmb.asm_order.put(order, ctx->stream))) return rc;
        ctx->asmb.asm_order_n = (uint32_t)order.size();
        ctx->asmb.asm_order_big = 0;
        const int big_u = ctx->knobs.kf_big_u;
        while (big_u > 0 && ctx->asmb.asm_order_big < order.size() &&
               B.regions[order[ctx->asmb.asm_order_big]].hap_count > (uint32_t)big_u)
            ctx->asmb.asm_order_big++;
    }
    std::vector<uint8_t> narrow((B.haps.size() + ctx->knobs.mfma_hpb - 1) / ctx->knobs.mfma_hpb, 1);  // (alive until the sync)
    for (size_t h = 0; h < B.haps.size(); h++)
        if (B.haps[h].len > kWlNarrowLen) narrow[h / ctx->knobs.mfma_hpb] = 0;
    if ((rc = build_lists(ctx, (uint32_t)B.haps.size(), narrow, &B))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->img.counts_live = dense;
    ctx->img.resident = b;
    ctx->img.upload_gen++;
    ctx->asmb.prev_spill = ctx->asmb.prev_redo = ctx->asmb.prev_cand = UINT32_MAX;
    ctx->img.mfma_group_words = mfma_group_words(B.haps.data(), (uint32_t)B.haps.size(), ctx->knobs.mfma_hpb);
    ctx->img.n_regions = (uint32_t)B.regions.size();
    ctx->scan.over_pending = false;
    ctx->scan.scanned = false;
    ctx->asmb.asm_state = 0;
    return TFBS_OK;
}

int tfbs_scan(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not uploaded to this ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->scan.ev0, ctx->stream));
    ctx->scan.kernel_timed = false;
    // asynchronous: the overflow lists are checked (and the scan redone if one
    // overflowed) when its results are read (tfbs_batch_reduce / download)
    const int n = launch_scan(ctx, (uint32_t)b->b.haps.size(), nullptr, 0);
    if (n < 0) return n;
    ctx->scan.scanned = true;
    ctx->asmb.asm_state = 0;
    if (!ctx->step.capturing) HIP_TRY(hipEventRecord(ctx->scan.ev1, ctx->stream));
    ctx->scan.last_launches = n;
    ctx->scan.timing_pending = true;
    b->b.counts_valid = b->b.reduced = false;
    b->b.enc_r0 = b->b.enc_r1 = 0;
    return TFBS_OK;
}

int tfbs_batch_download(tfbs_ctx *ctx, tfbs_batch *b) {
    if (!ctx || !b) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not resident on this ctx");
    if (!ctx->scan.scanned) return tfbs::fail(TFBS_E_STATE, "batch not scanned (tfbs_scan)");
    HIP_TRY(hipSetDevice(ctx->device));
    Batch &B = b->b;
    int rc;
    if (ctx->asmb.asm_state == 1 && ctx->asmb.asm_batch == &B && (rc = assembly_wait(ctx, B))) return rc;
    if ((rc = check_overflow(ctx, (uint32_t)B.haps.size()))) return rc;
    if (!ctx->img.counts_live) {  // no LUT/generic slots: the matrix is the assembly's alone
        if ((rc = ctx->img.counts.ensure(std::max<uint64_t>(B.n_counts, 1)))) return rc;
    }
    AsmArgs a = asm_args(ctx, B, 1);
    // (a scan whose checked assembly left the post-scan stage out and read its few records in
    // place -- no candidate, so check_overflow had nothing to do --: no buckets, the same reading)
    if (a.spill_count && !ctx->scan.post_done && !ctx->asmb.stages.post && ctx->asmb.stages.inplace) {
        a.spill_raw = ctx->scan.spill.p;
        a.spill_inplace = ctx->asmb.stages.inplace;
    }
    a.counts = ctx->img.counts.p;
    a.dense_base = 1;
    if ((rc = launch_key_asm(a, (uint32_t)B.regions.size(), ctx->stream))) return rc;
    B.counts.resize(B.n_counts);
    if (B.n_counts)
        HIP_TRY(hipMemcpyAsync(B.counts.data(), ctx->img.counts.p, B.n_counts * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    B.counts_valid = true;
    return TFBS_OK;
}

int tfbs_matches(tfbs_ctx *ctx, const uint8_t *nucs, const uint64_t *pos, size_t n, uint32_t *counts,
                 uint64_t *out_start, uint64_t *out_end, size_t cap, size_t *n_total) {
    if (!ctx || !n_total || !counts || (n && (!nucs || !pos))) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (n >= kMaxHapLen) return tfbs::fail(TFBS_E_ARG, "haplotype longer than 2^26 - 1 bases");
    const Patterns &P = *ctx->pats;
    // pack one haplotype; no inner ranges, hit bitmaps only
    std::vector<uint32_t> words((n + 15) / 16 + 3, 0u), nmask;
    bool has_n = false;
    for (size_t i = 0; i < n; i++) {
        if (nucs[i] > 4) return tfbs::fail(TFBS_E_BADBASE, "nucleotide code > 4");
        uint32_t c = nucs[i];
        if (c == 4) {
            has_n = true;
            c = 0;
        }
        words[i / 16] |= c << (2 * (i % 16));
    }
    DevHap hm{};
    hm.len = (uint32_t)n;
    if (has_n) {
        hm.flags |= HAP_HAS_N;
        nmask.assign((n + 31) / 32 + 2, 0u);
        for (size_t i = 0; i < n; i++)
            if (nucs[i] == 4) nmask[i / 32] |= 1u << (i % 32);
    }
    std::vector<DevHap> haps{hm};
    std::vector<DevRegion> regions{DevRegion{0, 0, 0, 1, UINT32_MAX, 1, 0}};
    std::vector<int32_t> inner{0, 0}, posrel{0};
    ctx->asmb.asm_order_n = 0;  // (this one-haplotype upload replaces the resident batch)
    const uint32_t wpp = (uint32_t)((n + 255) / 256 * 4);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    if ((rc = ctx->img.words.put(words, ctx->stream)) || (rc = ctx->img.nmask.put(nmask, ctx->stream)) ||
        (rc = ctx->img.posrel.put(posrel, ctx->stream)) || (rc = ctx->img.haps.put(haps, ctx->stream)) ||
        (rc = ctx->img.regions.put(regions, ctx->stream)) || (rc = ctx->img.inner.put(inner, ctx->stream)) ||
        (rc = ctx->img.counts.ensure(std::max<uint64_t>(P.pats.size(), 1))) || (rc = ctx->img.druns.ensure(1)) ||
        (rc = build_lists(ctx, 1, std::vector<uint8_t>{(uint8_t)(n <= kWlNarrowLen)})))
        return rc;
    ctx->img.counts_live = true;
    ctx->img.resident = nullptr;
    ctx->scan.scanned = false;
    ctx->img.mfma_group_words = mfma_group_words(haps.data(), 1, ctx->knobs.mfma_hpb);
    ctx->img.n_regions = 1;
    const size_t nh = (size_t)P.pats.size() * wpp;
    if ((rc = ctx->scan.hits.ensure(std::max<size_t>(nh, 1)))) return rc;
    if (nh) HIP_TRY(hipMemsetAsync(ctx->scan.hits.p, 0, nh * 8, ctx->stream));
    int l = launch_scan(ctx, 1, ctx->scan.hits.p, wpp);
    if (l < 0) return l;
    if ((rc = check_overflow(ctx, 1, ctx->scan.hits.p, wpp))) return rc;  // a rescan (larger lists) sets the same bits again
    std::vector<unsigned long long> h(nh);
    if (nh) HIP_TRY(hipMemcpyAsync(h.data(), ctx->scan.hits.p, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    size_t total = 0;
    for (size_t pi = 0; pi < P.pats.size(); pi++) {
        const Pat &q = P.pats[pi];
        uint32_t c = 0;
        for (uint32_t w = 0; w < wpp; w++) {
            unsigned long long m = h[pi * wpp + w];
            while (m) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                const size_t i = (size_t)w * 64 + bit;
                if (total < cap) {
                    out_start[total] = pos[i];
                    out_end[total] = pos[i] + q.len - 1;
                }
                total++;
                c++;
            }
        }
        counts[pi] = c;
    }
    *n_total = total;
    if (total > cap) return tfbs::fail(TFBS_E_ARG, "output capacity too small");
    return TFBS_OK;
}


}  // extern "C"
