// The device context's lifecycle and its timer and counter getters (tfbs_device_count,
// tfbs_ctx_create / destroy / sync, tfbs_ctx_last_*).  The stages are in ctx_scan.hip,
// ctx_assembly.hip, ctx_encode.hip, ctx_rows.hip and ctx_outputs.hip; the kernels in their own units.
#include "ctx.hpp"

using namespace tfbs;

int tfbs::env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    if (!v || !*v) return dflt;
    return atoi(v);
}

extern "C" {

int tfbs_device_count(int *n) {
    if (!n) return tfbs::fail(TFBS_E_ARG, "null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c == 0) {
        *n = 0;
        return tfbs::fail(TFBS_E_NODEVICE, "no HIP device visible");
    }
    *n = c;
    return TFBS_OK;
}

void tfbs_ctx_destroy(tfbs_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->rows.rw.th.joinable()) {  // the jobs still queued go out first
        {
            std::lock_guard<std::mutex> l(ctx->rows.rw.mu);
            ctx->rows.rw.stop = true;
        }
        ctx->rows.rw.cv.notify_all();
        ctx->rows.rw.th.join();
        if (ctx->rows.rw.th2.joinable()) ctx->rows.rw.th2.join();
    }
    if (ctx->asmb.var_owner) {  // its varying counts to the host before var_counts goes
        (void)tfbs::ensure_host_var_counts(*ctx->asmb.var_owner);
        std::lock_guard<std::mutex> g(ctx->asmb.var_owner->var_mu);
        if (ctx->asmb.var_owner->var_ctx == ctx) ctx->asmb.var_owner->var_ctx = nullptr;
        ctx->asmb.var_owner = nullptr;
    }
    // the six lazily made driver states; everything else frees itself, in reverse order of
    // its declaration (ctx.hpp): the step graph, the stages' buffers and events, then the stream
    tfbs::hits_state_destroy(ctx->hits_state);
    tfbs::best_state_destroy(ctx->best_state);
    tfbs::scores_state_destroy(ctx->scores_state);
    tfbs::effects_state_destroy(ctx->effects_state);
    tfbs::mutscan_state_destroy(ctx->mutscan_state);
    tfbs::affinity_state_destroy(ctx->affinity_state);
    tfbs::affinity_rows_state_destroy(ctx->affinity_rows_state);
    delete ctx;
}

int tfbs_ctx_create(int device, const tfbs_patterns *p, tfbs_ctx **out) {
    if (!p || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    int n = 0;
    int rc = tfbs_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return tfbs::fail(TFBS_E_ARG, "device index out of range");
    std::unique_ptr<tfbs_ctx, decltype(&tfbs_ctx_destroy)> hold(new tfbs_ctx(), tfbs_ctx_destroy);  // (every failure exit)
    tfbs_ctx *ctx = hold.get();
    ctx->device = device;
    ctx->pats = &tfbs::patterns_of(p);
    ctx->cfg.minw = env_int("TFBS_FAST_MINW", 2) == 4 ? 4 : 2;
    ctx->asmb.cor_cap = (uint32_t)std::max(1, env_int("TFBS_KEY_COR_CAP", 1 << 22));
    ctx->enc.host_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    ctx->scan.cand_over_cap = (uint32_t)std::max(1, env_int("TFBS_CAND_OVER_CAP", 1 << 20));  // grows on demand (tfbs_scan)
    PlanOptions opt;
    opt.tile_blocks = ctx->knobs.tile_blocks;
    opt.mfma = ctx->knobs.mfma;
    opt.mfma_lds_bytes = ctx->knobs.mfma_lds;
    rc = ctx->pats->build_plan(opt, &ctx->plan);
    if (rc) return rc;
    if (ctx->plan.zero_len_panics)
        return tfbs::fail(TFBS_E_ZEROLEN, "length-0 PWM with negative min_score (pattern.rs:150-156)");
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = ctx->stream.create();
    for (Event *t : {&ctx->scan.ev0, &ctx->scan.ev1, &ctx->scan.evk0, &ctx->scan.evk1, &ctx->asmb.asm_t0, &ctx->asmb.asm_t1})
        if (e == hipSuccess) e = t->create();
    for (Event *u : {&ctx->asmb.kf_fork, &ctx->asmb.kf_join, &ctx->scan.over_ev, &ctx->asmb.asm_ev})
        if (e == hipSuccess) e = u->create_untimed();
    if (e == hipSuccess) e = ctx->asmb.side.create();
    int n_cus = 0;
    if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return tfbs::fail(TFBS_E_HIP, std::string("HIP init: ") + hipGetErrorString(e));
    ctx->n_cus = (uint32_t)std::max(1, n_cus);
    const Plan &P = ctx->plan;
    ctx->cfg.lds_bytes = (size_t)P.max_tile_blocks * kBlockBytes;
    if (ctx->cfg.lds_bytes > 160 * 1024) return tfbs::fail(TFBS_E_ARG, "pattern tile exceeds the 160 KiB LDS");
    if (P.max_super_bytes + mfma_lds_fixed() > 160 * 1024)
        return tfbs::fail(TFBS_E_ARG, "MFMA super tile exceeds the 160 KiB LDS");
    if ((rc = fast_kernel_set_lds(ctx->cfg)) ||
        (rc = dinuc_kernel_set_lds((size_t)P.max_di_tile_blocks * kDiBlockBytes)))
        return rc;
    if ((rc = ctx->tabs.fast_units.put(P.fast_units, ctx->stream)) || (rc = ctx->tabs.fast_tiles.put(P.fast_tiles, ctx->stream)) ||
        (rc = ctx->tabs.lut.put(P.lut, ctx->stream)) || (rc = ctx->tabs.wfull.put(P.wfull, ctx->stream)) ||
        (rc = ctx->tabs.gen_pats.put(P.gen_pats, ctx->stream)) || (rc = ctx->tabs.gen_tiles.put(P.gen_tiles, ctx->stream)) ||
        (rc = ctx->tabs.gen_w.put(P.gen_w, ctx->stream)) || (rc = ctx->tabs.m_image.put(P.m_image, ctx->stream)) ||
        (rc = ctx->tabs.m_weights.put(P.m_weights, ctx->stream)) || (rc = ctx->tabs.m_meta.put(P.m_meta, ctx->stream)) ||
        (rc = ctx->tabs.m_supers.put(P.m_supers, ctx->stream)) || (rc = ctx->tabs.slot_mfma.put(P.slot_mfma, ctx->stream)) ||
        (rc = ctx->tabs.di_units.put(P.di_units, ctx->stream)) || (rc = ctx->tabs.di_tiles.put(P.di_tiles, ctx->stream)) ||
        (rc = ctx->tabs.di_lut.put(P.di_lut, ctx->stream)) || (rc = ctx->tabs.di_w.put(P.di_w, ctx->stream)))
        return rc;
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tfbs::fail(TFBS_E_HIP, std::string("upload: ") + hipGetErrorString(e));
    *out = hold.release();
    return TFBS_OK;
}

int tfbs_ctx_set_host_threads(tfbs_ctx *ctx, uint32_t threads) {
    if (!ctx || threads == 0) return tfbs::fail(TFBS_E_ARG, "null ctx or zero threads");
    ctx->enc.host_threads = threads;
    return TFBS_OK;
}

int tfbs_ctx_sync(tfbs_ctx *ctx) {
    if (!ctx) return tfbs::fail(TFBS_E_ARG, "null ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TFBS_OK;
}

float tfbs_ctx_last_scan_ms(const tfbs_ctx *ctx) {
    if (!ctx) return -1.f;
    auto *c = const_cast<tfbs_ctx *>(ctx);
    if (c->scan.timing_pending) {
        if (hipEventSynchronize(c->scan.ev1) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->scan.ev0, c->scan.ev1) == hipSuccess) c->scan.last_ms = ms;
            ms = 0.f;
            if (c->scan.kernel_timed && hipEventElapsedTime(&ms, c->scan.evk0, c->scan.evk1) == hipSuccess) c->scan.last_kernel_ms = ms;
        }
        c->scan.timing_pending = false;
    }
    return c->scan.last_ms;
}

int tfbs_ctx_last_scan_launches(const tfbs_ctx *ctx) { return ctx ? ctx->scan.last_launches : 0; }

int tfbs_ctx_rows_bgzf_seconds(const tfbs_ctx *ctx, double *out) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    out[0] = ctx->rows.rows_s[0];
    out[1] = ctx->rows.rows_s[1];
    return TFBS_OK;
}

int tfbs_ctx_rows_bgzf_blocks(const tfbs_ctx *ctx, uint64_t out[3]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    for (int i = 0; i < 3; i++) out[i] = ctx->rows.bg_blocks[i];
    return TFBS_OK;
}

int tfbs_ctx_scan_counters(tfbs_ctx *ctx, uint64_t out[5]) {
    if (!ctx || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    for (int i = 0; i < 5; i++) out[i] = 0;
    if (!ctx->scan.over.p || !ctx->scan.candn.p || !ctx->scan.hitn.p || !ctx->scan.scan_cand_cap) return TFBS_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nw = std::min(ctx->scan.hitn.n, ctx->scan.candn.n);
    std::vector<uint32_t> hn(nw), cn(nw);
    uint32_t ov[2];
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(hn.data(), ctx->scan.hitn.p, nw * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cn.data(), ctx->scan.candn.p, nw * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ov, ctx->scan.over.p, sizeof ov, hipMemcpyDeviceToHost));
    out[0] = ov[0];
    out[1] = ov[1];
    // (the waves of every slot the last scan launched; a unit's groups share each wave's
    // candidate lists: the LDS list's room once, the global list's once per group)
    const size_t G = std::max<size_t>(1, ctx->scan.last_margs.unit), ns = nw / kMBlockWaves;
    for (size_t s0 = 0; s0 < ns; s0 += G) {
        const size_t ngu = std::min(G, ns - s0);
        const uint64_t cap = (uint64_t)ngu * (ctx->scan.scan_cand_cap / kMBlockWaves), lcap = std::min<uint64_t>(cap, kMWaveCands);
        for (size_t w = 0; w < kMBlockWaves; w++) {
            uint64_t c = 0;
            for (size_t s = s0; s < s0 + ngu; s++) {
                c += cn[s * kMBlockWaves + w];
                out[4] += hn[s * kMBlockWaves + w];
            }
            out[2] += c;
            out[3] += c > lcap ? std::min<uint64_t>(c, lcap + cap) - lcap : 0;
        }
    }
    return TFBS_OK;
}

int tfbs_ctx_window_lists(const tfbs_ctx *ctx, uint64_t entries[2], double *seconds) {
    if (!ctx || !entries || !seconds) return tfbs::fail(TFBS_E_ARG, "null argument");
    entries[0] = ctx->lists.wl_entries[0];
    entries[1] = ctx->lists.wl_entries[1];
    *seconds = ctx->lists.wl_seconds;
    return TFBS_OK;
}
float tfbs_ctx_last_mfma_ms(const tfbs_ctx *ctx) {
    if (!ctx) return -1.f;
    tfbs_ctx_last_scan_ms(ctx);  // resolves the pending events
    return ctx->scan.kernel_timed ? ctx->scan.last_kernel_ms : -1.f;
}


}  // extern "C"
