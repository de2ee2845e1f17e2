// The device BGZF row pipeline (tfbs_batch_rows_bgzf): the block batches' slots, their copy
// back and write, and the two host threads of the asynchronous writer.
#include "ctx.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace tfbs;

namespace tfbs {

// n bytes to fd at its offset, which moves past them.  A large write goes out as
// positioned pieces on a few threads (a page-cache copy runs ~2-3 GB/s per thread:
// one thread made the rows' write the run flow's longest host step).  Plain writes in
// order for a descriptor without an offset (a pipe), one that is no regular file, and one
// opened with O_APPEND, where pwrite ignores its offset and the pieces would land in any order.
int write_out(int fd, const char *p, uint64_t n) {
    auto seq = [](int fd, const char *p, uint64_t n, int64_t at) -> int {  // at < 0: write()
        for (uint64_t o = 0; o < n;) {
            const size_t m = (size_t)std::min<uint64_t>(n - o, 1u << 30);
            const ssize_t w = at < 0 ? ::write(fd, p + o, m) : ::pwrite(fd, p + o, m, (off_t)(at + (int64_t)o));
            if (w < 0) {
                if (errno == EINTR) continue;
                return errno ? errno : EIO;
            }
            o += (uint64_t)w;
        }
        return 0;
    };
    constexpr uint64_t kPiece = 32u << 20;
    off_t at = -1;
    if (n >= 2 * kPiece) {
        struct stat st;
        const int fl = fcntl(fd, F_GETFL);
        if (fl >= 0 && !(fl & O_APPEND) && fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) at = lseek(fd, 0, SEEK_CUR);
    }
    int err = 0;
    if (at < 0) {
        err = seq(fd, p, n, -1);
    } else {
        const uint32_t T = (uint32_t)std::min<uint64_t>(4, n / kPiece);
        std::vector<int> errs(T, 0);
        std::vector<std::thread> ts;
        for (uint32_t t = 1; t < T; t++)
            ts.emplace_back([&, t] { errs[t] = seq(fd, p + n * t / T, n * (t + 1) / T - n * t / T, at + (int64_t)(n * t / T)); });
        errs[0] = seq(fd, p, n / T, at);
        for (auto &x : ts) x.join();
        for (int e : errs) err = err ? err : e;
        if (!err && lseek(fd, at + (off_t)n, SEEK_SET) < 0) err = errno;
    }
    return err ? tfbs::fail(TFBS_E_IO, std::string("write: ") + strerror(err)) : TFBS_OK;
}

}  // namespace tfbs

namespace {

// The BGZF batches of one tfbs_batch_rows_bgzf call, across its pieces: batch i uses
// slot i % kBgSlots; a launched batch is written out once two more are queued behind
// it (also across pieces), so the GPU never waits for a copy back or a file write.
int bgzf_drain(tfbs_ctx *ctx, int k, int fd, uint64_t &written);
struct BgPipe {
    uint64_t next = 0;                      // the call's next batch
    int pending[kBgSlots] = {};   // launched batches not yet written (their slots, oldest first)
    int n_pending = 0;
    uint64_t written = 0;
    int drain_oldest(tfbs_ctx *ctx, int fd) {
        const int rc = bgzf_drain(ctx, pending[0], fd, written);
        for (int i = 1; i < n_pending; i++) pending[i - 1] = pending[i];
        n_pending--;
        return rc;
    }
};

// The threads of rows_set_async: the copier takes the drained slots in order, copies
// each back (the main thread waits for its event to be recorded before it launches
// into the slot again) and hands it to the writer, which writes them in order -- a
// slot's copy overlaps the previous slot's write.  TFBS_ROWS_WRITER_DELAY_US: a pause
// before each copy (tests: the caller runs ahead of the copies).
static void rows_copier_loop(tfbs_ctx *ctx) {
    auto &w = ctx->rows.rw;
    for (;;) {
        RowsWriter::Job j;
        {
            std::unique_lock<std::mutex> l(w.mu);
            w.cv.wait(l, [&] { return w.stop || !w.q.empty(); });
            if (w.q.empty()) {  // (stop with nothing queued)
                w.copier_done = true;
                w.cv.notify_all();
                return;
            }
            j = w.q.front();
            w.q.pop_front();
        }
        const double t0 = now_s();
        int rc = TFBS_OK;
        std::string err;
        {
            std::lock_guard<std::mutex> l(w.mu);
            rc = w.rc;  // (after a failure the rest are dropped)
        }
        const int delay_us = env_int("TFBS_ROWS_WRITER_DELAY_US", 0);
        if (delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(delay_us));
        hipError_t he = hipSetDevice(ctx->device);
        if (!rc && (rc = ctx->rows.bg_host[j.k].reserve(std::max<uint64_t>(j.n, 1)))) err = tfbs_last_error();
        if (!rc && he == hipSuccess && j.n)
            he = hipMemcpyAsync(ctx->rows.bg_host[j.k].p, ctx->rows.bg_packed[j.k].p, j.n, hipMemcpyDeviceToHost, ctx->rows.copy_stream);
        if (he == hipSuccess) he = hipEventRecord(ctx->rows.bg_copied[j.k], ctx->rows.copy_stream);
        {
            std::lock_guard<std::mutex> l(w.mu);
            w.recorded[j.k] = true;  // (also on failure: the stream's wait must not block)
        }
        w.cv.notify_all();
        if (he == hipSuccess) he = hipEventSynchronize(ctx->rows.bg_copied[j.k]);
        if (!rc && he != hipSuccess) {
            rc = TFBS_E_HIP;
            err = std::string("rows copy back: ") + hipGetErrorString(he);
        }
        const double t1 = now_s();
        {
            std::lock_guard<std::mutex> l(w.mu);
            w.copy_s += t1 - t0;
            if (rc && !w.rc) {
                w.rc = rc;
                w.err = err;
            }
            w.wq.push_back(j);
        }
        w.cv.notify_all();
    }
}

static void rows_writer_loop(tfbs_ctx *ctx) {
    auto &w = ctx->rows.rw;
    for (;;) {
        RowsWriter::Job j;
        int rc;
        {
            std::unique_lock<std::mutex> l(w.mu);
            w.cv.wait(l, [&] { return !w.wq.empty() || (w.stop && w.copier_done); });
            if (w.wq.empty()) return;
            j = w.wq.front();
            w.wq.pop_front();
            rc = w.rc;
        }
        const double t0 = now_s();
        std::string err;
        if (!rc && (rc = write_out(j.fd, reinterpret_cast<const char *>(ctx->rows.bg_host[j.k].p), j.n))) err = tfbs_last_error();
        const double t1 = now_s();
        {
            std::lock_guard<std::mutex> l(w.mu);
            w.busy[j.k] = false;
            w.write_s += t1 - t0;
            if (rc && !w.rc) {
                w.rc = rc;
                w.err = err;
            }
        }
        w.cv.notify_all();
    }
}

// Waits until slot k's last job is done (k >= 0), until its copy back is enqueued
// (recorded), or until every queued job is done (k < 0); the writer's first failure.
static int rows_wait(tfbs_ctx *ctx, int k, bool recorded = false) {
    auto &w = ctx->rows.rw;
    std::unique_lock<std::mutex> l(w.mu);
    w.cv.wait(l, [&] {
        if (k >= 0) return !w.busy[k] || (recorded && w.recorded[k]);
        for (bool b : w.busy)
            if (b) return false;
        return w.q.empty() && w.wq.empty();
    });
    return w.rc ? tfbs::fail(w.rc, w.err) : TFBS_OK;
}

int bgzf_drain(tfbs_ctx *ctx, int k, int fd, uint64_t &written) {
    const double t0 = now_s();
    HIP_TRY(hipEventSynchronize(ctx->rows.bg_done[k]));
    const double t1 = now_s();
    const uint64_t total = ctx->rows.bg_total_host[3 * k];
    ctx->rows.bg_blocks[0] += ctx->rows.bg_slot_blocks[k];
    ctx->rows.bg_blocks[1] += ctx->rows.bg_total_host[3 * k + 1];
    ctx->rows.bg_blocks[2] += ctx->rows.bg_total_host[3 * k + 2];
    int r;
    if (ctx->rows.rows_async) {  // the writer thread copies it back and writes it (in order)
        if (!ctx->rows.rw.th.joinable()) {
            ctx->rows.rw.th = std::thread(rows_copier_loop, ctx);
            ctx->rows.rw.th2 = std::thread(rows_writer_loop, ctx);
        }
        if ((r = rows_wait(ctx, k))) return r;  // slot k's last job is done (its host buffer free)
        {
            std::lock_guard<std::mutex> l(ctx->rows.rw.mu);
            ctx->rows.rw.busy[k] = true;
            ctx->rows.rw.recorded[k] = false;
            ctx->rows.rw.q.push_back({fd, k, total});
        }
        ctx->rows.rw.cv.notify_all();
        ctx->rows.drain_s[0] += t1 - t0;
        written += total;
        return TFBS_OK;
    }
    if ((r = ctx->rows.bg_host[k].reserve(std::max<uint64_t>(total, 1)))) return r;
    if (total)
        HIP_TRY(hipMemcpyAsync(ctx->rows.bg_host[k].p, ctx->rows.bg_packed[k].p, total, hipMemcpyDeviceToHost, ctx->rows.copy_stream));
    HIP_TRY(hipEventRecord(ctx->rows.bg_copied[k], ctx->rows.copy_stream));
    HIP_TRY(hipEventSynchronize(ctx->rows.bg_copied[k]));
    const double t2 = now_s();
    ctx->rows.drain_s[0] += t1 - t0;
    ctx->rows.drain_s[1] += t2 - t1;
    written += total;
    if ((r = write_out(fd, reinterpret_cast<const char *>(ctx->rows.bg_host[k].p), total))) return r;  // the blocks as they are
    ctx->rows.drain_s[2] += now_s() - t2;
    return TFBS_OK;
}

// The device half of tfbs_batch_rows_bgzf: one row plan's BGZF blocks launched on the
// GPU (older batches written out as newer ones queue: BgPipe).  plan and heads (its
// heads as uploaded) must stay untouched until one of this piece's batches has been
// written out.

// TFBS_BGZF_PROF: the launch's bgzf_wave_kernel phase clocks (debug; synchronises).
static int bgzf_prof_report(tfbs_ctx *ctx, uint32_t nb) {
    std::vector<uint64_t> h((size_t)nb * 32);
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->rows.bg_prof.p, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double ph[5] = {0, 0, 0, 0, 0}, items = 0, st[16] = {}, list_a = 0;
    uint32_t nw = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint64_t *p = &h[(size_t)b * 32];
        if (!p[5]) continue;  // a bgzf_block_kernel block
        nw++;
        for (int k = 0; k < 5; k++) ph[k] += (double)(p[k + 1] - p[k]);
        if (p[7]) list_a += (double)(p[7] - p[1]);
        items += (double)p[6];
        for (int k = 0; k < 16; k++) st[k] += (double)p[8 + k];
    }
    const double d = nw ? nw : 1;
    fprintf(stderr,
            "[bgzf prof] blocks %u wave %u cycles/block: stage %.0f list %.0f items %.0f crc %.0f out %.0f; per block: "
            "items %.1f spins %.1f all-run %.1f look-back %.1f token-lit %.1f byte-lit %.1f heads %.1f newlines %.1f\n",
            nb, nw, ph[0] / d, ph[1] / d, ph[2] / d, ph[3] / d, ph[4] / d, items / d, st[0] / d, st[1] / d, st[2] / d,
            st[3] / d, st[4] / d, st[5] / d, st[6] / d);
    // wave-cycles per block: counting run groups / other groups, the deferred emits, the
    // groups with byte literals; other groups, those on the sample-by-sample look-back
    fprintf(stderr,
            "[bgzf prof] item cycles/block: count run groups %.0f, other groups %.0f; emit %.0f; byte-literal groups "
            "%.0f; other groups %.1f, on the serial look-back %.1f; listing: literal codes and run tests %.0f\n",
            st[8] / d, st[11] / d, st[9] / d, st[12] / d, st[7] / d, st[14] / d, list_a / d);
    return TFBS_OK;
}

int rows_bgzf_device(tfbs_ctx *ctx, const Batch &B, tfbs::RowPlan &plan, std::vector<char> &heads, int fd,
                     BgPipe &pp) {
    int rc;
    struct Done {  // the device part's seconds, on every exit
        tfbs_ctx *c;
        double t;
        ~Done() { c->rows.rows_s[1] += now_s() - t; }
    } done{ctx, now_s()};
    const uint32_t N = B.n_samples, ng = (N + kCumGroup - 1) / kCumGroup;
    const uint64_t n_blocks = (plan.text_bytes + kBgzfRaw - 1) / kBgzfRaw;
    if ((uint64_t)plan.rows.size() * (ng + 1) >= UINT32_MAX) return tfbs::fail(TFBS_E_NOMEM, "too many rows in one call");
    for (size_t i = 0; i < plan.rows.size(); i++) plan.rows[i].cum_off = (uint32_t)(i * (ng + 1));
    if (!n_blocks) {  // nothing launched: the pending batches go out now (their pieces' host data is released)
        while (pp.n_pending)
            if ((rc = pp.drain_oldest(ctx, fd))) return rc;
        return TFBS_OK;
    }
    if (!ctx->rows.bg_crc.n) {  // CRC32 byte table, shift operators and slice tables, once per ctx
        std::vector<uint32_t> t(tfbs::kBgzfCrcWords);
        ctx->rows.bg_crc_full = tfbs::bgzf_crc_tables(t.data(), t.data() + 256, t.data() + 256 + 32 * kBgzfOps,
                                                 t.data() + 256 + 32 * kBgzfOps + 768);
        if ((rc = ctx->rows.bg_crc.put(t, ctx->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // (t goes out of scope)
    }
    heads.assign(plan.heads.begin(), plan.heads.end());
    if ((rc = ctx->rows.bg_rows.put(plan.rows, ctx->stream)) || (rc = ctx->rows.bg_heads.put(heads, ctx->stream)) ||
        (rc = ctx->rows.bg_tok_text.put(plan.tok_text, ctx->stream)) ||
        (rc = ctx->rows.bg_tok_len.put(plan.tok_len, ctx->stream)) ||
        (rc = ctx->rows.bg_tok_lit.ensure(std::max<size_t>(plan.tok_len.size(), 1))) ||
        (rc = ctx->rows.bg_tok_litn.ensure(std::max<size_t>(plan.tok_len.size(), 1))) ||
        (rc = ctx->rows.bg_cum.ensure(std::max<size_t>(plan.rows.size() * (ng + 1), 1))))
        return rc;
    tfbs::BgArgs a{};
    a.rows = ctx->rows.bg_rows.p;
    a.n_rows = (uint32_t)plan.rows.size();
    a.heads = ctx->rows.bg_heads.p;
    a.tok_text = ctx->rows.bg_tok_text.p;
    a.tok_len = ctx->rows.bg_tok_len.p;
    a.tok_lit = ctx->rows.bg_tok_lit.p;
    a.tok_litn = ctx->rows.bg_tok_litn.p;
    a.codes = ctx->enc.enc_packed.p;
    a.cum = ctx->rows.bg_cum.p;
    a.n_samples = N;
    a.text_bytes = plan.text_bytes;
    a.crc_tab = ctx->rows.bg_crc.p;
    a.crc_ops = ctx->rows.bg_crc.p + 256;
    a.crc_slice = ctx->rows.bg_crc.p + 256 + 32 * kBgzfOps;
    a.crc_lane = ctx->rows.bg_crc.p + 256 + 32 * kBgzfOps + 768;
    a.crc_full = ctx->rows.bg_crc_full;
    a.stored = env_int("TFBS_BGZF_STORED", 0) != 0 ? 1u : 0u;
    const bool bg_check = env_int("TFBS_BGZF_CHECK", 0) != 0;  // (debug: checked every launch, synchronously)
    if (bg_check) {
        if ((rc = ctx->rows.bg_check.ensure(1))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->rows.bg_check.p, 0, 4, ctx->stream));
        a.check = ctx->rows.bg_check.p;
    }
    if ((rc = tfbs::launch_tok_lit(a, (uint32_t)plan.tok_len.size(), ctx->stream)) ||
        (rc = tfbs::launch_row_cum(a, ctx->stream)))
        return rc;
    // blocks per launch (512 MiB of block slots); TFBS_BGZF_BATCH_BLOCKS=n: smaller
    // launches, so one call cycles the kBgSlots slots (the tests' path)
    const uint64_t kBatchBlocks = (uint64_t)std::max(1, env_int("TFBS_BGZF_BATCH_BLOCKS", 8192));
    const uint64_t n_batches = (n_blocks + kBatchBlocks - 1) / kBatchBlocks;
    if (!ctx->rows.bg_total_host) HIP_TRY(ctx->rows.bg_total_host.alloc(3 * kBgSlots));
    for (int k = 0; k < kBgSlots; k++) {
        if (!ctx->rows.bg_done[k]) HIP_TRY(ctx->rows.bg_done[k].create_untimed());
        if (!ctx->rows.bg_copied[k]) HIP_TRY(ctx->rows.bg_copied[k].create_untimed());
    }
    if (!ctx->rows.copy_stream) HIP_TRY(ctx->rows.copy_stream.create());
    for (uint64_t i = 0; i < n_batches; i++, pp.next++) {
        const int k = (int)(pp.next % kBgSlots);
        const uint64_t b0 = i * kBatchBlocks;
        const uint32_t nb = (uint32_t)std::min(kBatchBlocks, n_blocks - b0);
        if (ctx->rows.rw.th.joinable()) {
            // async rows: slot k's last copy back -- of this call or of an earlier one, which
            // returned before its copies ran -- must be enqueued by the writer thread before
            // the stream may wait for it (below), and done before the slot's buffers grow
            // (a reallocation under a pending copy sent zeros to the file)
            const bool grows = ctx->rows.bg_out[k].cap < (size_t)nb * kBgzfMax || ctx->rows.bg_packed[k].cap < (size_t)nb * kBgzfMax ||
                               ctx->rows.bg_out_len[k].cap < nb || ctx->rows.bg_off[k].cap < (size_t)nb + 3;
            if ((rc = rows_wait(ctx, k, !grows))) return rc;
        }
        if ((rc = ctx->rows.bg_out[k].ensure((size_t)nb * kBgzfMax)) || (rc = ctx->rows.bg_out_len[k].ensure(nb)) ||
            (rc = ctx->rows.bg_off[k].ensure(nb + 3)) || (rc = ctx->rows.bg_packed[k].ensure((size_t)nb * kBgzfMax)) ||
            (rc = ctx->rows.bg_plans.ensure((size_t)nb * tfbs::bgzf_plan_bytes())))
            return rc;
        // slot k's packed blocks were copied back (kBgSlots batches ago) before they are overwritten
        if (ctx->rows.rw.th.joinable()) {  // (waited for above)
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->rows.bg_copied[k], 0));
        } else if (pp.next >= (uint64_t)kBgSlots) {  // (an earlier call's copies are done)
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->rows.bg_copied[k], 0));
        }
        a.plans = ctx->rows.bg_plans.p;
        a.block0 = b0;
        a.out = ctx->rows.bg_out[k].p;
        a.out_len = ctx->rows.bg_out_len[k].p;
        static const bool prof = env_int("TFBS_BGZF_PROF", 0) != 0;
        if (prof) {
            if ((rc = ctx->rows.bg_prof.ensure((size_t)nb * 32))) return rc;
            HIP_TRY(hipMemsetAsync(ctx->rows.bg_prof.p, 0, (size_t)nb * 256, ctx->stream));
            a.prof = ctx->rows.bg_prof.p;
        }
        if ((rc = tfbs::launch_bgzf_blocks(a, nb, ctx->stream)) || (prof && (rc = bgzf_prof_report(ctx, nb))) ||
            (rc = tfbs::launch_bgzf_compact(ctx->rows.bg_out[k].p, ctx->rows.bg_out_len[k].p, ctx->rows.bg_off[k].p, nb,
                                            ctx->rows.bg_packed[k].p, ctx->rows.bg_plans.p, ctx->stream)))
            return rc;
        if (bg_check) {
            uint32_t bad = 0;
            HIP_TRY(hipMemcpyAsync(&bad, ctx->rows.bg_check.p, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (bad)
                return fail(TFBS_E_STATE, "bgzf_wave_kernel: " + std::to_string(bad) +
                                                 " block-text writes met bits already set (TFBS_BGZF_CHECK)");
        }
        HIP_TRY(hipMemcpyAsync(ctx->rows.bg_total_host.p + 3 * k, ctx->rows.bg_off[k].p + nb, 24, hipMemcpyDeviceToHost, ctx->stream));
        ctx->rows.bg_slot_blocks[k] = nb;
        HIP_TRY(hipEventRecord(ctx->rows.bg_done[k], ctx->stream));
        pp.pending[pp.n_pending++] = k;
        if (pp.n_pending == kBgSlots && (rc = pp.drain_oldest(ctx, fd))) return rc;
    }
    return TFBS_OK;
}

}  // namespace

namespace tfbs {

void rows_bgzf_drain_seconds(const ::tfbs_ctx *ctx, double out[3]) {
    for (int i = 0; i < 3; i++) out[i] = ctx ? ctx->rows.drain_s[i] : 0.0;
    if (ctx) {  // (the writer thread's, read after rows_flush)
        out[1] += ctx->rows.rw.copy_s;
        out[2] += ctx->rows.rw.write_s;
    }
}

void rows_set_async(::tfbs_ctx *ctx, bool on) {
    if (ctx) ctx->rows.rows_async = on;
}

int rows_flush(::tfbs_ctx *ctx) {
    if (!ctx || !ctx->rows.rw.th.joinable()) return TFBS_OK;
    return rows_wait(ctx, -1);
}

// tfbs_batch_rows_bgzf; pos_base (optional): the POS base is asked for once the
// call's rows are counted (every piece's row parts built first).
int rows_bgzf_chained(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome, uint32_t min_maf,
                      uint32_t *fake_position, int fd, uint64_t *bytes, uint64_t *n_rows,
                      const std::function<int(uint64_t, uint32_t *)> &pos_base) {
    if (!ctx || !b || !chromosome || !fake_position || fd < 0) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (ctx->img.resident != b) return tfbs::fail(TFBS_E_STATE, "batch not resident on this ctx");
    Batch &B = b->b;
    r1 = std::min(r1, B.rh.size());
    r0 = std::min(r0, r1);
    if (!B.reduced || B.enc_r0 > r0 || B.enc_r1 < r1)
        return tfbs::fail(TFBS_E_STATE, "regions not encoded on this ctx (tfbs_batch_encode)");
    HIP_TRY(hipSetDevice(ctx->device));
    // the regions in pieces of >= 64 (at most 8): a helper thread formats piece j + 1's
    // rows (the host row plan: heads, POS, token tables) while the GPU makes piece j's
    // blocks; every piece starts a new BGZF block (the decompressed stream is the same).
    // kBgSlots + 1 plan slots: piece j's host data (uploaded by its device half) stays
    // put until one of its batches has been written out -- by then the host has waited
    // for an event after its uploads -- which BgPipe's lag guarantees before the helper
    // builds piece j + kBgSlots + 1 into the same slot.
    const size_t n = r1 - r0;
    const size_t pieces = std::max<size_t>(1, std::min<size_t>(8, n / 64));
    auto cut = [&](size_t j) { return r0 + n * j / pieces; };
    const std::string chrom(chromosome);
    constexpr size_t kPlanSlots = kBgSlots + 1;
    tfbs::RowPlan plans[kPlanSlots];
    std::vector<char> heads[kPlanSlots];
    std::shared_ptr<RowParts> parts;  // pos_base: every piece's rows before the first POS
    if (pos_base) {
        const double t0 = now_s();
        uint64_t nr = 0;
        int rc = build_row_parts(B, r0, r1, min_maf, ctx->enc.host_threads, parts, &nr);
        ctx->rows.rows_s[0] += now_s() - t0;
        if (rc || (rc = pos_base(nr, fake_position))) return rc;
    }
    auto build = [&](size_t j) {
        const double t0 = now_s();
        const int r = parts ? plan_from_parts(B, *parts, cut(j), cut(j + 1), chrom, fake_position, plans[j % kPlanSlots])
                            : tfbs::build_row_plan(B, cut(j), cut(j + 1), chrom, min_maf, fake_position,
                                                   ctx->enc.host_threads, plans[j % kPlanSlots]);
        ctx->rows.rows_s[0] += now_s() - t0;
        return r;
    };
    int rc = build(0);
    if (rc) return rc;
    BgPipe pp;
    ctx->rows.bg_blocks[0] = ctx->rows.bg_blocks[1] = ctx->rows.bg_blocks[2] = 0;
    uint64_t rows = 0, text = 0;
    for (size_t j = 0; j < pieces; j++) {
        int next_rc = TFBS_OK;
        std::thread helper;
        if (j + 1 < pieces) helper = std::thread([&, j] { next_rc = build(j + 1); });
        tfbs::RowPlan &plan = plans[j % kPlanSlots];
        rows += plan.n_rows;
        text += plan.text_bytes;
        rc = rows_bgzf_device(ctx, B, plan, heads[j % kPlanSlots], fd, pp);
        if (helper.joinable()) helper.join();
        if (rc) return rc;
        if (next_rc) return next_rc;
    }
    {
        const double t0 = now_s();
        while (pp.n_pending && !rc) rc = pp.drain_oldest(ctx, fd);
        ctx->rows.rows_s[1] += now_s() - t0;
        if (rc) return rc;
    }
    if (n_rows) *n_rows = rows;
    if (bytes) *bytes = pp.written;
    ctx->rows.rows_text_last = text;
    return TFBS_OK;
}

}  // namespace tfbs

extern "C" {

int tfbs_batch_rows_bgzf(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome,
                         uint32_t min_maf, uint32_t *fake_position, int fd, uint64_t *bytes, uint64_t *n_rows,
                         uint64_t *text_bytes) {
    const int rc = tfbs::rows_bgzf_chained(ctx, b, r0, r1, chromosome, min_maf, fake_position, fd, bytes, n_rows, {});
    if (!rc && text_bytes) *text_bytes = ctx->rows.rows_text_last;
    return rc;
}


}  // extern "C"
