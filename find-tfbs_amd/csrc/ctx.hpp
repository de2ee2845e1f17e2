// The device context (tfbs_ctx) as one struct per stage, and the functions the stages'
// units (ctx*.hip) call across one another.  Plain structs with public members; every
// member frees what it owns in its destructor.  Member order is teardown order, in
// reverse: streams and events are declared before the buffers that are used on them.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "affinity_rows.hpp"
#include "batch.hpp"
#include "bgzf_gpu.hpp"
#include "hip_util.hpp"
#include "hits.hpp"
#include "keys.hpp"
#include "patterns.hpp"
#include "rows.hpp"
#include "scan.hpp"
#include "scores.hpp"
#include "tfbs_internal.hpp"

namespace tfbs {

int env_int(const char *name, int dflt);

// The plan's tables, uploaded once at create.
struct PlanTables {
    DevBuf<DevUnit> fast_units;
    DevBuf<DevPattern> gen_pats;
    DevBuf<DevTile> fast_tiles, gen_tiles;
    DevBuf<int32_t> lut, wfull, gen_w, m_image, m_weights, m_meta;
    DevBuf<DevUnit> di_units;  // dinucleotide path (scan_dinuc.hip)
    DevBuf<DevTile> di_tiles;
    DevBuf<int32_t> di_lut, di_w;
    DevBuf<uint8_t> slot_mfma;  // Plan::slot_mfma
    DevBuf<DevMSuper> m_supers;
    template <class F>
    void each_buf(F &&f) const {
        f(fast_units), f(gen_pats), f(fast_tiles), f(gen_tiles), f(lut), f(wfull), f(gen_w), f(m_image);
        f(m_weights), f(m_meta), f(di_units), f(di_tiles), f(di_lut), f(di_w), f(slot_mfma), f(m_supers);
    }
};

// The environment's knobs, read when the context is made and read-only afterwards.
struct Knobs {
    // table blocks (4 KiB each) per LDS tile: 80 KiB, two workgroups per CU
    uint32_t tile_blocks = (uint32_t)std::min(36, std::max(8, env_int("TFBS_TILE_BLOCKS", 20)));
    uint32_t haps_per_block = (uint32_t)std::max(8, env_int("TFBS_HAPS_PER_BLOCK", 128));
    bool mfma = env_int("TFBS_MFMA", 1) != 0;  // int8 matrix-core path for eligible strands (0: LUT only)
    // LDS image budget of one MFMA super tile
    uint32_t mfma_lds = (uint32_t)std::min(144, std::max(8, env_int("TFBS_MFMA_LDS_KB", 44))) * 1024u;
    // haplotypes per MFMA workgroup (6 bits in a window list entry)
    uint32_t mfma_hpb = (uint32_t)std::min((int)kMMaxHapsPerBlock, std::max(4, env_int("TFBS_MFMA_HAPS_PER_BLOCK", 64)));
    // candidates per haplotype group, per super tile it is scanned against
    uint32_t cand_cap = (uint32_t)std::min(1 << 16, std::max(64, env_int("TFBS_CAND_CAP", 1024)));
    // the scan's unit, groups per workgroup (ScanArgs::unit): 1, 2, 4 forces it, 0 / unset:
    // chosen per batch (scan_unit_for)
    uint32_t scan_unit_env = [](int u) { return u == 1 || u == 2 || u == 4 ? u : 0; }(env_int("TFBS_SCAN_UNIT", 0));
    // 1 lds, 2 global, 0 the host's choice (ScanArgs::unit_words)
    uint32_t scan_unit_words_env = [](const char *uw) {
        return uw && !strcmp(uw, "lds") ? 1u : uw && !strcmp(uw, "global") ? 2u : 0u;
    }(getenv("TFBS_SCAN_UNIT_WORDS"));
    bool debug_over = env_int("TFBS_DEBUG_OVER", 0) != 0;  // print the overflow lists' fill after each check
    bool kf_prof_on = env_int("TFBS_KF_PROF", 0) != 0;
    bool kf_persistent = env_int("TFBS_KF_PERSIST", 1) != 0;          // 0: one workgroup per region
    uint32_t kf_grid = (uint32_t)std::max(0, env_int("TFBS_KF_GRID", 0));  // persistent workgroups per shape at most (0: what fits)
    // regions of more haplotypes take the big shape (0: every region on one shape)
    int kf_big_u = env_int("TFBS_KF_BIGU", (int)key_fast_big_u());
    // 0: every region through key_asm_kernel
    uint32_t key_fast_max_u = (uint32_t)std::max(0, env_int("TFBS_KEY_FAST_MAXU", 1 << 30));
    // 0: every region's corrections in the arena
    uint32_t key_cor_lds = (uint32_t)std::max(0, env_int("TFBS_KEY_COR_LDS", 1 << 30));
    int asm_lean_mode = env_int("TFBS_ASM_LEAN", 1);  // lean assemblies (AsmStages): 0 never, 1 predicted, 2 always (tests)
    // the post-scan stage in the scan's tail (measured: C2 0.083 vs 0.068 ms -- a ticket atomic per scan workgroup)
    bool post_fuse_env = env_int("TFBS_POST_FUSE", 0) != 0;
    // spill records an assembly without the post-scan stage reads in place at most (asm_skips_post;
    // 0: it reads none, the stage is left out only after an assembly without a record).  The fused
    // tail, asked for, keeps the records its own way
    uint32_t spill_inplace =
        post_fuse_env ? 0u : (uint32_t)std::min((int)kSpillInPlaceMax, std::max(0, env_int("TFBS_SPILL_INPLACE", (int)kSpillInPlaceMax)));
    // 0: plain launches
    bool step_graphs = env_int("TFBS_STEP_GRAPH", 1) != 0 && !getenv("TFBS_SCAN_PROF") && !kf_prof_on && !debug_over;
};

// The resident batch's image.
struct BatchImage {
    DevBuf<uint32_t> words, nmask, counts;  // counts: dense, for the LUT/generic slots (and tfbs_batch_download)
    bool counts_live = false;               // counts allocated for the resident batch
    DevBuf<int32_t> posrel, inner;
    DevBuf<DevHap> haps;
    DevBuf<uint32_t> druns;  // HAP_DEDUP haplotypes' diff runs
    DevBuf<DevRegion> regions;
    // key_fast_kernel's static records (AsmArgs::hap_reuse, region_asm), made by build_lists
    DevBuf<uint32_t> hap_reuse;
    DevBuf<uint4> region_asm;
    uint32_t n_regions = 0;
    const tfbs_batch *resident = nullptr;
    uint64_t upload_gen = 0;        // tfbs_batch_upload calls (a new batch image: a new graph)
    uint32_t mfma_group_words = 0;  // packed words of the largest haplotype group (LDS staging)
    template <class F>
    void each_buf(F &&f) const {
        f(words), f(nmask), f(counts), f(posrel), f(inner), f(haps), f(druns), f(regions);
        f(hap_reuse), f(region_asm);
    }
};

// The matrix-core window lists per depth class (ScanArgs::wlist), built at upload.
struct WindowLists {
    DevBuf<uint64_t> wl_off[2], wl_tmp;
    DevBuf<uint32_t> wl[2];
    DevBuf<uint16_t> wl16[2];  // the narrow groups' window lists
    DevBuf<uint8_t> gnarrow;   // per haplotype group of mfma_hpb: every haplotype <= kWlNarrowLen bases
    DevBuf<uint32_t> gorder;   // the scan's group order (most work first; TFBS_SCAN_LPT=0: none)
    DevBuf<uint32_t> gcost;    // (its per-group work estimates)
    bool wl_any_narrow = false, wl_any_wide = false;  // the resident batch has narrow / other groups
    DevBuf<uint4> hd, hd2;                            // the matrix-core scan's compact haplotype descriptors
    uint64_t wl_entries[2] = {0, 0};
    double wl_seconds = 0;   // the last build's wall time
    uint32_t wl_n_haps = 0;  // haplotypes the resident window lists were built for
    uint32_t scan_unit = 1;  // the resident batch's unit (Knobs::scan_unit_env, scan_unit_for)
    // shared windows (ScanArgs::share; TFBS_SHARE=0: none), built with the lists
    bool wl_share = false;  // the resident lists share windows
    DevBuf<uint64_t> sh_off[2], sh_stat;
    DevBuf<uint2> sh[2];
    DevBuf<uint32_t> sh_cur;
    DevBuf<ClassTab> sh_tab;
    uint64_t sh_entries[2] = {0, 0};              // sharer entries per class
    uint64_t sh_listed[2][2] = {{0, 0}, {0, 0}};  // per class: (window, strand) pairs and cells the lists hold
    // (wl_tmp, gcost, sh_cur, sh_stat, sh_tab: the build's own, no step's kernel reads them)
    template <class F>
    void each_buf(F &&f) const {
        f(gnarrow), f(gorder), f(hd), f(hd2);
        for (int c = 0; c < 2; c++) f(wl_off[c]), f(wl[c]), f(wl16[c]), f(sh_off[c]), f(sh[c]);
    }
};

struct ScanState {
    Event ev0, ev1;
    Event evk0, evk1;  // around the dominant kernel (the MFMA launches)
    Event over_ev;
    bool kernel_timed = false;
    float last_kernel_ms = 0.f, last_ms = 0.f;
    int last_launches = 0;
    bool timing_pending = false;
    bool scanned = false;  // the resident batch has been scanned (its lists exist)
    DevBuf<uint32_t> cands;               // matrix-core candidate lists (scan.hpp)
    DevBuf<uint32_t> hitl, hitn;          // matrix-core hit lists (scan.hpp)
    DevBuf<uint32_t> candn;               // per wave: candidates found (tfbs_ctx_scan_counters)
    DevBuf<uint32_t> ref_hits, ref_count;  // reference-window reuse (scan.hpp)
    DevBuf<uint32_t> spill, over;         // spill records, [0] their count, [1] candidates past the wave lists
    uint32_t spill_cap = 1u << 16;
    DevBuf<uint32_t> spill_sorted, spill_bcnt, spill_boff;  // the spill records in region order
    // the counts of spill_sorted's buckets (AsmArgs::spill_cnt) are the assembly's, at
    // asm_ctr + kAsmCtrWords (post_scan_kernel, the wide kernels), else check_overflow's spill_bcnt
    bool spill_cnt_ctr = false;
    DevBuf<uint32_t> cand_over;  // candidates past the waves' list regions (scan.hpp)
    uint32_t cand_over_cap = 1u << 20;
    DevBuf<unsigned long long> hits;  // tfbs_matches' hit bitmaps
    // the last scan's overflow counters, copied back asynchronously (checked,
    // and the scan redone with larger lists, before its results are read)
    PinnedArray<uint32_t> over_host;  // [spill records, candidates past the lists]
    bool over_pending = false;
    bool over_copied = false;  // the last scan's overflow counters copied to over_host
    bool post_done = false;    // the last scan's overflow candidates were rescored (launch_post_scan)
    ScanArgs last_margs{};     // the last matrix-core scan's arguments (launch_post_scan)
    uint32_t scan_cand_cap = 1024;  // the last scan's list entries per workgroup (ScanArgs::cand_cap)
    uint32_t scan_hit_cap = 1024;   // and its hit list entries per workgroup (ScanArgs::hit_cap)
    // fused post-scan (ScanArgs::post_done): tfbs_step allows it for its lean steps
    // (Knobs::post_fuse_env); post_fused: the last scan did it (its assembly skips the launch)
    bool post_fuse_ok = false, post_fused = false;
    DevBuf<unsigned long long> scan_prof;  // TFBS_SCAN_PROF=<file>: scan_mfma_all_kernel's per-wave stamps (prof builds)
    // (scan_prof: profiling runs take no step graph)
    template <class F>
    void each_buf(F &&f) const {
        f(cands), f(hitl), f(hitn), f(candn), f(ref_hits), f(ref_count), f(spill), f(over), f(spill_sorted);
        f(spill_bcnt), f(spill_boff), f(cand_over), f(hits);
    }
};

// What an assembly launched.  A lean one leaves out the wide spill bucketing and the leftover
// key pass when the batch's last assembly needed neither (C2 is launch-bound; Knobs::asm_lean_mode):
// the kernels flag what they could not do and the wait reruns the assembly in full.  It also
// leaves out the post-scan stage itself (the rescoring and the spill
// buckets, launched or in the scan's tail) when the batch's last checked assembly saw neither a
// spill record nor a candidate past the lists: that assembly reads no bucket (asm_args), and
// one that then reports either runs again in full.  post_fused: the stage ran in the scan
// kernel's tail.  A few records do not need the stage either: after a checked assembly with at
// most Knobs::spill_inplace of them (and no candidate) it is left out too, and the assembly's
// kernels read the records where the scan put them, every region's workgroup keeping its own
// (AsmArgs::spill_inplace); inplace is that limit, and a report of more records runs it again in full.
// (After an assembly with no record inplace is 0: no record is read, and one that appears is a rerun.)
struct AsmStages {
    bool wide = true, leftover = true, post = true, post_fused = false;
    uint32_t inplace = 0;  // post left out: the records it reads in place at most (0: none)
};

// Key assembly and reduction (tfbs_batch_assemble, tfbs_batch_reduce).
struct AsmState {
    Stream side;             // the big-region key assembly's stream,
    Event kf_fork, kf_join;  // forked from and joined to the ctx stream
    Event asm_ev, asm_t0, asm_t1;
    DevBuf<uint32_t> asm_scratch;  // key assembly counters of regions with many distinct haplotypes
    DevBuf<uint32_t> key_first, var_counts, asm_redo;  // asm_redo: the regions left to key_asm_kernel
    DevBuf<uint32_t> asm_ctr;                          // the assembly's counters (keys.hpp AsmCtr), the spill buckets after
    DevBuf<uint32_t> cor_arena;                        // key_fast_kernel's corrections past its LDS list
    uint32_t cor_cap = 1u << 22;
    DevBuf<uint8_t> key_flags;
    DevBuf<DevVarKey> var_keys;
    uint32_t var_keys_cap = 1u << 16;
    uint64_t var_cap = 1u << 24;
    bool var_cap_forced = false;          // TFBS_VAR_CAP applied (tfbs_batch_reduce)
    Batch *var_owner = nullptr;           // the batch whose varying counts are only in var_counts (device)
    PinnedArray<uint32_t> asm_host;       // asm_ctr's counter words copied back
    bool asm_ctr_zeroed = false;          // launch_scan zeroed asm_ctr (for the scan's first assembly)
    const Batch *asm_batch = nullptr;     // the batch the enqueued assembly is for
    int asm_state = 0;                    // 0 none, 1 enqueued, 2 complete (checked)
    bool asm_timed = false;
    float last_asm_ms = 0.f;
    DevBuf<uint64_t> kf_prof;         // TFBS_KF_PROF: key_fast_kernel phase clocks and sizes per region
    DevBuf<uint32_t> asm_order;       // the resident batch's regions by distinct haplotypes, most first
    uint32_t asm_order_n = 0;         // regions asm_order holds (0: none)
    uint32_t asm_order_big = 0;       // the first of them with more than key_fast_big_u() haplotypes
    // tfbs_ctx_assembly_trace: the assembly kernels' path word per region (AsmArgs::path)
    bool asm_trace = false;
    bool asm_traced = false;  // the last enqueued assembly wrote asm_path
    DevBuf<uint32_t> asm_path;
    // lean assemblies assembly_wait ran again in full: all, those that needed the wide spill
    // kernels, those that needed the leftover pass
    uint64_t asm_reruns = 0, asm_reruns_wide = 0, asm_reruns_left = 0;
    uint64_t asm_reruns_post = 0;  // those that had left the post-scan stage out and met a record or a candidate
    uint32_t prev_spill = UINT32_MAX, prev_redo = UINT32_MAX;  // the last checked assembly's (unknown: max)
    uint32_t prev_cand = UINT32_MAX;                           // and its scan's candidates past the lists
    AsmStages stages;             // what the enqueued assembly launched
    bool asm_full = false;        // (a rerun: everything)
    bool asm_post_rerun = false;  // the enqueued assembly is the rerun of one that had left the stage out
    // (kf_prof, asm_path: profiling and traced runs take no step graph)
    template <class F>
    void each_buf(F &&f) const {
        f(asm_scratch), f(key_first), f(var_counts), f(asm_redo), f(asm_ctr), f(cor_arena), f(key_flags), f(var_keys);
        f(asm_order);
    }
};

// Per-sample encoding (tfbs_batch_encode).
struct EncState {
    DevBuf<DevVarKey> enc_keys;
    DevBuf<uint8_t> enc_codes, enc_packed;
    DevBuf<uint16_t> enc_pidx;                       // per sample its haplotype pair
    DevBuf<uint32_t> enc_pab, enc_pcnt, enc_pair_n;  // per pair its distinct indices a | b << 16, its samples
    DevBuf<uint16_t> enc_memb;                       // membership rows of host-built regions (u16 per haplotype id)
    DevBuf<uint32_t> enc_nr_ids, enc_nr_meta;        // host-built regions' non-reference ids, per row (offset, reference)
    DevBuf<uint16_t> enc_nr_loc;                     // and their distinct indices (launch_memb_fill)
    DevBuf<uint64_t> enc_rows;                       // per region the device address of its membership row
    PinnedBytes enc_memb_host;  // host-built regions' membership rows staged for upload (reused)
    uint32_t host_threads = 16;  // host threads of tfbs_batch_encode (tfbs_ctx_set_host_threads)
    DevBuf<uint64_t> enc_off;
    DevBuf<EncHdr> enc_hdr;
    DevBuf<uint32_t> enc_vals, enc_hist;                   // kEncMaxVals + 1 per key
    DevBuf<uint32_t> enc_vals_c, enc_hist_c, enc_val_off;  // compacted for the download
};

constexpr int kBgSlots = 3;  // batches of blocks in flight: two queued while one is written out

// rows_set_async (the run flow's one-device path): a drained slot's blocks are
// copied back and written by this ctx's writer threads, in order, while the caller
// goes on; the slot's device buffers are reused once its copy is enqueued (the
// stream waits for bg_copied), its host buffer once its write is done (rows_flush:
// every write done)
struct RowsWriter {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    struct Job { int fd, k; uint64_t n; };
    std::deque<Job> q, wq;  // to copy back; copied, to write (in order)
    std::thread th2;        // the writes (th: the copies back)
    bool copier_done = false;
    bool busy[kBgSlots] = {};      // a job of the slot is queued or running
    bool recorded[kBgSlots] = {};  // its copy back is enqueued (bg_copied[k] recorded)
    bool stop = false;
    int rc = 0;
    std::string err;
    double copy_s = 0, write_s = 0;
};

// Device BGZF rows (tfbs_batch_rows_bgzf).
struct RowsBgzf {
    Stream copy_stream;
    Event bg_done[kBgSlots], bg_copied[kBgSlots];
    DevBuf<DevRow> bg_rows;
    DevBuf<char> bg_heads, bg_tok_text;
    DevBuf<uint8_t> bg_tok_len, bg_plans, bg_tok_litn;
    DevBuf<uint4> bg_tok_lit;
    DevBuf<uint32_t> bg_cum, bg_crc;  // bg_crc: byte table | shift operators
    DevBuf<uint64_t> bg_prof;         // TFBS_BGZF_PROF: bgzf_wave_kernel phase clocks
    uint32_t bg_crc_full = 0;         // bgzf_crc_tables' full-block CRC init term
    DevBuf<uint32_t> bg_check;        // TFBS_BGZF_CHECK=1: the checked BGZF wave kernel's violation count
    // the slots of block batches (one being made, the others copied back and written)
    DevBuf<uint8_t> bg_out[kBgSlots], bg_packed[kBgSlots];
    DevBuf<uint32_t> bg_out_len[kBgSlots];
    DevBuf<uint64_t> bg_off[kBgSlots];
    PinnedBytes bg_host[kBgSlots];          // compressed blocks staged for the host
    PinnedArray<uint64_t> bg_total_host;    // 3 per slot: its packed bytes, wave-kernel blocks, stored blocks
    uint32_t bg_slot_blocks[kBgSlots] = {};  // the blocks of each slot's launch
    uint64_t bg_blocks[3] = {0, 0, 0};  // the last call's blocks: written, wave kernel's, stored (tfbs_ctx_rows_bgzf_blocks)
    double rows_s[2] = {0, 0};          // tfbs_batch_rows_bgzf seconds: row plan (host), the rest
    double drain_s[3] = {0, 0, 0};      // of rows_s[1]: bgzf_drain's waits for the blocks, the copy back, the write
    RowsWriter rw;
    bool rows_async = false;
    uint64_t rows_text_last = 0;  // the last call's uncompressed row bytes
};

// tfbs_step: one step's scan and assembly launches captured as a hipGraph and
// replayed while the resident batch and every buffer they use stay as captured
struct StepGraph : NoCopy {
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
    uint64_t step_sig = 0;       // step_signature() of the graph (or of the last plain step)
    bool step_sig_seen = false;  // the last plain step had step_sig: the next one is captured
    AsmStages step_asm;          // what the graph's assembly launched
    bool capturing = false;      // the timing events and asm_ev are left out of a capture
    void drop() {
        if (step_exec) (void)hipGraphExecDestroy(step_exec);
        if (step_graph) (void)hipGraphDestroy(step_graph);
        step_exec = nullptr;
        step_graph = nullptr;
    }
    ~StepGraph() { drop(); }
};

}  // namespace tfbs

struct tfbs_ctx {
    int device = 0;
    tfbs::Stream stream;  // (first: destroyed after everything that ran on it)
    const tfbs::Patterns *pats = nullptr;
    tfbs::Plan plan;
    tfbs::LaunchConfig cfg;
    uint32_t n_cus = 256;  // the device's compute units
    tfbs::Knobs knobs;
    tfbs::PlanTables tabs;
    tfbs::BatchImage img;
    tfbs::WindowLists lists;
    tfbs::ScanState scan;
    tfbs::AsmState asmb;
    tfbs::EncState enc;
    tfbs::RowsBgzf rows;
    tfbs::StepGraph step;
    // hit lists, best sites, score rows, variant effects, mutation scans, affinities and affinity rows: tables, scratch and
    // timers, each made by its entry point's first call (deleted by tfbs_ctx_destroy)
    tfbs::HitsState *hits_state = nullptr;
    tfbs::BestState *best_state = nullptr;
    tfbs::ScoresState *scores_state = nullptr;
    tfbs::EffectsState *effects_state = nullptr;
    tfbs::MutscanState *mutscan_state = nullptr;
    tfbs::AffinityState *affinity_state = nullptr;
    tfbs::AffinityRowsState *affinity_rows_state = nullptr;  // (its frame is scores_state's, its records' tables affinity_state's)
};

namespace tfbs {

inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// A list capacity after an overflow: a quarter above what was needed.
inline void grow_cap(uint32_t &cap, uint32_t need, uint64_t lim) {
    if (need > cap) cap = (uint32_t)std::min<uint64_t>(lim, (uint64_t)need * 5 / 4 + 1024);
}

// ctx_scan.hip
int build_lists(tfbs_ctx *ctx, uint32_t n_haps, const std::vector<uint8_t> &narrow, Batch *B = nullptr);
int launch_scan(tfbs_ctx *ctx, uint32_t n_haps, unsigned long long *hits, uint32_t hits_wpp);
int check_overflow(tfbs_ctx *ctx, uint32_t n_haps, unsigned long long *hits = nullptr, uint32_t wpp = 0);

// ctx_assembly.hip
AsmArgs asm_args(tfbs_ctx *ctx, const Batch &B, int mode);
int assembly_wait(tfbs_ctx *ctx, Batch &B);

// A lean assembly without the post-scan stage (AsmStages::post): the batch's last
// checked assembly saw no candidate past the lists and no more spill records than are read in
// place (Knobs::spill_inplace; 0: no record) (TFBS_ASM_LEAN=2: always -- the tests' rerun).
inline bool asm_skips_post(const tfbs_ctx *ctx) {
    return ctx->knobs.asm_lean_mode != 0 && !ctx->asmb.asm_full &&
           (ctx->knobs.asm_lean_mode == 2 ||
            (ctx->asmb.prev_spill <= ctx->knobs.spill_inplace && ctx->asmb.prev_cand == 0));
}

// ctx_rows.hip: n bytes to fd at its offset, which moves past them.
int write_out(int fd, const char *p, uint64_t n);

}  // namespace tfbs
