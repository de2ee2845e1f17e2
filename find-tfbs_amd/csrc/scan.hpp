// Launch interface of the scan kernels (scan_kernels.hip, scan_dinuc.hip, scan_mfma.hip) and of the
// window-list builder (window_lists.hip), used by ctx_scan.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tfbs_internal.hpp"

namespace tfbs {

// Everything a scan launch reads or writes (device pointers).
struct ScanArgs {
    const DevTile *tiles;
    uint32_t n_tiles;
    const DevUnit *units;       // fast and dinucleotide paths: units; generic path: unused
    const DevPattern *gpats;    // generic path
    const int32_t *lut;         // fast path: 4 KiB table blocks; dinucleotide path: k-mer blocks
    // fast path: [A,C,G,T] per column; dinucleotide path: 16 pair weights per row
    // (windows containing N)
    const int32_t *wfull;
    const int32_t *gw;          // generic path: 5 weights per column
    const DevHap *haps;
    uint32_t n_haps;
    uint32_t hap_base;          // batch index of haps[0] (a launch over a later part of the batch)
    const DevRegion *regions;
    const int32_t *inner;
    const uint32_t *words;
    const uint32_t *nmask;
    const int32_t *posrel;
    // dense counts [count_off + key * count_stride] of the slots the LUT and generic
    // kernels score (stores); nullptr when every slot is on the matrix cores
    uint32_t *counts;
    uint32_t haps_per_block;
    const DevMSuper *msupers;   // matrix-core path
    uint32_t n_msupers;
    const int32_t *mimage;
    const int32_t *mweights;    // exact weights of the matrix-core strands
    const int32_t *mmeta;       // their per-tile rescoring fields
    uint32_t mimg_max;          // LDS bytes reserved for the largest super tile image
    unsigned long long *hits;   // debug (tfbs_matches): per (hap, pattern, 64-window chunk) hit masks
    uint32_t hits_wpp;
    uint32_t n_patterns_total;
    // matrix-core candidates (scan_mfma.hip): one region of cand_cap (strand |
    // haplotype in the group << 24, window) pairs per haplotype group (region
    // region_base + the group's index in the launch), an equal share per wave, each
    // wave's filled and rescored by the wave (a unit of n groups: the n regions of its
    // groups' slots as one, the haplotype counted from the unit's first)
    uint32_t *cands;  // kCandWords per entry
    uint32_t cand_cap;
    uint32_t region_base;
    // matrix-core hits, sparse (no count matrix, no atomics): the wave that
    // rescores its candidates appends one (haplotype, key = slot * n_inner +
    // range) pair per hit and overlapped inner range to its part of the
    // group's hit list (hitl + 2 (g hit_cap + wave hit_cap / 8), the candidate
    // list's geometry with hit_cap entries per group: cand_cap, or four times that
    // when windows are shared -- a donor's wave lists its sharers' pairs too) and stores
    // their number at hitn[8 g + wave]; the excess goes to the spill list.
    // Invariant: wave list w of haplotype group g of the resident batch is list
    // g * kMBlockWaves + w, in every launch (launch_mfma_all: region_base = the launch's
    // first group); the key assembly (key_kernels.hip) reads a region's lists by that index.
    // The order of the pairs inside a wave list is free: their only reader, the key
    // assembly, takes a region's lists flat and keeps pairs by haplotype (a list holds a
    // pass's own pairs first, then its donors' sharers' in rounds of 64 share entries)
    uint32_t *hitl;
    uint32_t hit_cap;
    uint32_t *hitn;
    uint32_t *candn;  // per wave (as hitn): the candidates it found (tfbs_ctx_scan_counters; no atomics)
    // matrix-core window lists (build_window_lists), per depth class (2, 4): the
    // windows the scan reads, haplotype-major, entry = window << 6 | the haplotype's
    // index in its group of haps_per_block (<= 64); haplotype h's entries start at
    // wlist_off[c][h] (n_haps + 1 offsets, relative to this launch's haps); a
    // narrow group (gnarrow[g], relative to this launch's groups: every haplotype of
    // at most kWlNarrowLen bases, so window << 6 | haplotype fits 16 bits) has its
    // entries at the same offsets of wlist16[c] instead (half the bytes to read)
    const uint32_t *wlist[2];
    const uint16_t *wlist16[2];
    const uint4 *hd;   // matrix-core scan: per haplotype (word_off, len, flags, nmask_off) of haps (build_window_lists)
    const uint4 *hd2;  // and (region, pos_off, drun_off, n_druns): the rescoring's
    const uint8_t *gnarrow;
    // scan_mfma_all_kernel: a workgroup scans one *unit*, `unit` (1, 2 or 4; 0 as 1)
    // consecutive haplotype groups (the last unit may be short) against each staged
    // super tile image; every group keeps its own list slot (region_base + group).
    // Workgroup b scans unit gorder[b] (the units in descending order of work, so the
    // launch ends on the small ones); null: unit b
    const uint32_t *gorder;
    uint32_t unit;
    // a unit's packed words (TFBS_SCAN_UNIT_WORDS): unit_words 0 = the host chooses
    // (global, as measured), 1 = "lds" (as many of the unit's first groups as fit beside
    // the image are copied to the LDS once per workgroup), 2 = "global" (read from
    // `words`); launch_mfma_all
    // sets unit_lds, the groups with LDS words, and unit_lds_words, their room (a unit
    // whose first unit_lds groups span more reads all its words from global memory)
    uint32_t unit_words, unit_lds, unit_lds_words;
    const uint64_t *wlist_off[2];
    // shared windows (build_window_lists, share != 0), per depth class: a window listed
    // for its donor haplotype only stands for the same window of the region's other
    // haplotypes whose bases and diff columns in it are the donor's.  Donor d's
    // sharers are the entries [share_off[c][d], share_off[c][d + 1]) of share[c]: (the
    // sharer's index in this launch's haps, i_lo | i_hi << 16) = "the sharer takes the
    // donor's windows [i_lo, i_hi)"; every hit of the donor is listed for them too
    // (scan_mfma.hip, expansion).  null: nothing is shared
    const uint64_t *share_off[2];
    const uint2 *share[2];
    // reference-window reuse (HAP_DEDUP haplotypes, tfbs_internal.hpp): dedup
    // != 0 scans only their dirty windows (the lists); the HAP_REF haplotypes' hits
    // (strand, window) are listed per region (ref_count[r] of kRefPerRegion at
    // ref_hits + 2 kRefPerRegion r), the excess in the spill list
    uint32_t dedup;
    // HAP_DEDUP haplotypes' diff runs: a hit of one in a window whose strand columns
    // [i, i + L - 1] meet no run is the reference's (the key assembly adds it), so
    // the rescoring does not list it
    const uint32_t *druns;
    uint32_t n_regions;
    uint32_t *ref_hits;
    uint32_t *ref_count;
    // spill list: (region | kind << 31, x, y) records -- kind 0 a hit (haplotype,
    // key), kind 1 a reference hit (strand, window) -- counted at over[0] (of
    // spill_cap), bucketed by region after the scan (launch_spill_buckets)
    uint32_t *spill;
    uint32_t *over;  // [0] spill records, [1] candidates past a wave's list
    uint32_t spill_cap;
    // candidates past a wave's list region: (haplotype, strand, window) triples,
    // rescored by a kernel after the scan (launch_post_scan)
    uint32_t *cand_over;
    uint32_t cand_over_cap;
    // fused post-scan (tfbs_step's lean steps): scan_mfma_all_kernel's last workgroup to
    // finish (ticket post_done) does post_scan_kernel's work -- the overflow candidates'
    // rescoring, the overflow counters to post_report, the spill records bucketed by
    // region (post_need_wide set when they are too many) -- instead of a launch after
    // the scan; post_done null: no fusion; post_bcnt as launch_post_fused's bcnt
    uint32_t *post_done;
    uint32_t post_regions;
    uint32_t *post_bcnt, *post_boff, *post_sorted, *post_report, *post_need_wide;
    // TFBS_SCAN_PROF builds of scan_mfma.hip (tools/variant_build.sh): per wave of
    // the workgroup's first list slot, kScanProfWords clock stamps and counts
    // (tools/scan_prof.py); null otherwise
    unsigned long long *prof;
};
constexpr uint32_t kScanProfWords = 16;
constexpr uint32_t kRefPerRegion = 64;
constexpr uint32_t kMBlockWaves = 8;  // waves per matrix-core workgroup (hit list parts per workgroup)
constexpr uint32_t kCandWords = 2;  // candidate list entry: strand | haplotype in the group (unit) << 24, window
constexpr uint32_t kMMaxUnit = 4;   // groups per unit: kMMaxUnit x kMMaxHapsPerBlock haplotypes fit the entry's 8 bits

struct LaunchConfig {
    int minw = 2;               // __launch_bounds__ min waves per SIMD of the fast kernel
    size_t lds_bytes = 0;       // dynamic LDS of the fast kernel
};

// Enqueues the fast and/or generic scan over n_haps haplotypes on `stream`
// (grids split below 2^31 workgroups).  Returns launches issued or <0.
int launch_fast(const ScanArgs &a, const LaunchConfig &cfg, uint32_t n_haps, hipStream_t stream);
int launch_generic(const ScanArgs &a, uint32_t n_haps, hipStream_t stream);
// Opts the fast kernel into more than 64 KiB of dynamic LDS.
int fast_kernel_set_lds(const LaunchConfig &cfg);
// Dinucleotide scan (scan_dinuc.hip) over the tiles of plan_dinuc.cpp: dense counts
// like the fast kernel's; lds_bytes: the largest tile's blocks (dynamic LDS).
int launch_dinuc(const ScanArgs &a, size_t lds_bytes, uint32_t n_haps, hipStream_t stream);
int dinuc_kernel_set_lds(size_t lds_bytes);
constexpr uint32_t kMWaveCands = 48;  // a scan wave's candidates kept in LDS before its global list
// Matrix-core scan (scan_mfma.hip): sparse hits (hitl / hitn / spill), no counts.
// group_words: the most packed words any haplotype group of haps_per_block spans.
// supers: the host copy of a.msupers (sorted by depth).  One launch on `stream` (one per
// kMLaunchGroups haplotype groups): one workgroup per unit of a.unit haplotype groups
// scans them against every super tile in turn (scan_mfma_all_kernel); a list slot per
// group, whatever the unit.  Returns launches issued or <0.
constexpr uint64_t kMLaunchGroups = ((1ull << 31) - 1) / kMMaxUnit * kMMaxUnit;  // whole units per launch
int launch_mfma_all(const ScanArgs &a, const DevMSuper *supers, uint32_t n_supers, uint32_t group_words, uint32_t n_haps,
                    hipStream_t stream);
// Rescores the candidates past the waves' lists (after launch_mfma_all on the same stream).
int launch_post_scan(const ScanArgs &a, hipStream_t stream);
// The same (when cand) and the spill records' buckets by region in one launch: region
// r's records at [boff[r], boff[r] + bcnt[r]) of sorted, boff[r] written only where
// bcnt[r] != 0 (the buckets' order in sorted is arbitrary); *done and bcnt's
// 2 (n_regions + 1) words (the counts, then the scatter's fill counters) must be zero.
// wide: also the grid-wide spill bucketing (more than kPostSerial records); report /
// need_wide: post_scan_kernel's optional outputs (see there); cand_grid: the rescoring's
// workgroups (1 when the batch's last scan had no candidate past the lists: the same
// result, without 256 workgroups' dispatch and tickets)
constexpr uint32_t kPostSerial = 8192;  // spill records post_scan_kernel's last workgroup buckets itself
int launch_post_fused(const ScanArgs &a, bool cand, uint32_t *done, uint32_t n_regions, uint32_t *bcnt, uint32_t *boff,
                      uint32_t *sorted, hipStream_t stream, bool wide = true, uint32_t *report = nullptr,
                      uint32_t *need_wide = nullptr, uint32_t cand_grid = 256);
uint32_t mfma_group_words(const DevHap *haps, uint32_t n_haps, uint32_t hpb);
constexpr uint32_t kMMaxHapsPerBlock = 64;  // 6 bits of a window list entry
// Builds the window lists of every haplotype of the batch for the depth classes
// c (0: class 2, 1: class 4) with lmin[c] != 0 (the class's shortest strand):
// all windows [0, len - lmin + 1) of a haplotype, only the dirty ones of a
// HAP_DEDUP haplotype when dedup -- a run meeting the window's first span[c]
// columns, span[c] the class's longest strand (tfbs_internal.hpp) --; off[c] gets n_haps + 1
// offsets, list[c] (grown with ensure_list) the entries.  Synchronises `stream`.
constexpr uint32_t kWlNarrowLen = 1024;  // haplotypes of a narrow group: windows < 2^10
struct WindowListBufs {
    uint64_t *off[2];      // n_haps + 1 each
    uint64_t *scan_tmp;    // >= scan_tmp_words(n_haps + 1)
    uint32_t *list[2];
    uint16_t *list16[2];   // the narrow groups' entries (gnarrow: one flag per group of hpb)
    const uint8_t *gnarrow;
    uint4 *hd;             // n_haps compact descriptors (ScanArgs::hd), written here
    uint4 *hd2;            // and ScanArgs::hd2
    uint64_t list_cap[2];  // entries
    // shared windows (share != 0): per class n_haps + 1 offsets by donor, the entries
    // (grown with ensure_share), 2 n_haps words of scratch (per-haplotype statistics,
    // then the fill cursors); stat: 2 u64 per class, the (window, strand) pairs and
    // cells of the windows the lists hold
    uint64_t *soff[2];
    uint32_t *scur;
    uint2 *share[2];
    uint64_t *stat;
};
// Per depth class: the strands a listed window with r columns left in its haplotype
// is scored for (those of length <= r), w[min(r, 32)] of them with c[min(r, 32)]
// cells in all (the scan statistics of lists with shared windows).
struct ClassTab {
    uint32_t w[33], c[33];
};
size_t scan_tmp_words(size_t n);
// In-place exclusive scan of n u64 values on `stream` (the window lists' offsets, the hit
// lists' record offsets); tmp: scan_tmp_words(n) words.
int exclusive_scan(uint64_t *x, uint64_t n, uint64_t *tmp, hipStream_t stream);
// Per haplotype group of hpb (n_groups): the window tiles of its lists, cost[g] =
// pairs of class 2 x w[0] + pairs of class 4 x w[1] (w: the per-pair work of each
// depth class's super tiles), for the scan's workgroup order (a unit's cost: the sum
// of its groups').
int group_costs(const uint64_t *off0, const uint64_t *off1, uint32_t n_haps, uint32_t hpb, uint32_t w0, uint32_t w1,
                uint32_t *cost, hipStream_t stream);
// share != 0: shared windows (ScanArgs::share) -- regions / words: the batch's; a
// HAP_DEDUP haplotype without indels or N lists a dirty window only when no
// lower-indexed haplotype of its region has the same window; shared[c] gets the
// sharer entries of class c (ensure_share grows bufs.share[c]), tab[c] the class's
// strand lengths, listed[c] the (window, strand) pairs and cells its list holds.
int build_window_lists(const DevHap *haps, uint32_t n_haps, const uint32_t *druns, const uint32_t lmin[2],
                       const uint32_t span[2], uint32_t hpb, uint32_t dedup, WindowListBufs &bufs, uint64_t total[2], hipStream_t stream,
                       int (*ensure_list)(void *ctx, int c, uint64_t n, uint32_t **p, uint16_t **p16),
                       void *ensure_ctx, uint32_t share = 0, const DevRegion *regions = nullptr,
                       const uint32_t *words = nullptr, const ClassTab *tab = nullptr,
                       int (*ensure_share)(void *ctx, int c, uint64_t n, uint2 **p) = nullptr,
                       uint64_t shared[2] = nullptr, uint64_t listed[2][2] = nullptr);
// The key assembly's static records of an uploaded batch (key_kernels.hip, key_fast_kernel's
// front reads them instead of the DevHaps): hap_reuse[h], one word per haplotype -- UINT32_MAX
// unless HAP_DEDUP, else (rrun_off - its region's run0) | n_rruns << 16 --, and region_asm[r] =
// (run0: the lowest rrun_off of the region's HAP_DEDUP haplotypes, UINT32_MAX if none; nruns:
// the highest rrun_off + n_rruns minus run0, 0 if none; lmax: the longest of its hap_count
// haplotypes and of its ref_hap; 0).  hap_reuse holds max(n_haps, 1) words.
int launch_region_asm(const DevHap *haps, uint32_t n_haps, const DevRegion *regions, uint32_t n_regions,
                      uint32_t *hap_reuse, uint4 *region_asm, hipStream_t stream);
size_t mfma_lds_fixed();  // LDS bytes the MFMA kernel needs besides the image and words

}  // namespace tfbs
