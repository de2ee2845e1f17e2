// Hit lists (tfbs_batch_hits), best sites (tfbs_batch_best), binding affinities (tfbs_batch_affinity),
// variant effects (tfbs_batch_effects) and mutation scans (tfbs_batch_mutscan): the interfaces of
// scan_hits.hip, scan_best.hip, scan_affinity.hip, scan_effects.hip and scan_mutscan.hip to
// ctx_outputs.hip, what they share on the host (the tables, ScanImage, site_range, text_out) and the
// host-only helpers of hits.cpp, best.cpp, affinity.cpp, effects.cpp and mutscan.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "batch.hpp"
#include "patterns.hpp"
#include "tfbs_internal.hpp"

namespace tfbs {

// One strand of the pattern set in creation order.  w_off: its exact int32 weights in
// HitTables::weights -- [column][A,C,G,T] for a mono PWM, [row][16] for a dinucleotide
// PWM (a multiple of 4 ints: 16-byte rows).  len 0: never matches (TFBS_KIND_OTHER).
struct DevHitStrand {
    uint32_t kind;
    uint32_t len;
    int32_t min_score;
    uint32_t w_off;
};

// Built from Patterns alone (never from the Plan).
struct HitTables {
    std::vector<DevHitStrand> strands;
    std::vector<int32_t> weights;
};
void build_hit_tables(const Patterns &P, HitTables *out);

// One hit as the fill pass writes it: batch haplotype index, pattern index (creation
// order), window, score.
struct DevHitRec {
    uint32_t hap, pattern, window;
    int32_t score;
};

// A ctx's hit-list state (scan_hits.hip): the tables on the device, the scratch and the
// timers; made by the ctx's first hits call.
struct HitsState;
void hits_state_destroy(HitsState *s);
// The resident batch image as the two kernels read it (device pointers); the hit kernel
// reads the first three.
struct ScanImage {
    const DevHap *haps;
    const uint32_t *words;
    const uint32_t *nmask;
    const int32_t *posrel;
    const DevRegion *regions;
    const int32_t *inner;
};
// The public range of the site of strand `pattern` at `window` of haplotype hm of region R
// (the callers' record loops hold both).
inline void site_range(const Batch &B, const Patterns &P, const RegionH &R, const DevHap &hm, uint32_t pattern,
                       uint32_t window, uint64_t *start, uint64_t *end) {
    const int64_t rel = (hm.flags & HAP_HAS_POS) ? B.posrel[hm.pos_off + window] : (int64_t)window;
    *start = R.es + (uint64_t)rel;
    *end = *start + P.pats[pattern].len - 1;
}
// A text handed out through the C API: *text a malloc'd, 0-terminated copy, *len its length.
int text_out(const std::string &s, char **text, size_t *len);
// The hit list of regions [r0, r1) of B (resident as img on `device`): appended to *out
// (sorted as specified), or -- out null -- the count pass alone into per_region[r - r0].
// *state is made on the first call.  Synchronises `stream` (a hipStream_t; this header
// is also the host sources', which include no HIP header).
int hits_run(HitsState **state, int device, void *stream, const Patterns &P, const ScanImage &img,
             const Batch &B, size_t r0, size_t r1, std::vector<tfbs_hit> *out, uint64_t *per_region);
// The last hits_run's times (ms): count pass, scan, fill pass (HIP events, summed over
// the chunks), copy-back + host part (wall).
void hits_last_ms(const HitsState *s, double out[4]);

// Distinct haplotype h (region-local) of region R as load_haplotypes made it: base codes
// 0-4 and positions, unpacked from the batch image.
void region_haplotype(const Batch &B, const RegionH &R, uint32_t h, std::vector<uint8_t> &nucs,
                      std::vector<uint64_t> &pos);
// tfbs_batch_hits_tsv's text appended to out (no header line).
int hits_tsv(const Batch &B, const tfbs_hit *hits, size_t n, const std::string &chrom, int mode, std::string &out);
// The diff modes' baseline of a region (hits.cpp): ids[h] = the ascending haplotype ids of
// distinct haplotype h (empty without membership), *base = the haplotype with the most
// carrier ids, ties to the one holding the lowest id (0 for a region without haplotypes).
int region_baseline(const Batch &B, const RegionH &R, std::vector<std::vector<uint32_t>> &ids, uint32_t *base);
// A `hap` line's carrier_ids column: "*" for the baseline, "." without membership.
std::string carrier_id_text(const Batch &B, const std::vector<std::vector<uint32_t>> &ids, uint32_t h, uint32_t base);

// ---- best sites (tfbs_batch_best): scan_best.hip's interface to ctx_outputs.hip, best.cpp's formatter
// One (haplotype, strand, range) as the kernel writes it: 16 bytes, one vector store.
struct alignas(16) DevBestRec {
    int32_t score;
    uint32_t window, n_windows, zero;
};
struct BestState;
void best_state_destroy(BestState *s);
// The dense best records of regions [r0, r1) of B (resident as img on `device`) appended to
// *out, sorted by (region, haplotype, pattern, range).  *state is made on the first call.
// Synchronises `stream` (a hipStream_t).
int best_run(BestState **state, int device, void *stream, const Patterns &P, const ScanImage &img, const Batch &B,
             size_t r0, size_t r1, std::vector<tfbs_best> *out);
// The last best_run's times (ms): the kernel (HIP events, summed over the chunks), copy-back + host part (wall).
void best_last_ms(const BestState *s, double out[2]);
// tfbs_batch_best_tsv's text appended to out (no header line); the records are whole regions.
int best_tsv(const Batch &B, const tfbs_best *best, size_t n, const std::string &chrom, int mode, std::string &out);

// ---- binding affinity (tfbs_batch_affinity): scan_affinity.hip's interface to ctx_outputs.hip, affinity.cpp's host side
// One (haplotype, strand, range) as the kernel writes it: 16 bytes, one vector store.
struct alignas(16) DevAffRec {
    uint64_t sum;
    uint32_t n_windows, n_nonzero;
};
// a(d) = floor(2^40 * exp(-d / 1000)) from affinity_tables.hpp (tfbs_affinity_weight).
uint64_t affinity_weight(uint64_t d);
// One value per strand in creation order: its pattern_id's top, 0 for a TFBS_KIND_OTHER strand;
// TFBS_E_ARG naming a strand whose sums can wrap int32 (tfbs_patterns_affinity_tops).
int affinity_tops(const Patterns &P, std::vector<int32_t> *tops);
// The most strands one pattern_id has (0 for an empty set).
uint32_t affinity_max_strands(const Patterns &P);
struct AffinityState;
void affinity_state_destroy(AffinityState *s);
// The dense affinity records of regions [r0, r1) of B (resident as img on `device`) appended
// to *out, sorted by (region, haplotype, pattern, range).  *state is made on the first call
// (the two tables and the tops uploaded).  Synchronises `stream` (a hipStream_t).
int affinity_run(AffinityState **state, int device, void *stream, const Patterns &P, const ScanImage &img,
                 const Batch &B, size_t r0, size_t r1, std::vector<tfbs_affinity> *out);
// The last affinity_run's times (ms): the kernel (HIP events, summed over the chunks), copy-back + host part (wall).
void affinity_last_ms(const AffinityState *s, double out[2]);
// tfbs_batch_affinity_tsv's text appended to out (no header line); the records are whole regions.
int affinity_tsv(const Batch &B, const tfbs_affinity *aff, size_t n, const std::string &chrom, int mode,
                 std::string &out);

// ---- variant effects (tfbs_batch_effects): scan_effects.hip's interface to ctx_outputs.hip, effects.cpp's formatter
// One scored record of a chunk as the kernel reads it: R and A packed into one run of the
// chunk's words (and N-mask words, has_n), A from base a_base (a multiple of 32) of the run.
struct DevEffVar {
    uint32_t word_off, nmask_off;  // the run's first word / N-mask word
    uint32_t len_r, len_a;         // bases of R and of A
    uint32_t a, z;                 // common prefix and suffix columns
    uint32_t a_base;               // A's first base in the run
    uint32_t has_n;
};
// One (scored record, strand) as the kernel writes it: 32 bytes, two vector stores.
struct alignas(16) DevEffRec {
    int32_t ref_score;
    uint32_t ref_window, n_ref, zero0;
    int32_t alt_score;
    uint32_t alt_window, n_alt, zero1;
};
struct EffectsState;
void effects_state_destroy(EffectsState *s);
// The dense effect records of regions [r0, r1) of B (built with keep_variants) appended to
// *out, sorted by (region, variant, pattern).  Reads no resident image.  *state is made on
// the first call.  Synchronises `stream` (a hipStream_t).
int effects_run(EffectsState **state, int device, void *stream, const Patterns &P, const Batch &B, size_t r0,
                size_t r1, std::vector<tfbs_effect> *out);
// The last effects_run's times (ms): host prep (wall), the kernel (HIP events, summed over
// the chunks), copy-back + host part (wall).
void effects_last_ms(const EffectsState *s, double out[3]);
// tfbs_batch_effects_tsv's text appended to out (no header line); the records are whole regions.
int effects_tsv(const Batch &B, const tfbs_effect *e, size_t n, const std::string &chrom, int mode, std::string &out);

// ---- mutation scan (tfbs_batch_mutscan): scan_mutscan.hip's interface to ctx_outputs.hip, mutscan.cpp's formatter
// The longest strand the kernel's ring of window scores serves (a ring of 128 scores holds
// the 64 windows of a chunk and the 64 before them: a column's windows reach back L - 1);
// a longer strand takes the slow path.  tfbs_mutscan_ring_max_length() returns it.
constexpr uint32_t kMutRingMax = 65;
// One region of a chunk as the kernel reads it: R packed into the chunk's words (and N-mask
// words, has_n).
struct DevMutRegion {
    uint32_t word_off, nmask_off;  // R's first word / N-mask word
    uint32_t len;                  // columns of R
    uint32_t has_n;
};
// One mutation record as the fill pass writes it: 32 bytes, two vector stores.  The host adds
// the region, the positions and n_windows.
struct alignas(16) DevMutRec {
    uint32_t region;  // of the chunk
    uint32_t pattern, column;
    uint32_t rak;  // ref | alt << 8 | kind << 16
    int32_t ref_score;
    uint32_t ref_window;
    int32_t alt_score;
    uint32_t alt_window;
};
struct MutscanState;
void mutscan_state_destroy(MutscanState *s);
// The mutation records of regions [r0, r1) of B (built with keep_variants) whose kind is in
// `kinds`, appended to *out, sorted by (region, pattern, column, alt base); out null: the count
// pass alone.  *total: the records.  Reads no resident image.  *state is made on the first
// call.  Synchronises `stream` (a hipStream_t).
int mutscan_run(MutscanState **state, int device, void *stream, const Patterns &P, const Batch &B, size_t r0, size_t r1,
                uint32_t kinds, std::vector<tfbs_mutation> *out, uint64_t *total);
// The last mutscan_run's times (ms): host packing (wall), count pass + offset scan, fill pass
// (HIP events, summed over the chunks), copy-back + host expansion (wall).
void mutscan_last_ms(const MutscanState *s, double out[4]);
// tfbs_batch_mutscan_tsv's text appended to out (no header line); any records of the batch.
int mutscan_tsv(const Batch &B, const tfbs_mutation *m, size_t n, const std::string &chrom, std::string &out);

}  // namespace tfbs
