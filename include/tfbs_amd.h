/*
 * tfbs_amd.h -- C ABI of the MI355X-native PWM scanner that drops in for
 * find-tfbs's per-haplotype TFBS scoring path (Helkafen/find-tfbs v1.0.1).
 *
 * The reference has no FFI on this path: it is the Rust `Pattern` enum
 * (types.rs:86-90) dispatched by `matches` (pattern.rs:141-171), fed by
 * `load_haplotypes` (haplotype.rs:77-88) and consumed by
 * `count_matches_by_sample` / `counts_as_genotypes` (main.rs:439-534).  Each
 * entry point below names the reference function it replaces; INTEGRATION.md
 * shows the Rust `extern "C"` block a maintainer would add to bind them.
 *
 * Conventions
 *  - Every entry returns int: TFBS_OK (0) or a negative TFBS_E_* code;
 *    tfbs_last_error() returns this thread's message for the last failure.
 *    The reference panics where these codes are returned (cited per code).
 *  - Caller owns every buffer it passes for the duration of the call; the
 *    library copies what it keeps.  Opaque objects are freed by their
 *    *_destroy.  No callbacks.
 *  - tfbs_patterns is immutable after creation and may be shared across
 *    threads.  tfbs_ctx and tfbs_batch are single-threaded objects; use one
 *    ctx per host thread / per GPU (the reference runs one reader per worker,
 *    main.rs:333-371).
 *  - Nucleotide codes are the reference enum order A=0 C=1 G=2 T=3 N=4
 *    (types.rs:5-8); weights are milli-log-odds int32 per column [A,C,G,T,N]
 *    with N = 0 (types.rs:103-114).
 *  - Haplotype ids are 2*sample + side, side 0 = Left, 1 = Right
 *    (types.rs:29-30, 66-70).
 */
#ifndef TFBS_AMD_H
#define TFBS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFBS_OK 0
#define TFBS_E_ARG (-1)         /* bad argument / call order */
#define TFBS_E_BADBASE (-2)     /* util.rs:15 "Unknown nucleotide" panic */
#define TFBS_E_REFMISMATCH (-3) /* haplotype.rs:126-128 panic */
#define TFBS_E_MNP (-4)         /* haplotype.rs:141-142 "Missing case" panic */
#define TFBS_E_PLOIDY (-5)      /* haplotype.rs:32 assert */
#define TFBS_E_RANGE (-6)       /* main.rs:407 u64 underflow / FASTA seek failure */
#define TFBS_E_PARSE (-7)       /* pattern.rs parse().unwrap()/expect panics */
#define TFBS_E_IO (-8)          /* file open/read failures (pattern.rs:116, bed.rs:34, ...) */
#define TFBS_E_HIP (-9)         /* HIP runtime error */
#define TFBS_E_NODEVICE (-10)   /* no HIP device: the product never falls back to the CPU */
#define TFBS_E_ALLELES (-11)    /* haplotype.rs:22 alleles[1] on a record with one allele */
#define TFBS_E_ZEROLEN (-12)    /* pattern.rs:150-156 index past the end for a length-0 PWM */
#define TFBS_E_NOPATTERN (-13)  /* main.rs:238 assert!(pwm_list.len() > 0) */
#define TFBS_E_STATE (-14)      /* object used out of order */
#define TFBS_E_NOMEM (-15)

const char *tfbs_strerror(int code);
const char *tfbs_last_error(void);
const char *tfbs_version(void);

/* ------------------------------------------------------------------ */
/* Patterns: the plugin surface (types.rs:86-114; README.md:68-72)      */
/* ------------------------------------------------------------------ */
#define TFBS_KIND_PWM 0   /* Pattern::PWM */
#define TFBS_KIND_OTHER 1 /* Pattern::OtherPattern: length 0, never matches */
/* A dinucleotide PWM (HOCOMOCO's H11DI models; the reference has no counterpart):
 * L >= 2 bases, R = L - 1 rows of 16 milli-log-odds weights indexed 4 a + b for the
 * pair (base a, next base b), A=0 C=1 G=2 T=3 (AA, AC, AG, AT, CA, ..., TT).  The
 * window starting at base i scores sum_{j<R} W[j][4 s[i+j] + s[i+j+1]] (wrapping
 * int32; a pair holding an N adds 0) and matches iff score > min_score, with the
 * match range [pos[i], pos[i] + L - 1].  pattern_length is L (bases).  Limits, each
 * TFBS_E_ARG: L < 2; L > 32; a pattern_id whose strands mix this kind and
 * TFBS_KIND_PWM; the strands of one pattern_id needing more lookup tables than one
 * kernel tile holds (64 KiB; four strands of 32 bases take 16 KiB, so 16 such strands). */
#define TFBS_KIND_DIPWM 2
#define TFBS_DIR_P 0      /* PWMDirection::P ("+") */
#define TFBS_DIR_N 1      /* PWMDirection::N ("-") */

typedef struct tfbs_pattern_desc {
    uint16_t pattern_id;    /* shared by both strands of one PWM (pattern.rs:73-77) */
    uint8_t direction;      /* TFBS_DIR_* */
    uint8_t kind;           /* TFBS_KIND_* */
    uint32_t length;        /* columns (pattern_length, types.rs:92-101); TFBS_KIND_DIPWM: bases L */
    const int32_t *weights; /* length x 5 ints [A,C,G,T,N]; the N column is ignored (always 0);
                               TFBS_KIND_DIPWM: (length - 1) x 16 ints */
    int32_t min_score;      /* a window matches iff score > min_score (pattern.rs:151) */
    const char *name;       /* pattern_id -> name (main.rs:239-250) */
} tfbs_pattern_desc;

typedef struct tfbs_patterns tfbs_patterns;

/* Replaces building Vec<Pattern> by hand: copies n descriptors. */
int tfbs_patterns_create(const tfbs_pattern_desc *descs, size_t n, tfbs_patterns **out);
/* Replaces parse_pwm_files (pattern.rs:37-87): names_csv is --pwm_names,
 * add_reverse = !--forward_only.  Fails with TFBS_E_NOPATTERN when nothing loads. */
int tfbs_patterns_from_files(const char *pwm_file, const char *threshold_dir, float pwm_threshold,
                             const char *names_csv, int add_reverse, tfbs_patterns **out);
/* The same over a mononucleotide file and a dinucleotide file; either may be NULL.
 * The mono file's definitions take pattern ids 0..n-1 exactly as above (a
 * definition named in names_csv takes an id whether or not its threshold loads,
 * pattern.rs:66-81; one not named takes none); the dinucleotide file's continue
 * from n under the same rule.  The dinucleotide file has the mono
 * file's layout: a ">name" line, then one row per transition of 16
 * whitespace-separated floats in the order AA AC AG AT CA CC ... TT (first base
 * major), each read by parse_weight; a row whose field count is not 16 is skipped;
 * a definition of R rows covers R + 1 bases; thresholds come from
 * <threshold_dir>/<name>.thr as for a PWM.  (The column order and the R = L - 1 row
 * count were written from memory of HOCOMOCO's dinucleotide files and of SARUS and
 * have not been checked against a real file: compare with yours before relying on
 * it.)  add_reverse adds the strand W'[i][4a + b] = W[R-1-i][4(3-b) + (3-a)], whose
 * score on s is the forward strand's on the reverse complement of s. */
int tfbs_patterns_from_files_di(const char *pwm_file, const char *dipwm_file, const char *threshold_dir,
                                float pwm_threshold, const char *names_csv, int add_reverse, tfbs_patterns **out);
size_t tfbs_patterns_count(const tfbs_patterns *p);
/* Pointers in *out stay valid while p lives. */
int tfbs_patterns_get(const tfbs_patterns *p, size_t i, tfbs_pattern_desc *out);
/* Name for a pattern_id (main.rs:239-250, last writer wins); NULL if unknown. */
const char *tfbs_patterns_name_of(const tfbs_patterns *p, uint16_t pattern_id);
/* max pattern_length over all patterns (main.rs:404). */
uint32_t tfbs_patterns_max_length(const tfbs_patterns *p);
void tfbs_patterns_destroy(tfbs_patterns *p);
/* Host-only diagnostics of the device plan the scan would use with tiles of
 * tile_blocks 4 KiB table blocks (and, if mfma, the matrix-core path): strands
 * on the 16-bit octet path, the 32-bit quad path, the generic (L > 32) kernel
 * and the FP4 x FP6 MFMA path, and their tiles. */
typedef struct tfbs_plan_stats {
    uint32_t n_octet_strands, n_quad_strands, n_generic_strands;
    uint32_t n_fast_tiles, n_fast_units, n_generic_tiles, max_tile_blocks;
    uint64_t lut_bytes;
    uint32_t n_mfma_strands, n_mfma_tiles, n_mfma_supers;
} tfbs_plan_stats;
int tfbs_patterns_plan_stats(const tfbs_patterns *p, uint32_t tile_blocks, int mfma, tfbs_plan_stats *out);
/* The dinucleotide part of the plan (scored by its own kernel, never by the matrix
 * cores): strands, tiles and the bytes of their lookup tables.  Any output may be NULL. */
int tfbs_patterns_dinuc_stats(const tfbs_patterns *p, uint32_t *n_strands, uint32_t *n_tiles, uint64_t *lut_bytes);
/* Host-only diagnostic of the dinucleotide lookup tables: the scores that the scan
 * kernel's lookup loop gives pattern i (a TFBS_KIND_DIPWM strand) on n_images images,
 * evaluated on the host from the plan's tiles, units and tables -- the arrays a device
 * context uploads -- and never from the pattern's rows.  An image is 32 base codes
 * (0-3 = A,C,G,T): the window's bases followed by whatever comes after them; the score
 * of a strand of L bases does not depend on the codes past L.  The plan is built once
 * per call.  TFBS_E_ARG for a pattern that is not a dinucleotide strand or a code
 * above 3. */
int tfbs_patterns_dinuc_lut_scores(const tfbs_patterns *p, size_t i, const uint8_t *images, size_t n_images,
                                   int32_t *out_scores);
/* Host-only diagnostic of the matrix-core bound (mfma.cpp) for pattern i and
 * one window of pattern_length bases (0-3 = A,C,G,T, 4 = N): the window's
 * bound digit sum q8 = 8 Q, the strand's threshold t8, its scale and column
 * offset c.  The bound is c + scale * q8 / 8 >= apply_pwm (pattern.rs:125-135);
 * the window is a candidate iff q8 > t8, which every window with
 * score > min_score (pattern.rs:151) is.  eligible = 0: the pattern is scored
 * by the LUT kernels instead (the other fields are 0). */
typedef struct tfbs_mfma_bound {
    int32_t eligible;
    int64_t q8, t8, scale, c;
} tfbs_mfma_bound;
int tfbs_patterns_mfma_bound(const tfbs_patterns *p, size_t i, const uint8_t *bases, tfbs_mfma_bound *out);
/* Host-only, read-only diagnostic of the matrix-core plan: copies of the arrays a
 * device context uploads for the matrix-core scan and nothing derived from them.  The
 * plan is built once per call exactly as tfbs_ctx_create builds it with TFBS_MFMA=1
 * and TFBS_MFMA_LDS_KB=lds_kb (0: the default, 44; clamped to 8..144 as there).  image: the FP6 digit fragments of every super tile
 * (lane layout: mfma.cpp, scan_mfma.hip); supers: per super tile its tile count, depth
 * class nk (2 or 4), the byte offset and size of its image, the depth segment ends
 * (byte d - 1: the first tile deeper than d), the common candidate threshold t0, the
 * accumulator's start value acc0 (f32 bits), its shortest and longest strand and the
 * global index of its first tile; meta: per tile 384 ints, strand sn's min_score,
 * weight offset, length and slot at 4 sn .. 4 sn + 3, its pattern index at 256 + sn
 * (-1: a padding strand), the tile's depth class at 320.  *image_bytes, *n_supers and
 * *meta_ints always receive the sizes; each array may be NULL (sizes only) and is
 * TFBS_E_ARG if its capacity (bytes, entries, ints) is too small. */
typedef struct tfbs_mfma_super {
    uint32_t tile_count, nk, img_off, img_bytes, seg;
    int32_t t0;
    uint32_t acc0, lmin, lmax, tile0;
} tfbs_mfma_super;
int tfbs_patterns_mfma_plan(const tfbs_patterns *p, uint32_t lds_kb, uint8_t *image, size_t image_cap,
                            size_t *image_bytes, tfbs_mfma_super *supers, size_t supers_cap, size_t *n_supers,
                            int32_t *meta, size_t meta_cap, size_t *meta_ints);
/* Host-only, read-only diagnostic of the LUT and generic plan: copies of the arrays a
 * device context uploads for scan_fast_kernel and scan_generic_kernel and nothing derived
 * from them.  The plan is built once per call as tfbs_ctx_create builds it with
 * TFBS_TILE_BLOCKS=tile_blocks (not clamped here) and TFBS_MFMA=mfma.  tiles / units: the
 * fast tiles and their units (plan.cpp; a unit's tables are blocks lut_off .. lut_off +
 * nblk - 1 of its tile, a tile's blocks lut_begin .. lut_begin + nblocks - 1 of lut);
 * lut: the table blocks, 1024 ints each (256 codes x 16 bytes: eight int16 halves of an
 * OCTET16 unit, four int32 of a QUAD32 unit); gen_tiles / gen_pats / gen_w: the generic
 * kernel's tiles (first / last index gen_pats), its strands and their weights (five per
 * column from col_off, N last); slot_pid / slot_mfma: per count slot its pattern_id and
 * whether the matrix cores score it.  *sizes always receives the entry counts; buf may
 * be NULL (sizes only), each of its arrays may be NULL, and an array whose capacity (in
 * entries) is too small is TFBS_E_ARG, as is a NULL p or sizes. */
typedef struct tfbs_lut_tile {
    uint32_t first, last, lut_begin, nblocks, slot_begin, nslots, lmin;
} tfbs_lut_tile;
typedef struct tfbs_lut_unit {
    uint32_t lut_off, nblk, nstrand, kind; /* kind 0: OCTET16, 1: QUAD32 */
    uint32_t init[4];
    int32_t thr[8], min_score[8];
    uint32_t len[8], slot_local[8], orig_index[8];
} tfbs_lut_unit;
typedef struct tfbs_lut_gen_pat {
    uint32_t col_off;
    int32_t min_score;
    uint32_t len, slot_local, orig_index;
} tfbs_lut_gen_pat;
typedef struct tfbs_lut_plan_sizes {
    size_t n_tiles, n_units, lut_ints, n_gen_tiles, n_gen_pats, gen_w_ints, n_slots;
} tfbs_lut_plan_sizes;
typedef struct tfbs_lut_plan_buffers {
    tfbs_lut_tile *tiles;
    size_t tiles_cap;
    tfbs_lut_unit *units;
    size_t units_cap;
    int32_t *lut;
    size_t lut_cap;
    tfbs_lut_tile *gen_tiles;
    size_t gen_tiles_cap;
    tfbs_lut_gen_pat *gen_pats;
    size_t gen_pats_cap;
    int32_t *gen_w;
    size_t gen_w_cap;
    uint16_t *slot_pid;
    size_t slot_pid_cap;
    uint8_t *slot_mfma;
    size_t slot_mfma_cap;
} tfbs_lut_plan_buffers;
int tfbs_patterns_lut_plan(const tfbs_patterns *p, uint32_t tile_blocks, int mfma, const tfbs_lut_plan_buffers *buf,
                           tfbs_lut_plan_sizes *sizes);

/* ------------------------------------------------------------------ */
/* Thresholds from a p-value: exact score distributions                  */
/* (the reference has no counterpart; README.md, "Thresholds from a      */
/* p-value")                                                            */
/* ------------------------------------------------------------------ */
/* Take a TFBS_KIND_PWM or TFBS_KIND_DIPWM strand of L bases.  S(x) is its score of the
 * sequence x in {A,C,G,T}^L, summed without wrapping (the count path's score; the mono N
 * column plays no part); cnt(s) = #{x : S(x) = s}; tail(m) = #{x : S(x) >= m}, an exact
 * integer of at most 4^L: 4^L for m <= the lowest attainable score, 0 above the highest.
 * The threshold of a p-value p (a finite double, 0 <= p < 1): x = floor(p * 4^L), exact (p
 * is a dyadic rational: a shift of its 53-bit mantissa inside 128 bits), and
 *     min_score = max{ m : tail(m) > x },
 * always an attained score.  The windows that match (score > min_score) are the largest top
 * set of scores whose p-value is <= p: parse_threshold_file's rule (the last table row with
 * pvalue > threshold, matched strictly above) on an exact table.  p = 0 gives the highest
 * score: nothing matches.
 * Limits, each TFBS_E_ARG with a message naming the strand: L > 63 (4^L must fit 128 bits);
 * sum_j max(|lo_j|, |hi_j|) > INT32_MAX over the columns' (rows') lowest and highest weights
 * (the sums could wrap int32); sum_j (hi_j - lo_j) + 1 > 2^24 bins (mono) or 2^22
 * (dinucleotide: four tables, one per last base); p outside [0, 1) or not finite.
 * device >= 0: the HIP device that computes the tables (score_dist.hip), in chunks of
 * strands whose buffers fit TFBS_PVALUE_SCRATCH_MB (default 256, fractions allowed, read at
 * the call; at least one strand; the result does not depend on it).  device == -1: the
 * same definition on the host's threads (TFBS_HOST_THREADS, at most 16) in 128-bit integers.
 *
 * tfbs_patterns_score_tails: tail(scores[k]) of strand i (creation order) as two 64-bit
 * halves.  The denominator is 4^length: the p-value of "score >= m" as a double is
 * ldexp((double)tail_hi * 18446744073709551616.0 + (double)tail_lo, -2 * (int)length)
 * (rounded; the integers are exact).  TFBS_E_ARG for a TFBS_KIND_OTHER strand. */
int tfbs_patterns_score_tails(const tfbs_patterns *p, int device, size_t i, const int32_t *scores, size_t n,
                              uint64_t *tail_lo, uint64_t *tail_hi);
/* One min_score per strand in creation order (tfbs_patterns_count entries); a
 * TFBS_KIND_OTHER strand gets its own min_score back. */
int tfbs_patterns_pvalue_thresholds(const tfbs_patterns *p, int device, double pvalue, int32_t *min_scores);
/* A copy of p whose strand k has min_score min_scores[k]; ids, names, order and weights
 * are p's. */
int tfbs_patterns_with_min_scores(const tfbs_patterns *p, const int32_t *min_scores, tfbs_patterns **out);
/* tfbs_patterns_from_files_di's ids and names without a threshold directory: every
 * definition named in names_csv loads and its strands take tfbs_patterns_pvalue_thresholds'
 * min_score (on `device`, -1: the host).  A definition the limits refuse fails the call
 * with a message naming it.  TFBS_E_NOPATTERN when nothing is named. */
int tfbs_patterns_from_files_pvalue(const char *pwm_file, const char *dipwm_file, const char *names_csv,
                                    int add_reverse, int device, double pvalue, tfbs_patterns **out);
/* The bins one workgroup takes in a gather step (out[0]) and in the suffix sum (out[1]) of
 * score_dist.hip: the spans at which the device path crosses a tile (for its tests). */
void tfbs_pvalue_tile_widths(uint32_t out[2]);

/* pattern.rs:13-16 parse_weight: (f32(s) * 1000f32).round() as i32. */
int tfbs_parse_weight(const char *s, int32_t *out);
/* pattern.rs:18-35 parse_threshold_file: returns 1 (found, *out set), 0 (None) or an error. */
int tfbs_parse_threshold_file(const char *path, float pwm_threshold, int32_t *out);

/* ------------------------------------------------------------------ */
/* Device context: one GPU, one HIP stream, the pattern tables in HBM   */
/* ------------------------------------------------------------------ */
typedef struct tfbs_ctx tfbs_ctx;

int tfbs_device_count(int *n);
/* Uploads the 4-mer lookup tables of p to `device`.  p must outlive ctx. */
int tfbs_ctx_create(int device, const tfbs_patterns *p, tfbs_ctx **out);
void tfbs_ctx_destroy(tfbs_ctx *ctx);
int tfbs_ctx_sync(tfbs_ctx *ctx);
/* Host threads the ctx's host-side work may use (tfbs_batch_encode's staging;
 * default min(16, hardware threads)): a run with one ctx per device passes its share. */
int tfbs_ctx_set_host_threads(tfbs_ctx *ctx, uint32_t threads);
/* Device time (HIP events on the ctx stream) of the last tfbs_scan, ms. */
float tfbs_ctx_last_scan_ms(const tfbs_ctx *ctx);
/* Number of scan-kernel launches issued by the last tfbs_scan. */
int tfbs_ctx_last_scan_launches(const tfbs_ctx *ctx);
/* Device time (ms) of the last tfbs_scan's matrix-core kernel launches alone
 * (HIP events on the ctx stream), or -1 if the scan ran no MFMA tile. */
float tfbs_ctx_last_mfma_ms(const tfbs_ctx *ctx);
/* The matrix-core window lists of the uploaded batch (built by tfbs_batch_upload):
 * entries[c] = windows depth class c (0: strands of 1-2 K chunks, 1: 3-4) reads,
 * *seconds = the build's wall time.  Zeros before an upload or without MFMA strands. */
int tfbs_ctx_window_lists(const tfbs_ctx *ctx, uint64_t entries[2], double *seconds);
/* The last matrix-core scan's list counters (waits for it): out[0] spill records,
 * out[1] candidates past the waves' lists (rescored by post_scan_kernel), out[2]
 * candidates found, out[3] of them written to the waves' global lists (past the
 * LDS ones), out[4] (haplotype, key) pairs in the hit lists.  Zeros without one. */
int tfbs_ctx_scan_counters(tfbs_ctx *ctx, uint64_t out[5]);

/* Replaces matches() (pattern.rs:141-171) for ONE haplotype against every
 * pattern, on the GPU.  nucs are codes 0..4, pos the NucleotidePos.pos values.
 * Writes match ranges grouped by pattern index (in creation order): for each
 * pattern i, counts[i] matches; the ranges are concatenated into out_start /
 * out_end (start = pos[w], end = pos[w] + L - 1) in window order.  *n_total
 * receives the total; TFBS_E_ARG if cap is too small (then *n_total is the need). */
int tfbs_matches(tfbs_ctx *ctx, const uint8_t *nucs, const uint64_t *pos, size_t n, uint32_t *counts,
                 uint64_t *out_start, uint64_t *out_end, size_t cap, size_t *n_total);

/* ------------------------------------------------------------------ */
/* Haplotype reconstruction (haplotype.rs:94-156)                       */
/* ------------------------------------------------------------------ */
/* patch_haplotype over a reference window.  Diffs are flattened: diff d has
 * ref codes dref[roff..roff+dnref[d]) and alt codes dalt[aoff..aoff+dnalt[d]).
 * Writes at most cap bases; *n_out gets the length (TFBS_E_ARG if > cap). */
int tfbs_patch_haplotype(uint64_t range_start, uint64_t range_end, size_t n_diffs, const uint64_t *dpos,
                         const uint8_t *dref, const uint32_t *dnref, const uint8_t *dalt, const uint32_t *dnalt,
                         const uint8_t *ref_nucs, const uint64_t *ref_pos, size_t n_ref, uint8_t *out_nucs,
                         uint64_t *out_pos, size_t cap, size_t *n_out);

/* ------------------------------------------------------------------ */
/* Region batches: load_haplotypes + find_all_matches + counting          */
/* (haplotype.rs:13-88, main.rs:94-154, 395-436, 439-534)                */
/* ------------------------------------------------------------------ */
typedef struct tfbs_batch tfbs_batch;

/* n_samples = selected samples (main.rs:293-314).  keep_membership = 0 drops
 * per-haplotype group membership (scan-only use; rows then unavailable). */
int tfbs_batch_create(const tfbs_patterns *p, uint32_t n_samples, int keep_membership, tfbs_batch **out);
void tfbs_batch_destroy(tfbs_batch *b);
/* Registers a BED source by basename (bed.rs:49-60); returns its index >= 0. */
int tfbs_batch_add_bed(tfbs_batch *b, const char *basename);
/* main.rs:404: L_max of the halo-extended windows, if wider than the pattern set's
 * longest strand (>= it; before the first region).  A batch scanning a shard of the
 * pattern_ids passes the whole set's L_max so that its windows, distinct haplotypes
 * and counts are those of the unsharded run (SURVEY.md 8(e) region x PWM shard). */
int tfbs_batch_set_window_lmax(tfbs_batch *b, uint32_t lmax);
/* load_diffs / group_by_diffs / load_haplotypes (haplotype.rs:16-88) on a device
 * (before the first region; device < 0: host only): a region whose applied
 * records are all SNVs inside its window (REF = the window's base, ALT another of
 * A/C/G/T, at most 64, one per position, carrier ids ascending) and whose window
 * has no N gets its haplotypes' diff masks, distinct groups, patched and packed
 * haplotypes and membership computed there (the membership stays on the device, a
 * u16 distinct index per haplotype id, fetched only when a host path needs it).  A
 * region with indels or N whose applied records are at most 64 distinct diffs with
 * ascending carriers is grouped there (distinct masks, carrier counts, membership:
 * the O(haplotypes x records) part) and the host patches only its distinct groups
 * (TFBS_DEV_PATCH=0: built on the host).  Every other region, and one of more than
 * 2 047 distinct diff masks, is built on the host.  The batch is the same either
 * way (tfbs_batch_region_input_digest).
 *
 * device == TFBS_GROUPER_HOST: the same grouping in plain C++ on the host (the device
 * path of the build -- qualification, chunks, the finish of every group, membership
 * rows fetched where a device would read them in place -- without a device; for tests
 * and for comparing the two).  TFBS_GROUP_REGIONS (1..1024, read at every build) caps
 * the regions grouped by one launch; unset: 1024, or what 1 GiB of masks holds. */
#define TFBS_GROUPER_HOST (-2)
int tfbs_batch_set_build_device(tfbs_batch *b, int device);
/* on != 0: regions ended from now on are queued, not built; until the release they are
 * not part of the batch (tfbs_batch_num_regions and every reader see the batch without
 * them).  on == 0 releases: the queued regions are built by one call on the host's
 * threads (TFBS_HOST_THREADS, at most 16) and appended in the order they were ended --
 * with a build device one grouper launch per chunk of regions instead of one per
 * region.  A region that fails to build fails the release with its error; then none
 * of the queued regions is added and all are dropped.  tfbs_batch_destroy drops queued
 * regions unbuilt.  TFBS_E_STATE while a region is open. */
int tfbs_batch_hold(tfbs_batch *b, int on);
/* Regions grouped on the device / built on the host so far. */
int tfbs_batch_build_stats(const tfbs_batch *b, uint64_t *dev_regions, uint64_t *host_regions);
/* Chunks of regions handed to the grouper so far, one launch each. */
int tfbs_batch_group_calls(const tfbs_batch *b, uint64_t *calls);
/* Of the regions grouped on the device, those whose distinct groups the host
 * patched (indels / N). */
int tfbs_batch_patch_stats(const tfbs_batch *b, uint64_t *patched_regions);

/* The grouper of tfbs_batch_set_build_device driven alone: raw carrier lists in, what
 * the grouper produced out.  device >= 0: the HIP grouper of that device;
 * TFBS_GROUPER_HOST: the host grouper.  Calls on one handle reuse its scratch and its
 * membership rows, as the batches of a run do.
 *
 * One call is one launch over n_regions regions of H haplotype ids.  Region j has
 * n_records[j] records (a record's rank is its index in its region); n_carriers holds
 * every record's carrier count, regions back to back, and ids every record's carrier
 * ids, back to back in the same order.  Per region: n_groups[j] = its distinct
 * non-empty masks (UINT32_MAX: more than 2 047, the region a batch builds on the
 * host); its masks and their carrier counts in the grouper's order, regions back to
 * back in masks / counts (cap entries each; *n_masks = the entries, TFBS_E_ARG when
 * cap is short); rows + j * H = its membership row as the grouper's fetch hands it
 * out (a mask's index per id, n_groups[j] for an id without one; 0xFFFF throughout for
 * an overflowing region, whose row the grouper leaves unwritten).
 *
 * Refused with TFBS_E_ARG before anything is launched: H == 0, more than 64 records in
 * a region, a record without a carrier, an id >= H, ids not strictly ascending, more
 * than 1 024 regions or n_regions * H > 2^27 (a batch's chunk rule). */
typedef struct tfbs_grouper tfbs_grouper;
int tfbs_grouper_create(int device, tfbs_grouper **out);
void tfbs_grouper_destroy(tfbs_grouper *g);
int tfbs_grouper_group(tfbs_grouper *g, uint32_t H, size_t n_regions, const uint32_t *n_records,
                       const uint32_t *n_carriers, const uint32_t *ids, uint32_t *n_groups, uint64_t *masks,
                       uint32_t *counts, size_t cap, size_t *n_masks, uint16_t *rows);
/* main.rs:404-407: the halo-extended window of a merged region. */
int tfbs_batch_region_ext(const tfbs_batch *b, uint64_t merged_start, uint64_t merged_end, uint64_t *ext_start,
                          uint64_t *ext_end);
/* Starts a merged region; ref_ascii = FASTA bases from ext_start (main.rs:156-161,
 * may be shorter than the window at a contig end). */
int tfbs_batch_region_begin(tfbs_batch *b, uint64_t merged_start, uint64_t merged_end, const char *ref_ascii,
                            size_t n_ref);
/* One inner peak selected by select_inner_peaks (main.rs:62-72); duplicates count twice. */
int tfbs_batch_region_add_inner(tfbs_batch *b, uint32_t bed, uint64_t start, uint64_t end);
/* One BCF record (haplotype.rs:16-60): gt = 2 raw BCF GT ints per selected
 * sample, INT32_MIN+1 = vector_end.  Left carries ALT iff gt0 == 4 (Unphased(1)),
 * Right iff gt1 == 5 (Phased(1)). */
int tfbs_batch_region_add_record_gt(tfbs_batch *b, uint64_t pos, uint32_t n_alleles, const char *ref,
                                    const char *alt, const int32_t *gt);
/* Same with the carrying haplotype ids given directly (phased synthetic data). */
int tfbs_batch_region_add_record_carriers(tfbs_batch *b, uint64_t pos, const char *ref, const char *alt,
                                          const uint32_t *hap_ids, size_t n);
/* Groups, patches, deduplicates and packs the region's distinct haplotypes. */
int tfbs_batch_region_end(tfbs_batch *b);

size_t tfbs_batch_num_regions(const tfbs_batch *b);
size_t tfbs_batch_num_haplotypes(const tfbs_batch *b); /* distinct haplotypes (number_of_haplotypes, main.rs:97-130) */
/* Windows the scan scores: sum over distinct haplotypes and PWM patterns of max(0, len - L + 1). */
uint64_t tfbs_batch_num_windows(const tfbs_batch *b);
/* Column lookups the scan performs: sum over windows of the pattern length L. */
uint64_t tfbs_batch_num_cell_ops(const tfbs_batch *b);
/* Per-sample-weighted windows (each distinct haplotype times its carrier count). */
uint64_t tfbs_batch_num_effective_windows(const tfbs_batch *b);
/* Windows and column lookups the scan executes: a window of an SNV-only haplotype
   whose bases and positions equal the region's reference window takes the
   reference window's result (reference-window reuse, TFBS_DEDUP=0 disables it);
   helper reference haplotypes of regions without a reference group count here.
   After tfbs_batch_upload they count what the uploaded window lists hold: a window
   that several SNV-only haplotypes of a region have in common once (shared windows,
   TFBS_SHARE=0 at the upload disables them). */
uint64_t tfbs_batch_num_scan_windows(const tfbs_batch *b);
uint64_t tfbs_batch_num_scan_cell_ops(const tfbs_batch *b);
/* Packed bytes the scan reads from HBM per launch (sequence + masks + positions + metadata). */
uint64_t tfbs_batch_input_bytes(const tfbs_batch *b);
/* Bytes of the dense u32 counts (the LUT / generic kernels' slots, and the debug
   download tfbs_batch_download fills); the matrix-core path writes sparse hit lists. */
uint64_t tfbs_batch_output_bytes(const tfbs_batch *b);

/* Copies the packed batch into ctx device memory (H2D). */
int tfbs_batch_upload(tfbs_ctx *ctx, tfbs_batch *b);
/* Scans the uploaded batch on the GPU (the work of matches() over every distinct
 * haplotype, main.rs:101-147, plus the overlap test of main.rs:503): sparse hit
 * lists -- one (distinct haplotype, pattern_id slot x inner range) entry per hit
 * and overlapped range from the matrix-core kernel, the region's reference
 * haplotype's hits listed for reference-window reuse -- and, for strands the
 * LUT / generic kernels score, dense counts.  Asynchronous on the ctx stream;
 * tfbs_batch_assemble / tfbs_batch_reduce / tfbs_batch_download turn the lists
 * into per-key counts. */
int tfbs_scan(tfbs_ctx *ctx, tfbs_batch *b);
/* D2H copy of the counts into the batch. */
int tfbs_batch_download(tfbs_ctx *ctx, tfbs_batch *b);
/* Alternative to tfbs_batch_download for row emission (the gather half of
 * count_matches_by_sample, main.rs:500-534, moved to the device): classifies
 * every (region, pattern_id, inner range) key on the GPU (some distinct
 * haplotype matched / distinct haplotypes disagree) and downloads only the
 * flags and one count per key; the per-haplotype counts of the disagreeing keys
 * stay on the device (tfbs_batch_encode / tfbs_batch_rows_bgzf read them there)
 * and are downloaded when a host key / row function first needs them -- the ctx
 * makes that copy itself before it reduces another batch or is destroyed.  The
 * key / row functions below then work as after a download. */
int tfbs_batch_reduce(tfbs_ctx *ctx, tfbs_batch *b);
/* The device half of tfbs_batch_reduce, enqueued behind tfbs_scan with no host
 * wait (main.rs:94-154's per-region result + count_matches_by_sample's key
 * vectors, main.rs:500-534): candidates past the scan's lists rescored, spill
 * records bucketed, every region's keys assembled from its hit lists -- each
 * HAP_DEDUP haplotype's count is the reference haplotype's plus its own hits
 * minus the reference hits inside its dirty windows -- classified, and the
 * varying keys' counts compacted on the device.  tfbs_batch_assemble_wait
 * waits for it and checks every list (a scan list that overflowed is rescanned
 * larger, a full varying-key list reassembled); tfbs_batch_reduce then only
 * downloads.  One step of scan + assembly = tfbs_scan, tfbs_batch_assemble,
 * tfbs_batch_assemble_wait. */
int tfbs_batch_assemble(tfbs_ctx *ctx, tfbs_batch *b);
int tfbs_batch_assemble_wait(tfbs_ctx *ctx, tfbs_batch *b);
/* One step of the resident batch: tfbs_scan + tfbs_batch_assemble +
 * tfbs_batch_assemble_wait, same results.  From the third step alike on (same
 * batch, no buffer regrown), the scan's and the assembly's launches run as one
 * hipGraph captured on the third (TFBS_STEP_GRAPH=0: never); graph steps leave
 * the timing queries (tfbs_ctx_last_scan_ms, ...) at the last plain step's. */
int tfbs_step(tfbs_ctx *ctx, tfbs_batch *b);
/* Device time (ms, HIP events on the ctx stream) of the last assembly, -1 if none ran. */
float tfbs_ctx_last_assemble_ms(const tfbs_ctx *ctx);
/* The assembly's path report (read-only; the tests' proof that a case took the branch it
 * was built for).  tfbs_ctx_assembly_trace(ctx, 1): every assembly enqueued from now on
 * writes one word per region -- thread 0 of the workgroup that takes the region, one plain
 * store -- and tfbs_step runs its launches plainly (no graph).  Off (the default) the
 * kernels get a null pointer and the step is unchanged.
 * tfbs_batch_assembly_paths: the words of the last checked assembly of b (after
 * tfbs_batch_reduce / tfbs_batch_assemble_wait / tfbs_step), n = the batch's regions, in
 * region order; zeros for a region no kernel took; an error if that assembly was enqueued
 * before the trace was turned on.  A rerun overwrites a region's word; a
 * region key_fast_kernel gave up keeps its word (the bits decided before the give-up and
 * the reason) and gains key_asm_kernel's TFBS_PATH_ASM* bits.
 *   key_fast_kernel (branches listed in key_kernels.hip; a bit below the point of a give-up
 *   is left clear):
 *   FAST          key_fast_kernel took the region
 *   BIG           the 1 024-thread shape (regions of more than TFBS_KF_BIGU haplotypes), else the small one
 *   WALK          dirty reference hits by the sorted walk (U x nref > 65 536), else pairwise
 *   STEPBITS      wave 0 kept a bit per pairwise step and reserved its slots once
 *   DIRTY_LISTED  the dirty corrections were listed in the first pass (pairwise, nD <= the shape's list)
 *   COR_ARENA     the corrections went to the launch arena, else LDS
 *   LISTS_SLICED  the hit lists were taken a slice at a time (more lists than the shape stages)
 *   RUNS_L2       the diff runs were read from global memory, else LDS
 *   HAP_GLOBAL    more haplotypes than descriptors in LDS: the others were read again
 *   U32           u32 counters, else packed u16
 *   CNT_ARENA     counter chunks in the arena (more than 32 LDS chunks), else LDS
 *   TICKET        a persistent workgroup took the region with a ticket (not its first)
 *   GIVEUP        key_fast_kernel left the region to key_asm_kernel; TFBS_PATH_WHY(word) is the
 *                 reason: 0 shape (haplotypes, keys, inner ranges), 2 diff runs (no input, see
 *                 below), 3 reference hits, 4 arena full (corrections), 5 arena full (counters)
 *   key_asm_kernel (the reduction's list pass):
 *   ASM           key_asm_kernel took the region
 *   ASM_HAPS      more haplotypes than its LDS descriptors (1 024)
 *   ASM_RUNS      more diff runs than it stages (2 048)
 *   ASM_HITS      more own hits than it stages (2 048): re-read per pass
 *   ASM_REFS      more reference hits than it stages (256): re-read
 *   ASM_SCRATCH   counters in the batch's scratch (more than 6 144 haplotypes)
 * The limits behind the bits, small | big shape (U distinct haplotypes, nref reference hits,
 * nD dirty (haplotype, reference hit, range < 32) triples, T touched keys): 256 | 1 024
 * threads; descriptors of 512 | 2 048 haplotypes in LDS; 1 536 | 12 288 staged runs (the span
 * of the region's run lists); 128 | 256 hit lists staged at once (8 per haplotype group and
 * super tile); pairwise while U x nref <= 65 536; a wave's lanes are 64 / rpl haplotypes x rpl
 * hits (rpl: nref rounded up to a power of two, 64 at most), its steps ceil(U / (waves x 64 /
 * rpl)) x ceil(nref / rpl): step bits up to 64 steps; dirty corrections listed in the first pass
 * while pairwise and nD <= 3 584 | 8 192; corrections in LDS while listed own hits + the
 * region's spill records (the reference hits past its list of 64 among them) + nD <= min(3 584 |
 * 8 192, TFBS_KEY_COR_LDS), else a share of the arena of TFBS_KEY_COR_CAP words (full: give-up
 * 4); packed u16 counters while 4 x (longest haplotype + 64) < 65 536 and TFBS_KEY_COR_LDS != 0;
 * rows per chunk min(3 072 | 24 576 x (2 if packed) / U, 256 | 1 024); more than 32 chunks, or
 * TFBS_KEY_COR_LDS = 0: u32 counters of min(T, 256 | 1 024) rows in the arena (full: give-up
 * 5).  Give-up 0: U > min(2 048, TFBS_KEY_FAST_MAXU), more than 16 384 keys or 32 inner ranges;
 * 3: nref > 256.  Give-up 2 (65 536 or more staged runs) has no input: at most 2 048 haplotypes
 * of at most 16 runs in their own and 16 in the reference's columns, and the span starts at the
 * first haplotype's reference-column list, behind its own: at most 2 048 x 32 - 16 = 65 520. */
enum {
    TFBS_PATH_FAST = 1u << 0,
    TFBS_PATH_BIG = 1u << 1,
    TFBS_PATH_WALK = 1u << 2,
    TFBS_PATH_STEPBITS = 1u << 3,
    TFBS_PATH_DIRTY_LISTED = 1u << 4,
    TFBS_PATH_COR_ARENA = 1u << 5,
    TFBS_PATH_LISTS_SLICED = 1u << 6,
    TFBS_PATH_RUNS_L2 = 1u << 7,
    TFBS_PATH_HAP_GLOBAL = 1u << 8,
    TFBS_PATH_U32 = 1u << 9,
    TFBS_PATH_CNT_ARENA = 1u << 10,
    TFBS_PATH_TICKET = 1u << 11,
    TFBS_PATH_GIVEUP = 1u << 12,
    TFBS_PATH_WHY_SHIFT = 13, /* 3 bits */
    TFBS_PATH_ASM = 1u << 16,
    TFBS_PATH_ASM_HAPS = 1u << 17,
    TFBS_PATH_ASM_RUNS = 1u << 18,
    TFBS_PATH_ASM_HITS = 1u << 19,
    TFBS_PATH_ASM_REFS = 1u << 20,
    TFBS_PATH_ASM_SCRATCH = 1u << 21
};
#define TFBS_PATH_WHY(word) (((word) >> TFBS_PATH_WHY_SHIFT) & 7u)
int tfbs_ctx_assembly_trace(tfbs_ctx *ctx, int on);
int tfbs_batch_assembly_paths(tfbs_ctx *ctx, const tfbs_batch *b, uint32_t *mask, uint32_t n);
/* The key assembly's static records of what was last uploaded (debug, read-only; made on the
 * device at every upload, the one-haplotype upload of tfbs_matches included).  region_asm: four
 * words per region -- run0, the lowest run offset (reference columns) of its haplotypes that
 * reuse the reference's hits, UINT32_MAX if none; nruns, the highest such offset + count minus
 * run0, 0 if none; lmax, the longest of its distinct haplotypes and of its reference haplotype;
 * 0.  hap_reuse: one word per uploaded haplotype -- UINT32_MAX unless it reuses, else (its run
 * offset - run0) | its runs << 16.  *n_regions / *n_haps get the sizes; both caps 0: only those. */
int tfbs_ctx_region_asm(tfbs_ctx *ctx, uint32_t *region_asm, size_t cap_regions, uint32_t *hap_reuse, size_t cap_haps,
                        size_t *n_regions, size_t *n_haps);
/* The figures of the last checked assembly (any ctx, trace on or off): out[0] regions left to
 * key_asm_kernel, out[1] arena words asked for, out[2] spill records, out[3] / out[4] 1 if it
 * launched the wide spill bucketing kernels / the leftover pass (a lean assembly leaves out
 * what the batch's last one did not need, TFBS_ASM_LEAN), and since the ctx was made: out[5]
 * lean assemblies run again in full, out[6] those of them that needed the wide kernels (more
 * than 8 192 spill records; the device flag a lean post_scan_kernel sets, cleared by the rerun --
 * or, for an assembly without the post-scan stage, the rerun's record count),
 * out[7] those that needed the leftover pass. */
int tfbs_ctx_assembly_figures(tfbs_ctx *ctx, uint64_t out[8]);
/* The post-scan stage (the overflow candidates' rescoring and the spill records' buckets) of the
 * last checked assembly: out[0] 1 if it was left out (a lean assembly leaves it out when the
 * batch's last checked assembly saw no candidate past the lists and at most TFBS_SPILL_INPLACE
 * spill records -- default 8 192, 0: none --, which the assembly's kernels then read where the
 * scan left them; under TFBS_ASM_LEAN=2 always), out[1] since the ctx was made the assemblies
 * that had left it out, reported a candidate or more records than that and ran again in full
 * (they count in out[5] of tfbs_ctx_assembly_figures too), out[2] 1 if the stage ran in the
 * scan kernel's last workgroup (TFBS_POST_FUSE=1, which turns the in-place reading off) and
 * not as a launch, 2 if it was left out and the records were read in place, out[3] the scan's
 * candidates past the waves' lists (out[2] of tfbs_ctx_assembly_figures: its spill records). */
int tfbs_ctx_post_figures(tfbs_ctx *ctx, uint64_t out[4]);
/* What the key assembly branches on, from the host batch (no device; the tests' proofs).
 * tfbs_batch_region_layout: out[0] the region's first distinct haplotype in the batch (the
 * scan groups haplotypes TFBS_MFMA_HAPS_PER_BLOCK at a time from 0), out[1] its distinct
 * haplotypes, out[2] the batch index of its reference haplotype (out[0] + out[1]: a helper
 * copy; UINT32_MAX: no haplotype reuses the reference's hits, none are listed), out[3] its
 * distinct inner ranges.
 * tfbs_batch_region_hap_runs: distinct haplotype h of the region -- *reuses 1 if it inherits
 * the reference's hits outside its dirty windows; its diff runs in the reference's columns
 * (window w of a strand of length L is dirty iff some run [a, b] has a <= w + L - 1 and
 * b >= w; b = UINT32_MAX: to the end; [a, a - 1]: two touching segments): *n_runs of them at
 * *run_off of the batch's run array (key_fast_kernel stages the span from the region's lowest
 * offset to its highest end), the first cap as (a, b) pairs in ab.
 * tfbs_batch_region_hap_own_runs: the same haplotype's diff runs in its own columns, which
 * decide the windows the matrix-core scan reads and whose hits it lists (the window lists and
 * the rescoring's dirty test, with the same predicate over the haplotype's windows); the same
 * arguments and errors.  The list of tfbs_batch_region_hap_runs itself when every column of
 * the haplotype stands at its reference column (no indel); otherwise a list of its own, which
 * that one follows in the run array, and either may be empty while the other is not (equal
 * *run_off: one list, or no run in the haplotype's own columns). */
int tfbs_batch_region_layout(const tfbs_batch *b, size_t region, uint32_t out[4]);
int tfbs_batch_region_hap_runs(const tfbs_batch *b, size_t region, uint32_t h, int *reuses, uint32_t *run_off,
                               uint32_t *n_runs, uint32_t *ab, uint32_t cap);
int tfbs_batch_region_hap_own_runs(const tfbs_batch *b, size_t region, uint32_t h, int *reuses, uint32_t *run_off,
                                   uint32_t *n_runs, uint32_t *ab, uint32_t cap);
/* counts_as_genotypes' per-sample half on the device (main.rs:439-534, SURVEY.md
 * 8(f) f1) for the varying keys of regions [r0, r1) after tfbs_batch_reduce:
 * per key v[s] = C[hap(2s)] + C[hap(2s+1)] over the samples, min / max, the
 * sorted distinct values with their sample counts, and one u8 code per sample;
 * rows of these regions are then formatted from the codes (no per-sample
 * count gather on the host).  Keys whose region has > 65 535 distinct haplotypes
 * (u16 membership) or > 8 192 distinct (left, right) haplotype pairs (the LDS pair
 * table, pair_table_kernel), or with > 255 distinct totals or a total range >= 65 536,
 * keep the host path (tfbs_internal.hpp kEncMax*). */
int tfbs_batch_encode(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1);
/* tfbs_batch_encode with flags: TFBS_ENC_DEVICE_CODES keeps the per-sample codes on
 * the device only (for tfbs_batch_rows_bgzf; host row functions then take their
 * slower path for these keys). */
#define TFBS_ENC_DEVICE_CODES 1
int tfbs_batch_encode_flags(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, int flags);
/* Which path the keys of the last tfbs_batch_encode call took (read-only, zeros
 * before one): out[0] the varying keys of its regions, out[1] / out[2] / out[3] those
 * encoded with 2- / 4- / 8-bit codes, out[4] those not encoded because their
 * region's haplotype pairs were not listed (> 8 192 pairs or > 65 535 distinct
 * haplotypes), out[5] those left to the host for their total range (>= 65 536),
 * out[6] for their number of distinct totals (> 255).  out[0] is the sum of the rest. */
int tfbs_batch_encode_stats(const tfbs_batch *b, uint64_t out[7]);

/* The rows of regions [r0, r1) (main.rs:415-429, same text as tfbs_batch_rows) as
 * BGZF blocks (main.rs:258-290's BGzWriter) built on the GPU
 * after tfbs_batch_encode over them: row heads formatted on the host, the
 * per-sample genotype text generated from the device codes and deflated there
 * (deflate, CRC32), so the text never crosses PCIe.  Whole blocks -- the last one
 * shorter -- are written to file descriptor fd (after the header's blocks);
 * *fake_position is the POS counter, advanced per row; *bytes / *n_rows /
 * *text_bytes (optional) receive the bytes written, the rows and their
 * uncompressed bytes. */
int tfbs_batch_rows_bgzf(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome,
                         uint32_t min_maf, uint32_t *fake_position, int fd, uint64_t *bytes, uint64_t *n_rows,
                         uint64_t *text_bytes);
/* Seconds spent in tfbs_batch_rows_bgzf on this ctx so far: out[0] the row plan on
 * the host (heads, token tables), out[1] the rest (uploads, kernels, copy-back, write). */
int tfbs_ctx_rows_bgzf_seconds(const tfbs_ctx *ctx, double *out);
/* The BGZF blocks of the last tfbs_batch_rows_bgzf call on this ctx (read-only):
 * out[0] the blocks written, out[1] those whose rows were all staged (deflated by
 * bgzf_wave_kernel; the others by bgzf_block_kernel), out[2] those that did not
 * deflate to half their size and were stored (BTYPE 00). */
int tfbs_ctx_rows_bgzf_blocks(const tfbs_ctx *ctx, uint64_t out[3]);

/* After download: count_matches_by_sample (main.rs:500-534), keys ordered by
 * (inner.start, inner.end, bed basename, pattern_id).  keys are per region. */
int tfbs_batch_region_num_keys(const tfbs_batch *b, size_t region, size_t *n);
int tfbs_batch_region_key(const tfbs_batch *b, size_t region, size_t k, uint32_t *bed, uint64_t *start,
                          uint64_t *end, uint16_t *pattern_id, uint32_t *left, uint32_t *right);
/* counts_as_genotypes + row emission (main.rs:415-429, 439-498) for every
 * region, in region order.  Appends rows to *text (malloc'd; free with
 * tfbs_free); *fake_position is the POS counter, advanced per row. */
int tfbs_batch_rows(const tfbs_batch *b, const char *chromosome, uint32_t min_maf, uint32_t *fake_position,
                    char **text, size_t *len);
/* The rows of one region (main.rs:415-429 for one process_peak call), same
 * format and POS handling as tfbs_batch_rows. */
int tfbs_batch_region_rows(const tfbs_batch *b, size_t region, const char *chromosome, uint32_t min_maf,
                           uint32_t *fake_position, char **text, size_t *len);
/* 64-bit digest of one region's keys at the distinct-haplotype level (key
 * identity in row order + every distinct haplotype's count): equal digests
 * from the dense download and the device reduction, or from a sharded and an
 * unsharded batch, mean equal count_matches_by_sample maps (main.rs:500-534). */
int tfbs_batch_region_digest(const tfbs_batch *b, size_t region, uint64_t *digest);
/* Order-free digest: the sum over the region's keys of a hash of the key (bed,
 * range, multiplicity, pattern_id) and its distinct haplotypes' counts.  Batches
 * over disjoint pattern_id shards of one pattern set (same windows: see
 * tfbs_batch_set_window_lmax) sum to the unsharded batch's digest. */
int tfbs_batch_region_key_digest_sum(const tfbs_batch *b, size_t region, uint64_t *digest);
/* Digest of what the host prep packed for a region (window, inner keys, distinct
 * haplotypes' bases / N masks / positions, carriers, membership): equal for the
 * same region built in any batch or shard. */
int tfbs_batch_region_input_digest(const tfbs_batch *b, size_t region, uint64_t *digest);
/* Canonical per-region digests of regions [r0, r1) (the full-size golden files of
 * tests/golden/, made by the oracle's orc_job_digests; no reference counterpart):
 * keys[i] = the sum over the region's keys of a hash of (bed index, start, end,
 * pattern_id, S) with S = sum over samples s of L[s] w(2s) + R[s] w(2s + 1) mod 2^64
 * (w = splitmix64; count_matches_by_sample's vectors, main.rs:500-534, as a linear
 * sketch computed from the distinct haplotypes' counts and the membership);
 * rows[i] = XXH64 (seed 0) of the region's rows with their "<chr>\t<POS>\t"
 * prefix removed (main.rs:415-429), n_rows[i] their number.  Regions run on
 * `threads` host threads; keys or rows (with n_rows) may be null to skip that digest.
 * Needs the counts (download or reduce) and the membership. */
int tfbs_batch_region_digests(const tfbs_batch *b, size_t r0, size_t r1, uint32_t min_maf, uint32_t threads,
                              uint64_t *keys, uint64_t *rows, uint64_t *n_rows);
/* Distinct haplotypes (number_of_haplotypes, main.rs:97-130) and records (variant_count) of a region. */
int tfbs_batch_region_stats(const tfbs_batch *b, size_t region, uint32_t *n_haplotypes, uint32_t *n_variants);
/* Formats the rows of regions [r0, r1) (main.rs:415-429) on `threads` host threads and
 * discards them: the row count and bytes (without POS digits).  The bench's
 * end-to-end leg times it; tfbs_run writes the same rows. */
int tfbs_batch_format_rows(const tfbs_batch *b, const char *chromosome, uint32_t min_maf, uint32_t threads,
                           size_t r0, size_t r1, uint64_t *n_rows, uint64_t *n_bytes);
/* Host prep seconds of the batch's synthetic fills (out[4]): generation and
 * build_region (thread CPU-seconds, summed), build_region + the serial commit
 * (wall: the prep a BCF reader's records go through) and the whole fill (wall,
 * generation included). */
int tfbs_batch_prep_seconds(const tfbs_batch *b, double *out);
/* ------------------------------------------------------------------ */
/* Hit lists: find_all_matches (main.rs:94-154) kept, not counted        */
/* ------------------------------------------------------------------ */
/* One matching site.  For a region of a batch the hit list is every (distinct
 * haplotype h, pattern strand p, window i) with: h one of the region's n_haplotypes
 * distinct haplotypes (helper reference copies are not included); p a TFBS_KIND_PWM or
 * TFBS_KIND_DIPWM strand of L bases (TFBS_KIND_OTHER never matches); i + L <= len(h);
 * score > min_score.  score is the count path's: the wrapping int32 sum of the columns'
 * weights (an N column adds 0; any L) or of the pair weights (a pair holding an N adds
 * 0).  The match range is [pos[i], pos[i] + L - 1] (pattern.rs:157-160); inner ranges
 * play no part.  Hits are sorted by (region, haplotype, pattern, window). */
typedef struct tfbs_hit {
    uint32_t region, haplotype, pattern, window; /* batch region, distinct haplotype of the region,
                                                    pattern index in creation order, window start (base index) */
    uint64_t start, end;
    int32_t score;
    uint32_t reserved;
} tfbs_hit;

/* find_all_matches (main.rs:94-154) for regions [r0, r1) of the batch resident on ctx
 * (after tfbs_batch_upload; needs no scan; leaves every scan / reduce / encode result
 * and later step untouched).  *out is malloc'd (tfbs_free), sorted as specified.  Its
 * own kernel (scan_hits.hip) scores every window of every distinct haplotype from the
 * pattern set alone; the device scratch (counters, offsets and records) of one pass is
 * bounded by TFBS_HITS_SCRATCH_MB (default 256; at least one haplotype; read at the
 * call) and the result does not depend on it.  TFBS_E_STATE for a batch not resident. */
int tfbs_batch_hits(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_hit **out, size_t *n);
/* The count pass alone: per_region[r - r0]. */
int tfbs_batch_hits_count(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint64_t *per_region);
/* Device time (ms, HIP events on the ctx stream, summed over the scratch chunks) of the
 * last tfbs_batch_hits / tfbs_batch_hits_count: out[0] the count pass, out[1] the offset
 * scan, out[2] the fill pass; out[3] the copy-back and host part (wall ms). */
int tfbs_ctx_last_hits_ms(const tfbs_ctx *ctx, double out[4]);
/* Host only.  Distinct haplotype h of a region as load_haplotypes made it
 * (codes 0-4, NucleotidePos.pos) and its number of carrier ids.
 * TFBS_E_ARG with *n = the need when cap is short. */
int tfbs_batch_region_haplotype(const tfbs_batch *b, size_t region, uint32_t h, uint8_t *nucs, uint64_t *pos,
                                size_t cap, size_t *n, uint32_t *carriers);
/* Host only.  out[id] = distinct index of haplotype id 2*sample+side (2 * n_samples entries).
 * Fetches a device-grouped row through region_membership.
 * TFBS_E_STATE without keep_membership. */
int tfbs_batch_region_membership(const tfbs_batch *b, size_t region, uint32_t *out);
/* Host only.  Formats hits (a tfbs_batch_hits result for whole regions) as TSV, one
 * line per record, tab-separated, under the header
 *   #chrom region haplotype carriers kind name pattern_id strand start end score carrier_ids
 * chrom = `chromosome` as given, region = <merged_start>-<merged_end>, haplotype = the
 * distinct index, carriers = its number of carrier ids, strand + or -.
 * TFBS_HITS_ALL: one `hit` line per hit in list order, carrier_ids ".".
 * TFBS_HITS_DIFF (every region of the batch, one without hits included: pass the hits of all of
 * them): per region the baseline is the distinct haplotype with the most
 * carrier ids (ties: the one holding the lowest haplotype id).  Each distinct haplotype
 * in index order writes one `hap` line (pattern fields ".", carrier_ids its ascending
 * haplotype ids comma-joined, "*" for the baseline, "." without membership), then -- the
 * baseline -- its hits as `base` lines, or -- any other -- its `gain` lines in (pattern,
 * window) order and its `loss` lines in (pattern, baseline window) order, a loss carrying
 * the baseline hit's range and score.  Hits compare as a multiset on (pattern, start,
 * end): of n_h hits of the haplotype and n_b of the baseline under one key the last
 * n_h - n_b of the haplotype's in window order are gains, or the last n_b - n_h of the
 * baseline's are losses; a hit present in both with another score is neither.
 * The header line is not part of *text (malloc'd, tfbs_free). */
#define TFBS_HITS_ALL 0
#define TFBS_HITS_DIFF 1
#define TFBS_HITS_HEADER "#chrom\tregion\thaplotype\tcarriers\tkind\tname\tpattern_id\tstrand\tstart\tend\tscore\tcarrier_ids\n"
int tfbs_batch_hits_tsv(const tfbs_batch *b, const tfbs_hit *hits, size_t n, const char *chromosome, int mode,
                        char **text, size_t *len);

/* ------------------------------------------------------------------ */
/* Best sites: the threshold-free best score per haplotype, strand and  */
/* inner range                                                          */
/* ------------------------------------------------------------------ */
/* One best record.  Take a region of a batch, h one of its n_haplotypes distinct
 * haplotypes (helper reference copies are not included), p a pattern strand in creation
 * order of L bases, k one of the region's distinct non-empty inner ranges, numbered in
 * ascending (start, end) order (tfbs_batch_region_range).  Window i of h exists for p iff
 * i + L <= len(h); its match range is [pos[i], pos[i] + L - 1] (pattern.rs:157-160) and its
 * score the count path's and the hit list's (the wrapping int32 column sum, an N column
 * adding 0, any L; or the wrapping int32 pair sum, a pair holding an N adding 0).  Window i
 * belongs to range k iff range_overlaps(inner_k, match) (range.rs:18-21, the count path's
 * asymmetric rule: the match's start or its end lies inside the inner range).
 *   n_windows  the windows that belong to k
 *   score      the maximum of their wrapped scores, compared as signed int32
 *   window     the lowest i attaining it
 *   start, end that window's match range
 * n_windows == 0 (TFBS_KIND_OTHER, a haplotype shorter than L, no window overlapping the
 * range): score = INT32_MIN, window = UINT32_MAX, start = end = 0; n_windows tells a genuine
 * INT32_MIN from this.  min_score and the bed multiplicity play no part; empty inner ranges
 * (end < start) have no record.  The result is dense: every (region, h, p, k) has exactly
 * one record, sorted by (region, haplotype, pattern, range), so regions [r0, r1) give
 * sum_r n_haplotypes(r) * n_patterns * n_ranges(r) records and a region's block reshapes to
 * [h][p][k]. */
typedef struct tfbs_best {
    uint32_t region, haplotype, pattern, range;
    uint32_t window, n_windows;
    int32_t score;
    uint32_t reserved;
    uint64_t start, end;
} tfbs_best; /* 48 bytes */

/* The best records of regions [r0, r1) of the batch resident on ctx (after
 * tfbs_batch_upload; needs no scan; leaves every scan / reduce / encode result and later
 * step untouched).  *out is malloc'd (tfbs_free).  Its own kernel (scan_best.hip) scores
 * every window of every distinct haplotype with the hit list's scoring code and reduces
 * per range; it works in chunks of whole haplotypes whose device records fit
 * TFBS_BEST_SCRATCH_MB (default 256; at least one haplotype; read at the call) and the
 * result does not depend on it.  TFBS_E_STATE for a batch not resident, TFBS_E_ARG for
 * r0 > r1 or r1 > num_regions; an empty range of regions or an empty pattern set gives
 * *n = 0. */
int tfbs_batch_best(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_best **out, size_t *n);
/* Host only.  The region's distinct non-empty inner ranges (tfbs_best.range indexes them)
 * and range k of them, in ascending (start, end) order. */
int tfbs_batch_region_num_ranges(const tfbs_batch *b, size_t region, size_t *n);
int tfbs_batch_region_range(const tfbs_batch *b, size_t region, size_t k, uint64_t *start, uint64_t *end);
/* The last tfbs_batch_best's times (ms): out[0] the kernel (HIP events on the ctx stream,
 * summed over the scratch chunks), out[1] the copy-back and host part (wall). */
int tfbs_ctx_last_best_ms(const tfbs_ctx *ctx, double out[2]);
/* Host only.  Formats best records as TSV, tab-separated, under the header
 *   #chrom region bed inner_start inner_end name pattern_id haplotype carriers kind strand start end score delta carrier_ids
 * The n records passed must be whole regions (each region's n_haplotypes * n_patterns *
 * n_ranges records, regions ascending), not the whole batch: the text of a batch is the
 * concatenation of its regions' texts, so a caller may format one region at a time.  A
 * region without a record (no non-empty inner range, no pattern) writes nothing.
 * Lines are per pattern_id, not per strand: the value of (haplotype, pattern_id, key) is
 * the best over the pattern_id's strands -- the highest score, ties to the strand earlier
 * in creation order; a strand with n_windows == 0 never wins; all of them so: "none".
 * Keys are the region's (bed, inner range) pairs with a non-empty range, each once
 * whatever its multiplicity, in the rows' order (inner start, inner end, bed as
 * registered); under a key ascending pattern_id, then the haplotype index.  chrom, region,
 * haplotype, carriers, name and strand are the hit TSV's; bed is the registered basename.
 * TFBS_BEST_ALL: one `best` line per (key, pattern_id, haplotype); a "none" value writes
 * "." for strand, start, end and score; delta and carrier_ids are ".".
 * TFBS_BEST_DIFF: per region the hit TSV's baseline (the distinct haplotype with the most
 * carrier ids, ties: the one holding the lowest haplotype id) and first its `hap` lines
 * as the hit TSV's diff mode writes them (bed, inner_start, inner_end, name, pattern_id,
 * strand, start, end, score and delta "."); then for each (key, pattern_id) where some
 * haplotype's value differs from the baseline's in score or in being "none" one `base`
 * line for the baseline and one `alt` line per differing haplotype in index order.  delta
 * on an `alt` line is the haplotype's score minus the baseline's as a signed 64-bit
 * difference (no wrap), "." when either is "none"; elsewhere ".".  A (key, pattern_id)
 * where nothing differs writes nothing.
 * The header line is not part of *text (malloc'd, tfbs_free). */
#define TFBS_BEST_ALL 0
#define TFBS_BEST_DIFF 1
#define TFBS_BEST_HEADER "#chrom\tregion\tbed\tinner_start\tinner_end\tname\tpattern_id\thaplotype\tcarriers\tkind\tstrand\tstart\tend\tscore\tdelta\tcarrier_ids\n"
int tfbs_batch_best_tsv(const tfbs_batch *b, const tfbs_best *best, size_t n, const char *chromosome, int mode,
                        char **text, size_t *len);

/* ------------------------------------------------------------------ */
/* Binding affinity: per distinct haplotype, pattern strand and inner  */
/* range the sum over every window of exp(score), in exact fixed point */
/* ------------------------------------------------------------------ */
/* The weight of a window d >= 0 milli-log-odds below the reference score, in Q40:
 *   a(d) = floor(2^40 * exp(-d / 1000))
 * a mathematical definition: a(0) = 2^40, a(27725) = 1, a(d) = 0 for every d >= 27726
 * (1000 ln 2^40 = 27725.89).  Host and device realise it from two committed tables,
 * T1[r] = floor(2^63 exp(-r / 1000)), r < 1000, and T2[q] = floor(2^63 exp(-q)), q < 28, as
 * umul64hi(T1[d % 1000], T2[d / 1000]) >> 22, which equals the definition on all of
 * [0, 27726] (tools/gen_affinity_tables.py writes the tables with 80-digit decimals). */
uint64_t tfbs_affinity_weight(uint64_t d);
/* The reference score top(q) of a pattern_id q: the maximum over q's TFBS_KIND_PWM and
 * TFBS_KIND_DIPWM strands of sum_j max(0, max_b w_j[b]) (b over A, C, G, T; a dinucleotide
 * strand: over its rows of 16), the C of the matrix-core bound: an N column or a pair holding
 * an N adds 0, so top(q) - score >= 0 for every window of every strand of q.  out takes one
 * value per strand in creation order (tfbs_patterns_count entries): its pattern_id's top, 0
 * for a TFBS_KIND_OTHER strand.  TFBS_E_ARG naming the strand when a strand's sums can wrap
 * int32 (sum_j max(|lo_j|, |hi_j|) > INT32_MAX, tfbs_patterns_score_tails' rule). */
int tfbs_patterns_affinity_tops(const tfbs_patterns *p, int32_t *out);
/* One (distinct haplotype h, pattern strand p, inner range k) of a region; h, p, k, window
 * existence, match range and range membership are the best sites', scores the hit list's.
 *   n_windows  the windows that belong to k (tfbs_best.n_windows)
 *   n_nonzero  those of them with a(d) > 0, d = top(pattern_id of p) - score
 *   sum        the sum of a(d) over them
 * A TFBS_KIND_OTHER strand, a haplotype shorter than L and a range without a window give
 * zeros.  No floating point takes part: the sum is the same for any lane order, chunking,
 * scratch budget and device.  The strands of a pattern_id share one top, so their records
 * add, and so do a sample's two haplotypes: ln(affinity) = top / 1000 + ln(sum) - 40 ln 2.
 * Dense and sorted by (region, haplotype, pattern, range) as the best records; min_score and
 * the bed multiplicity play no part; empty inner ranges have no record. */
typedef struct tfbs_affinity {
    uint32_t region, haplotype, pattern, range;
    uint32_t n_windows, n_nonzero;
    uint64_t sum;
} tfbs_affinity; /* 32 bytes */
/* The affinity records of regions [r0, r1) of the batch resident on ctx (after
 * tfbs_batch_upload; needs no scan; leaves every scan / reduce / encode / rows / hits / best /
 * scores / effects / mutscan result and the step graph untouched).  *out is malloc'd
 * (tfbs_free).  Its own kernel (scan_affinity.hip) walks every window as the best-site kernel
 * does and sums the weights per range; chunks of whole haplotypes whose device records fit
 * TFBS_AFFINITY_SCRATCH_MB (default 256; at least one haplotype; read at the call), and the
 * result does not depend on it.  The ctx's first call uploads the two tables and the tops.
 * Errors as tfbs_batch_best; TFBS_E_ARG also for a batch of another pattern set than the
 * ctx's, when a strand's sums can wrap int32 (tfbs_patterns_affinity_tops) and for a region
 * whose longest haplotype times the most strands of one pattern_id reaches 2^23 (every fold
 * stays below 2^63). */
int tfbs_batch_affinity(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_affinity **out, size_t *n);
/* The last tfbs_batch_affinity's times (ms): out[0] the kernel (HIP events on the ctx stream,
 * summed over the scratch chunks), out[1] the copy-back and host part (wall). */
int tfbs_ctx_last_affinity_ms(const tfbs_ctx *ctx, double out[2]);
/* Host only.  Formats affinity records as TSV, tab-separated, under the header
 *   #chrom region bed inner_start inner_end name pattern_id haplotype carriers kind top n_windows affinity delta carrier_ids
 * The records are whole regions, as tfbs_batch_best_tsv's; a region without a record writes
 * nothing.  Lines are per pattern_id: the value of (haplotype, pattern_id, key) is A = the sum
 * of `sum` and N = the sum of n_windows over the pattern_id's strands; N == 0: "none".  Keys,
 * their order, chrom, region, bed, name, haplotype, carriers, the baseline and the `hap`
 * lines (the seven columns bed .. pattern_id and top .. delta ".") are the best TSV's.
 * TFBS_AFFINITY_ALL: one `aff` line per (key, pattern_id, haplotype) with top, N and A; a
 * "none" value writes "." for n_windows and affinity; delta and carrier_ids are ".".
 * TFBS_AFFINITY_DIFF: the `hap` lines first; then for each (key, pattern_id) where some
 * haplotype differs from the baseline in A or in being "none" one `base` line and one `alt`
 * line per differing haplotype in index order; delta on an `alt` line is A - A_base as a
 * signed 64-bit number, "." when either is "none"; elsewhere ".".
 * The header line is not part of *text (malloc'd, tfbs_free). */
#define TFBS_AFFINITY_ALL 0
#define TFBS_AFFINITY_DIFF 1
#define TFBS_AFFINITY_HEADER "#chrom\tregion\tbed\tinner_start\tinner_end\tname\tpattern_id\thaplotype\tcarriers\tkind\ttop\tn_windows\taffinity\tdelta\tcarrier_ids\n"
int tfbs_batch_affinity_tsv(const tfbs_batch *b, const tfbs_affinity *aff, size_t n, const char *chromosome,
                            int mode, char **text, size_t *len);

/* ------------------------------------------------------------------ */
/* Variant effects: per record the best site touching it on the REF and */
/* on the ALT allele, per pattern strand                                */
/* ------------------------------------------------------------------ */
/* Before the batch's first region: on != 0 makes every region keep its fetched reference
 * codes and a compact copy of each record (pos, REF and ALT codes, n_alleles, the number of
 * carrier ids, the status below), on every build path.  Default off: the batch is then
 * byte for byte what it was (memory, digests, device bytes) and the effects calls return
 * TFBS_E_STATE.  TFBS_E_STATE once a region is open or added. */
int tfbs_batch_keep_variants(tfbs_batch *b, int on);
/* A record's status, tested in this order: n_alleles != 2 (load_diffs counts it and never
 * applies it); no selected haplotype id carries ALT; patching this record alone into the
 * window is refused (TFBS_E_REFMISMATCH / TFBS_E_MNP -- reachable in a region that builds:
 * an overlapping diff truncates a haplotype without a REF check, so a bad-REF SNV inside a
 * deletion that all its carriers also carry builds fine and fails alone); else scored. */
#define TFBS_VAR_SCORED 0
#define TFBS_VAR_MULTIALLELIC 1
#define TFBS_VAR_NO_CARRIER 2
#define TFBS_VAR_UNPATCHED 3
/* Host only.  Record v (BCF order, v < the n_variants of tfbs_batch_region_stats) of a region
 * of a batch that keeps its variants: REF / ALT as nucleotide codes 0-4 into ref / alt (cap
 * entries each).  *n_ref / *n_alt are always set: TFBS_E_ARG on a short cap tells the need,
 * as tfbs_batch_region_haplotype does.  TFBS_E_STATE without tfbs_batch_keep_variants. */
int tfbs_batch_region_variant(const tfbs_batch *b, size_t region, size_t v, uint64_t *pos, uint8_t *ref, uint8_t *alt,
                              size_t cap, size_t *n_ref, size_t *n_alt, uint32_t *n_alleles, uint32_t *carriers,
                              uint32_t *status);
/* One effect record: region, record v of it, pattern strand p in creation order (L bases).
 * For a scored record let R = patch_haplotype((es, ee), [], ref) and A = patch_haplotype((es,
 * ee), [v], ref), both sequences of (code, pos) columns; a = the length of their longest
 * common prefix (code and pos equal), z = that of their longest common suffix with
 * z <= min(len R, len A) - a.  Window i of side X (n = len X) is *affected* iff i + L <= n,
 * i + L > a and i < n - z: it exists and lies neither wholly in the common prefix nor wholly
 * in the common suffix.  (An SNV: the L windows covering the site, clipped at the ends; an
 * insertion: the reference windows spanning the junction; a deletion: the alt windows
 * spanning it; a record outside the window, A == R: none; a deletion running to the
 * window's end, A a prefix of R: none on the alt side.)
 *   n_ref, ref_score, ref_window   the affected windows of R, the maximum of their scores
 *                                  (signed int32), the lowest i attaining it
 *   n_alt, alt_score, alt_window   the same on A
 *   ref_start .. alt_end           pos_X[i] and pos_X[i] + L - 1 of the two best windows
 * Scores are the hit list's and the best sites' (wrapping int32 column sum, an N column
 * adding 0, any L; wrapping int32 pair sum, a pair holding an N adding 0).  A side without an
 * affected window (TFBS_KIND_OTHER, a side shorter than L, an unscored record) holds
 * score = INT32_MIN, window = UINT32_MAX, start = end = 0; n_ref / n_alt tell that from a
 * genuine INT32_MIN.  min_score, the inner ranges and the bed multiplicity play no part.
 * Dense and sorted by (region, variant, pattern): regions [r0, r1) give
 * sum_r n_variants(r) * n_patterns records, a region's block reshapes to [v][p]. */
typedef struct tfbs_effect {
    uint32_t region, variant, pattern, status;
    uint32_t n_ref;
    int32_t ref_score;
    uint32_t ref_window;
    uint32_t n_alt;
    int32_t alt_score;
    uint32_t alt_window;
    uint64_t ref_start, ref_end, alt_start, alt_end;
} tfbs_effect; /* 72 bytes */
/* The effect records of regions [r0, r1) of a batch that keeps its variants, on a ctx made
 * from the batch's pattern set (needs neither upload nor scan; leaves every scan / reduce /
 * encode / rows result and the step graph untouched).  *out is malloc'd (tfbs_free).  The
 * host patches R once per region and A per scored record and packs both; its own kernel
 * (scan_effects.hip) scores only the affected windows with the hit list's scoring code, one
 * wave per (scored record, strand).  It works in chunks of whole records whose packed image
 * and device records fit TFBS_EFFECTS_SCRATCH_MB (default 256, fractions allowed; at least
 * one record; read at the call) and the result does not depend on it.  TFBS_E_STATE without
 * tfbs_batch_keep_variants, TFBS_E_ARG for r0 > r1 or r1 > num_regions; an empty range of
 * regions or an empty pattern set gives *n = 0. */
int tfbs_batch_effects(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, tfbs_effect **out, size_t *n);
/* The last tfbs_batch_effects' times (ms): out[0] the host's patching and packing (wall),
 * out[1] the kernel (HIP events on the ctx stream, summed over the scratch chunks), out[2]
 * the copy-back and the host's expansion (wall). */
int tfbs_ctx_last_effects_ms(const tfbs_ctx *ctx, double out[3]);
/* Host only.  Formats effect records (whole regions, ascending) as TSV, tab-separated, under
 * the header
 *   #chrom region variant pos ref alt carriers kind name pattern_id strand ref_start ref_end ref_score alt_start alt_end alt_score delta
 * chrom and region are the hit TSV's.  Per region and record in order first one `var` line:
 * pos, ref, alt, the carrier count, in `name` the status as scored|multiallelic|no_carrier|
 * unpatched, every other field ".".  Then, for a scored record, one line per pattern strand
 * in creation order (name, pattern_id, strand + or -).  A side passes iff n > 0 and
 * score > the strand's min_score; kind is gain (only alt passes), loss (only ref passes),
 * change (both, scores differ), same (both, scores equal), none (neither).
 * TFBS_EFFECTS_SITES writes gain, loss and change lines; TFBS_EFFECTS_ALL all five kinds,
 * for every strand with n_ref + n_alt > 0.  A side with n == 0 writes "." for its three
 * fields; delta is alt_score - ref_score as a signed 64-bit difference, "." when either side
 * has no window.  A batch's text is the concatenation of its regions' texts.
 * The header line is not part of *text (malloc'd, tfbs_free). */
#define TFBS_EFFECTS_SITES 0
#define TFBS_EFFECTS_ALL 1
#define TFBS_EFFECTS_HEADER "#chrom\tregion\tvariant\tpos\tref\talt\tcarriers\tkind\tname\tpattern_id\tstrand\tref_start\tref_end\tref_score\talt_start\talt_end\talt_score\tdelta\n"
int tfbs_batch_effects_tsv(const tfbs_batch *b, const tfbs_effect *e, size_t n, const char *chromosome, int mode,
                           char **text, size_t *len);

/* ------------------------------------------------------------------ */
/* Mutation scan: every possible SNV of a region's reference window,    */
/* per pattern strand                                                   */
/* ------------------------------------------------------------------ */
/* For a region of a batch made with tfbs_batch_keep_variants let R = patch_haplotype((es,
 * ee), [], ref), n columns of (code, pos): the R of the variant effects.  A substitution is
 * (c, b): a column c with R[c] in {A,C,G,T} and a base b in {A,C,G,T}, b != R[c]; an N column
 * has none.  The mutation record of (region, pattern strand p of L bases, c, b) is, field for
 * field, the effect record tfbs_batch_effects gives for a scored bi-allelic SNV record
 * (pos_R[c], REF = R[c], ALT = b) of that region and strand:
 *   n_windows               the affected windows i: i + L <= n and c - L + 1 <= i <= c (the
 *                           effects' rule with a = c, z = n - 1 - c); the same on both sides
 *   ref_score, ref_window   the maximum of their scores on R (signed int32), the lowest i
 *                           attaining it
 *   alt_score, alt_window   the same on R with column c set to b
 *   ref_start .. alt_end    pos_R[window] and that plus L - 1
 *   kind                    the effects TSV's: a side passes iff score > the strand's
 *                           min_score; 0 gain (only alt passes), 1 loss (only ref), 2 change
 *                           (both, scores differ), 3 same (both, equal), 4 none (neither)
 * Scores are the hit list's (wrapping int32 column sum, an N column adding 0, any L; wrapping
 * int32 pair sum, a pair holding an N adding 0).  A record exists iff the strand is
 * TFBS_KIND_PWM or TFBS_KIND_DIPWM, n_windows > 0 and its kind is in the call's `kinds` mask.
 * The result is sparse and sorted by (region, pattern, column, alt base).  Inner ranges, the
 * bed multiplicity and the region's BCF records play no part. */
#define TFBS_MUT_GAIN 1
#define TFBS_MUT_LOSS 2
#define TFBS_MUT_CHANGE 4
#define TFBS_MUT_SAME 8
#define TFBS_MUT_NONE 16
#define TFBS_MUT_SITES 7
#define TFBS_MUT_ALL 31
typedef struct tfbs_mutation {
    uint32_t region, column, pattern; /* offsets 0, 4, 8 */
    uint8_t ref, alt, kind, reserved; /* 12 .. 15: codes 0-3; kind 0 gain .. 4 none */
    uint64_t pos;                     /* 16: pos_R[column] */
    uint32_t n_windows;               /* 24 */
    int32_t ref_score;                /* 28 */
    uint32_t ref_window;              /* 32 */
    int32_t alt_score;                /* 36 */
    uint32_t alt_window;              /* 40 */
    uint32_t reserved1;               /* 44 */
    uint64_t ref_start, ref_end, alt_start, alt_end; /* 48, 56, 64, 72 */
} tfbs_mutation; /* 80 bytes */
/* The mutation records of regions [r0, r1) whose kind is in `kinds`, on a ctx made from the
 * batch's pattern set (needs neither upload nor scan; leaves every scan / reduce / encode /
 * rows / hits / best / scores / effects result and the step graph untouched).  *out is
 * malloc'd (tfbs_free).  The host packs each region's R once; the kernel (scan_mutscan.hip)
 * scores every reference window once, keeps the scores in a ring in LDS and forms each alt
 * score as the reference score plus one weight difference (two pair-weight differences for a
 * dinucleotide strand), one wave per (region, strand); a count pass, an exclusive scan and a
 * fill pass place the records without atomics or a sort.  Strands longer than
 * tfbs_mutscan_ring_max_length() bases take a slower exact path.  It works in chunks of
 * whole regions, and fills in runs of whole (region, strand) pairs, that fit
 * TFBS_MUTSCAN_SCRATCH_MB (default 256, fractions allowed; one region and one pair at least;
 * read at the call); the result does not depend on it.  TFBS_E_STATE without
 * tfbs_batch_keep_variants; TFBS_E_ARG for r0 > r1, r1 > num_regions, kinds == 0,
 * kinds > TFBS_MUT_ALL or a ctx of another pattern set; an empty range of regions or an empty
 * pattern set gives *n = 0. */
int tfbs_batch_mutscan(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint32_t kinds, tfbs_mutation **out,
                       size_t *n);
/* The count pass alone: *n = the records tfbs_batch_mutscan would give. */
int tfbs_batch_mutscan_count(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, uint32_t kinds, uint64_t *n);
/* The longest strand (bases) that the kernel's ring of window scores serves. */
uint32_t tfbs_mutscan_ring_max_length(void);
/* The last mutation scan's times (ms): out[0] the host's packing (wall), out[1] the count
 * pass and the offset scan, out[2] the fill pass (HIP events on the ctx stream, summed over
 * the scratch chunks), out[3] the copy-back and the host's expansion (wall). */
int tfbs_ctx_last_mutscan_ms(const tfbs_ctx *ctx, double out[4]);
/* Host only.  Formats mutation records (any records of the batch, in list order: they are
 * self-contained) as TSV, tab-separated, one line per record, under the header
 *   #chrom region pos ref alt kind name pattern_id strand ref_start ref_end ref_score alt_start alt_end alt_score delta
 * chrom, region, name and strand are the effects TSV's; delta is alt_score - ref_score as a
 * signed 64-bit difference.  The header line is not part of *text (malloc'd, tfbs_free). */
#define TFBS_MUTSCAN_HEADER "#chrom\tregion\tpos\tref\talt\tkind\tname\tpattern_id\tstrand\tref_start\tref_end\tref_score\talt_start\talt_end\talt_score\tdelta\n"
int tfbs_batch_mutscan_tsv(const tfbs_batch *b, const tfbs_mutation *m, size_t n, const char *chromosome, char **text,
                           size_t *len);

/* ------------------------------------------------------------------ */
/* Score rows: per-sample best-score genotypes as a second VCF          */
/* ------------------------------------------------------------------ */
/* The rows of the main output count the sites above min_score; a score row carries how
 * strongly a sample binds.  Keys, pattern ids and values are the best TSV's: a key is a
 * (bed, inner range) pair with a non-empty range, taken once, in the rows' order (inner
 * start, inner end, bed as registered); under it pattern_id ascends.  B(h, q, key), the
 * value of distinct haplotype h for pattern id q, is the best record over q's strands: the
 * highest score, ties to the strand earlier in creation order, a strand with n_windows == 0
 * never; "none" when all its strands have n_windows == 0.  min_score plays no part.
 *
 * A candidate row (key, q): sample s with haplotypes a = memb[2s], b = memb[2s + 1] has
 * x_s = (int64)B(a) + (int64)B(b); a "none" value of a haplotype that some sample carries
 * means no row.  lo = min x, hi = max x, spread = hi - lo (up to 2^33 - 2).  No row when
 * n_samples == 0, spread == 0 or spread < min_spread (milli-log-odds).  With d = x_s - lo the
 * sample's field is
 *     d == 0             "\t0|0:0.0"      counts as zero
 *     d == spread        "\t1|1:2.0"      counts as two
 *     4 d < spread       "\t0|0:" DS      zero
 *     4 d < 3 spread     "\t0|1:" DS      one
 *     else               "\t1|1:" DS      two
 * DS = t / 10000 "." (t % 10000 on four digits), t = round_half_even(20000 d / spread) in
 * integers (no floating point anywhere): a field is 8 or 11 bytes.  maf is
 * counts_as_genotypes' rule (main.rs:482-489) on the three counts; the row is written iff
 * maf >= min_maf, as
 *   <chr>\t<POS>\t<bed>,<name>,<start>-<end>\t.\t.\t.\tPASS\tSCORES=<lo>,<hi>;freqs=<zero>/<one>/<two>\tGT:DS<fields>\n
 * (<chr> without any "chr", <name> tfbs_patterns_name_of, lo / hi signed decimal, POS a
 * counter of written rows as tfbs_batch_rows' *fake_position).
 *
 * Host only: the definition on one candidate row's per-sample values.  1 = row (info =
 * "SCORES=...;freqs=...", genotypes = the fields, both 0-terminated), 0 = no row;
 * TFBS_E_ARG when a buffer is too short. */
int tfbs_scores_as_genotypes(const int32_t *left, const int32_t *right, size_t n, uint64_t min_spread, uint32_t *maf,
                             char *info, size_t info_cap, char *genotypes, size_t gt_cap);
/* The score rows of regions [r0, r1) of the batch resident on ctx (after tfbs_batch_upload;
 * needs no scan; the batch made with keep_membership, else TFBS_E_STATE as for a batch that
 * is not resident; leaves every scan / reduce / encode / rows / hits / best result and the
 * step graph untouched).  *text is malloc'd (tfbs_free), *len its length, *n_rows its rows;
 * *fake_position is the first row's POS and is advanced per row.  text == NULL counts only:
 * *n_rows is set, *fake_position left untouched (it may be NULL).  The per-sample work runs
 * on the device (score_rows.hip): the best kernel's records are folded to values where they
 * lie, a row's statistics come from the region's distinct haplotype pairs, and the text
 * kernel writes the fields; the text equals tfbs_scores_as_genotypes' byte for byte.  Device
 * scratch (records, values, tokens, the text of some rows at a time) is bounded by
 * TFBS_SCORES_SCRATCH_MB (default 256, fractions allowed, read at the call; at least one
 * region's records and one row's text); the result does not depend on it. */
int tfbs_batch_score_rows(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome,
                          uint32_t min_maf, uint64_t min_spread, uint32_t *fake_position, char **text, size_t *len,
                          uint64_t *n_rows);
/* The last tfbs_batch_score_rows' times (ms): out[0] the best kernel, out[1] the fold and
 * statistics kernels, out[2] the text kernel (HIP events on the ctx stream, summed over the
 * scratch chunks), out[3] the copy-back and host part (wall). */
int tfbs_ctx_last_scores_ms(const tfbs_ctx *ctx, double out[4]);

/* ------------------------------------------------------------------ */
/* Affinity rows: per-sample log2 binding affinity as a second VCF      */
/* ------------------------------------------------------------------ */
/* The third measure of how a sample binds, added up over the sample: keys are the score rows'
 * (a (bed, non-empty inner range) pair, taken once, in the order inner start, inner end, bed;
 * under it pattern_id ascends).  The value of distinct haplotype h for pattern id q under a key
 * is the affinity TSV's: A(h) = the sum of `sum` over q's strands, N(h) = the sum of n_windows;
 * N == 0 is "none".  A candidate row (key, q) writes no row when a haplotype that a sample
 * carries is "none".  Otherwise sample s with haplotypes a = memb[2s], b = memb[2s + 1] has
 * x_s = A(a) + A(b) (u64; each term is below 2^63 by tfbs_batch_affinity's refusal) and
 *     y_s = mlog2(x_s),  mlog2(x) = floor(1000 * log2(x)) for x >= 1 (0 .. 63999),  mlog2(0) = -1
 * (the monotone extension: x = 0 with N > 0 is real, every window beyond the weight's cutoff).
 * lo = min y, hi = max y, spread = hi - lo (at most 64000).  No row when n_samples == 0,
 * spread == 0 or spread < min_spread (milli-bits; 0 counts as 1).  With d = y_s - lo the class,
 * t and the 8- or 11-byte field are the score rows'; maf is their rule on the three counts and
 * the row is written iff maf >= min_maf, as
 *   <chr>\t<POS>\t<bed>,<name>,<start>-<end>\t.\t.\t.\tPASS\tLOG2AFF=<lo>,<hi>;AFF=<xlo>,<xhi>;TOP=<top>;freqs=<zero>/<one>/<two>\tGT:DS<fields>\n
 * xlo / xhi the exact minimum and maximum of x in unsigned decimal (lo = mlog2(xlo), hi =
 * mlog2(xhi)), top tfbs_patterns_affinity_tops' value of q; <chr>, <name> and POS as in the score
 * rows.  Back to nats: ln(affinity_s) ~ top / 1000 + ln 2 * ((lo + DS / 2 * spread) / 1000 - 40).
 *
 * mlog2 is exact: with e = bitlen(x) - 1 and xn = x << (63 - e) it is 1000 e + max{j : P[j] <= xn}
 * over P[j] = ceil(2^63 * 2^(j / 1000)), 1 000 u64 written by tools/gen_affinity_tables.py with an
 * exact integer 1000th root.  out[i] = mlog2(x[i]); device -1 computes on the host, >= 0 with one
 * launch of the statistics kernel's own function on that HIP device. */
int tfbs_affinity_mlog2(const uint64_t *x, size_t n, int device, int32_t *out);
/* Host only: the definition on one candidate row's per-sample values (left[s], right[s] = A of
 * the sample's two haplotypes).  1 = row (info = "LOG2AFF=...;AFF=...;TOP=...;freqs=...",
 * genotypes = the fields, both 0-terminated), 0 = no row; TFBS_E_ARG when a value is 2^63 or
 * more or a buffer is too short. */
int tfbs_affinity_as_genotypes(const uint64_t *left, const uint64_t *right, size_t n, int32_t top, uint64_t min_spread,
                               uint32_t *maf, char *info, size_t info_cap, char *genotypes, size_t gt_cap);
/* The affinity rows of regions [r0, r1) of the batch resident on ctx: the arguments, the
 * count-only form (text == NULL) and the TFBS_E_STATE / TFBS_E_ARG cases are
 * tfbs_batch_score_rows'; a pattern set or a region that tfbs_batch_affinity refuses is refused
 * here with the same code and message.  Needs no scan; leaves every scan / reduce / encode /
 * rows / hits / best / affinity / scores / effects / mutscan result, their timers and the step
 * graph untouched.  The work runs on the device (affinity_rows.hip): the affinity kernel's
 * records are folded to (A, none) where they lie, a row's statistics and logarithms come from
 * the region's distinct haplotype pairs, and the score rows' text kernel writes the fields; the
 * text equals tfbs_affinity_as_genotypes' byte for byte.  Device scratch is bounded by
 * TFBS_AFFINITY_ROWS_SCRATCH_MB (default 256, fractions allowed, read at the call; at least one
 * region's records and one row's text); the result does not depend on it. */
int tfbs_batch_affinity_rows(tfbs_ctx *ctx, tfbs_batch *b, size_t r0, size_t r1, const char *chromosome,
                             uint32_t min_maf, uint64_t min_spread, uint32_t *fake_position, char **text, size_t *len,
                             uint64_t *n_rows);
/* The last tfbs_batch_affinity_rows' times (ms): out[0] the affinity kernel, out[1] the fold and
 * statistics kernels, out[2] the text kernel (HIP events on the ctx stream, summed over the
 * scratch chunks), out[3] the copy-back and host part (wall). */
int tfbs_ctx_last_affinity_rows_ms(const tfbs_ctx *ctx, double out[4]);

void tfbs_free(void *p);

/* counts_as_genotypes alone (main.rs:439-498): 1 = row (strings written), 0 = no variation. */
int tfbs_counts_as_genotypes(const uint32_t *left, const uint32_t *right, size_t n, uint32_t *maf, char *info,
                             size_t info_cap, char *genotypes, size_t gt_cap);

/* ------------------------------------------------------------------ */
/* The find-tfbs command flow (main.rs:163-393) and its file formats     */
/* (f2 BCF, f3 CLI + BGZF writer, f4 FASTA/BED)  */
/* ------------------------------------------------------------------ */
typedef struct tfbs_run_args {
    const char *chromosome;        /* --chromosome */
    const char *bcf;               /* --input */
    const char *bed_files;         /* --bed (comma list) */
    const char *reference;         /* --reference (FASTA with .fai) */
    const char *samples_file;      /* --samples, NULL = all BCF samples */
    const char *pwm_file;          /* --pwm_file */
    const char *pwm_threshold_dir; /* --pwm_threshold_directory */
    const char *pwm_names;         /* --pwm_names (comma list) */
    const char *output;            /* --output (BGZF VCF) */
    float pwm_threshold;           /* --pwm_threshold */
    int forward_only;              /* --forward_only */
    uint32_t min_maf;              /* --min_maf */
    uint32_t threads;              /* --threads: host threads building regions */
    uint64_t after_position;       /* --after_position */
    int tabix;                     /* --tabix */
    int verbose;                   /* --verbose */
    int device;                    /* HIP device (when devices is NULL/empty) */
    uint32_t regions_per_batch;    /* merged regions per GPU batch (0 = 512) */
    const char *devices;           /* comma list of HIP devices, one region shard each ("0,1,2,3";
                                      a device may repeat); NULL/"" = just `device` */
    const char *dipwm_file;        /* --dipwm_file: dinucleotide PWMs (tfbs_patterns_from_files_di), NULL = none;
                                      pwm_file may be NULL when it is set */
    const char *hits_output;       /* --hits_output: the batches' hit lists as BGZF TSV (tfbs_batch_hits_tsv under
                                      TFBS_HITS_HEADER), NULL = none: the run does nothing more than without it */
    int hits_mode;                 /* --hits_mode: TFBS_HITS_ALL / TFBS_HITS_DIFF */
    const char *best_output;       /* --best_output: the batches' best sites as BGZF TSV (tfbs_batch_best_tsv under
                                      TFBS_BEST_HEADER), NULL = none: the run does nothing more than without it */
    int best_mode;                 /* --best_mode: TFBS_BEST_ALL / TFBS_BEST_DIFF */
} tfbs_run_args;
/* Replaces run() (main.rs:234-393): writes <output>.part, renames it to output.
 * The merged regions go in batches of regions_per_batch (the reference's 50-peak
 * chunks over worker threads, main.rs:332-381); each batch is built (BCF records,
 * load_diffs; SNV-only regions grouped on the GPU), scanned, reduced, encoded and
 * its rows made as BGZF blocks on the device.  Several devices:
 * batch g runs on device g % n, each device with its own pipeline (BCF reader --
 * CSI-indexed seek when <bcf>.csi exists --, FASTA reader, host prep thread,
 * ctx); batch g's first POS is batch g - 1's plus its row count (published before
 * either deflates) and the batches' blocks are written in order, so the output
 * text is identical for any device list. */
int tfbs_run(const tfbs_run_args *args);
/* What later versions add to a run: tfbs_run_args keeps its layout, so a caller built
 * against an older header goes on working.  Only the first `size` bytes are read; a field
 * beyond them counts as 0 / NULL.  tfbs_run(args) is tfbs_run_ex(args, NULL). */
typedef struct tfbs_run_ext {
    uint32_t size;                  /* sizeof(tfbs_run_ext) of the caller */
    const char *effects_output;     /* --effects_output: the batches' variant effects as BGZF TSV
                                       (tfbs_batch_effects_tsv under TFBS_EFFECTS_HEADER), NULL = none: the run
                                       does nothing more than without it (its batches keep no variants, unless
                                       mutscan_output asks for them) */
    int effects_mode;               /* --effects_mode: TFBS_EFFECTS_SITES / TFBS_EFFECTS_ALL */
    const char *scores_output;      /* --scores_output: the batches' score rows (tfbs_batch_score_rows) as a second
                                       BGZF VCF under the main output's #CHROM line, POS from 1, min_maf as the
                                       main rows'; NULL = none: the run does nothing more than without it */
    uint64_t scores_min_spread;     /* --scores_min_spread: tfbs_batch_score_rows' min_spread (0 counts as 1) */
    double pwm_pvalue;              /* --pwm_pvalue: > 0: the patterns load by tfbs_patterns_from_files_pvalue on the
                                       run's first device; pwm_threshold_dir may then be NULL and pwm_threshold is
                                       ignored.  0: thresholds come from the directory as before */
    const char *mutscan_output;     /* --mutscan_output: the batches' mutation scans as BGZF TSV
                                       (tfbs_batch_mutscan_tsv under TFBS_MUTSCAN_HEADER), NULL = none: the run
                                       does nothing more than without it */
    uint32_t mutscan_kinds;         /* --mutscan_kinds: a mask of TFBS_MUT_*; 0 = TFBS_MUT_GAIN | TFBS_MUT_LOSS */
    const char *affinity_output;    /* --affinity_output: the batches' binding affinities as BGZF TSV
                                       (tfbs_batch_affinity_tsv under TFBS_AFFINITY_HEADER), NULL = none: the run
                                       does nothing more than without it */
    int affinity_mode;              /* --affinity_mode: TFBS_AFFINITY_ALL / TFBS_AFFINITY_DIFF */
    const char *affinity_rows_output;   /* --affinity_rows_output: the batches' affinity rows
                                           (tfbs_batch_affinity_rows) as a further BGZF VCF under the main output's
                                           #CHROM line, POS from 1 on a chain of its own, min_maf as the main rows';
                                           NULL = none: the run does nothing more than without it */
    uint64_t affinity_rows_min_spread;  /* --affinity_rows_min_spread: tfbs_batch_affinity_rows' min_spread
                                           (milli-bits; 0 counts as 1) */
} tfbs_run_ext;
int tfbs_run_ex(const tfbs_run_args *args, const tfbs_run_ext *ext);

typedef struct tfbs_bcf tfbs_bcf;
/* Replaces rust-htslib IndexedReader::from_path / header().samples() (main.rs:46-52, 255). */
int tfbs_bcf_open(const char *path, tfbs_bcf **out);
void tfbs_bcf_close(tfbs_bcf *b);
size_t tfbs_bcf_num_samples(const tfbs_bcf *b);
/* 1 if <path>.csi was loaded: fetches that would rewind or skip ahead seek to the
 * index's chunk start (IndexedReader::fetch, haplotype.rs:78-79); 0 = streaming sweep. */
int tfbs_bcf_indexed(const tfbs_bcf *b);
const char *tfbs_bcf_sample_name(const tfbs_bcf *b, size_t i);
/* Samples whose GT is decoded, in this order (default: all); main.rs:293-314's sample selection,
 * applied while decoding.  Rewinds the stream. */
int tfbs_bcf_select(tfbs_bcf *b, const size_t *idx, size_t n);
/* Replaces reader.fetch(rid, beg, end) (haplotype.rs:79): records with pos < end && pos + rlen > beg,
 * in file order.  Streams the file: queries with nondecreasing beg on one contig read it once,
 * an earlier beg or another contig rewinds to the start. */
int tfbs_bcf_fetch(tfbs_bcf *b, const char *chrom, uint64_t beg, uint64_t end, size_t *n_records);
/* Record i of the last fetch: raw GT ints, 2 per selected sample, INT32_MIN+1 = vector_end; alt NULL
 * for a single-allele record. */
int tfbs_bcf_record(const tfbs_bcf *b, size_t i, uint64_t *pos, uint32_t *rlen, uint32_t *n_alleles, const char **ref,
                    const char **alt, const int32_t **gt);
/* Carriers mode (on != 0; rewinds the stream): records keep load_diffs' carrier ids of a bi-allelic
 * record (haplotype.rs:16-41: 2 k iff GT[0] = Unphased(1), 2 k + 1 iff GT[1] = Phased(1), k the
 * selected sample), found on the reader's threads while decoding, instead of raw GT (tfbs_bcf_record
 * then returns gt NULL).  tfbs_run reads its BCF this way. */
int tfbs_bcf_set_carriers_mode(tfbs_bcf *b, int on);
/* The BCF reader's raw DEFLATE decoder (RFC 1951; BGZF blocks, htslib's bgzf.c
 * reads them with zlib): in_len bytes into exactly out_len bytes.  TFBS_OK, or
 * TFBS_E_PARSE for a stream it does not decode exactly (the reader then inflates
 * that block with zlib).  Exported for its tests. */
int tfbs_inflate_raw(const void *in, size_t in_len, void *out, size_t out_len);
/* Record i of the last fetch in carriers mode: ascending carrier ids and the ploidy check
 * (TFBS_OK, or TFBS_E_PLOIDY when a selected sample's GT does not hold 2 alleles,
 * haplotype.rs:24-26); 0 ids for a record that is not bi-allelic. */
int tfbs_bcf_record_carriers(const tfbs_bcf *b, size_t i, const uint32_t **ids, size_t *n, int *gt_status);
/* Replaces bio fasta IndexedReader fetch(chrom, start, stop) + read (main.rs:156-161). */
int tfbs_fasta_fetch(const char *fasta, const char *chrom, uint64_t start, uint64_t stop, char **out, size_t *n);
/* BGZF writer as BGzWriter (main.rs:267-276): data blocks, `flushes` empty blocks, EOF block. */
int tfbs_bgzf_write_file(const char *path, const char *text, size_t n, int flushes);
int tfbs_bgzf_read_file(const char *path, char **out, size_t *n);
/* RangeStack (range.rs:43-87): out arrays need n entries. */
int tfbs_merge_ranges(const uint64_t *starts, const uint64_t *ends, size_t n, uint64_t *out_s, uint64_t *out_e,
                      size_t *n_out);

/* ------------------------------------------------------------------ */
/* Synthetic workloads                            */
/* ------------------------------------------------------------------ */
/* Writes <dir>/pwms.txt and <dir>/thr/<name>.thr for n PWMs; lengths follow
 * config 2 (L = 8..15) or 3 (L = 8 + i%15, the last 30 L = 23 + i%8) or
 * 5 (L = 25..30).  names_csv (malloc'd) lists the names. */
int tfbs_synth_write_pwms(const char *dir, uint32_t n_pwms, int length_config, uint64_t seed, char **names_csv);
typedef struct tfbs_synth_region tfbs_synth_region;
/* Region `index` of a synthetic chromosome: BED row [1000+400*index, 1200+400*index],
 * Poisson(20) distinct variant sites over the ext window of max length lmax,
 * carriers with P(k) ~ 1/k on 1..H/10; indel_pct % of sites are 1-10 bp indels. */
int tfbs_synth_region_make(uint64_t seed, uint64_t index, uint32_t n_samples, uint32_t lmax, uint32_t indel_pct,
                           tfbs_synth_region **out);
void tfbs_synth_region_destroy(tfbs_synth_region *r);
void tfbs_synth_region_info(const tfbs_synth_region *r, uint64_t *merged_start, uint64_t *merged_end,
                            uint64_t *ext_start, const char **ref_ascii, size_t *n_ref, size_t *n_records);
void tfbs_synth_region_record(const tfbs_synth_region *r, size_t i, uint64_t *pos, const char **ref,
                              const char **alt, const uint32_t **carriers, size_t *n_carriers);
/* Adds regions [first, first+count) to b (one bed source "synthetic.bed" is
 * registered on first use; each region's inner peak is its BED row). */
int tfbs_synth_fill_batch(tfbs_batch *b, uint64_t seed, uint64_t first, uint64_t count, uint32_t indel_pct);

/* The resident batch's matrix-core window lists, per haplotype group (groups of
 * TFBS_MFMA_HAPS_PER_BLOCK haplotypes, in batch order): pairs[g] = the pairs of window
 * tiles (32 windows each, the last pair of an odd count holds one) of group g's list of
 * depth class cls (0: strands of up to 16 columns' tiles, 1: the longer ones') -- what the
 * scan's waves draw, one pair at a time.  *n_groups receives the group count; cap = 0 only
 * asks for it.  Waits for the stream.  Zeros for a class without tiles. */
int tfbs_ctx_group_pairs(tfbs_ctx *ctx, int cls, uint32_t *pairs, size_t cap, size_t *n_groups);

/* The resident batch's shared windows (debug API, as tfbs_ctx_group_pairs): entries[h] =
 * the sharer entries of haplotype h (batch order) as a donor in depth class cls -- what
 * the rescoring's expansion walks for each of h's hits.  *n_haps receives the haplotype
 * count; cap = 0 only asks for it.  Waits for the stream.  Zeros when nothing is shared
 * in the class (TFBS_SHARE=0, or no tile or no sharer of the class). */
int tfbs_ctx_share_entries(tfbs_ctx *ctx, int cls, uint32_t *entries, size_t cap, size_t *n_haps);

#ifdef __cplusplus
}
#endif
#endif /* TFBS_AMD_H */
