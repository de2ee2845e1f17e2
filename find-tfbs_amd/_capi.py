"""ctypes declarations for libtfbs_amd.so (include/tfbs_amd.h).

The library is built in-tree (``make`` or ``__graft_entry__.build()``) into
find-tfbs_amd/lib/.  Loading fails loudly if it is missing: there is no
Python or CPU fallback for the scan.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# TFBS_LIB overrides the in-tree build (e.g. a host-AddressSanitizer build of the same sources)
LIB_PATH = os.environ.get("TFBS_LIB") or os.path.join(HERE, "lib", "libtfbs_amd.so")

u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i32p = C.POINTER(C.c_int32)
vp = C.c_void_p


class tfbs_pattern_desc(C.Structure):
    _fields_ = [
        ("pattern_id", C.c_uint16),
        ("direction", C.c_uint8),
        ("kind", C.c_uint8),
        ("length", C.c_uint32),
        ("weights", i32p),
        ("min_score", C.c_int32),
        ("name", C.c_char_p),
    ]


class tfbs_plan_stats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_octet_strands", "n_quad_strands", "n_generic_strands",
                                           "n_fast_tiles", "n_fast_units", "n_generic_tiles",
                                           "max_tile_blocks")] + [("lut_bytes", C.c_uint64)] + \
        [(n, C.c_uint32) for n in ("n_mfma_strands", "n_mfma_tiles", "n_mfma_supers")]


class tfbs_mfma_bound(C.Structure):
    _fields_ = [("eligible", C.c_int32), ("q8", C.c_int64), ("t8", C.c_int64), ("scale", C.c_int64),
                ("c", C.c_int64)]


class tfbs_mfma_super(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("tile_count", "nk", "img_off", "img_bytes", "seg")] + \
        [("t0", C.c_int32)] + [(n, C.c_uint32) for n in ("acc0", "lmin", "lmax", "tile0")]


class tfbs_lut_tile(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("first", "last", "lut_begin", "nblocks", "slot_begin", "nslots", "lmin")]


class tfbs_lut_unit(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("lut_off", "nblk", "nstrand", "kind")] + [("init", C.c_uint32 * 4)] + \
        [("thr", C.c_int32 * 8), ("min_score", C.c_int32 * 8)] + \
        [(n, C.c_uint32 * 8) for n in ("len", "slot_local", "orig_index")]


class tfbs_lut_gen_pat(C.Structure):
    _fields_ = [("col_off", C.c_uint32), ("min_score", C.c_int32), ("len", C.c_uint32), ("slot_local", C.c_uint32),
                ("orig_index", C.c_uint32)]


class tfbs_lut_plan_sizes(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("n_tiles", "n_units", "lut_ints", "n_gen_tiles", "n_gen_pats",
                                          "gen_w_ints", "n_slots")]


class tfbs_lut_plan_buffers(C.Structure):
    _fields_ = [("tiles", C.POINTER(tfbs_lut_tile)), ("tiles_cap", C.c_size_t),
                ("units", C.POINTER(tfbs_lut_unit)), ("units_cap", C.c_size_t),
                ("lut", i32p), ("lut_cap", C.c_size_t),
                ("gen_tiles", C.POINTER(tfbs_lut_tile)), ("gen_tiles_cap", C.c_size_t),
                ("gen_pats", C.POINTER(tfbs_lut_gen_pat)), ("gen_pats_cap", C.c_size_t),
                ("gen_w", i32p), ("gen_w_cap", C.c_size_t),
                ("slot_pid", u16p), ("slot_pid_cap", C.c_size_t),
                ("slot_mfma", u8p), ("slot_mfma_cap", C.c_size_t)]


class tfbs_run_args(C.Structure):
    _fields_ = [
        ("chromosome", C.c_char_p), ("bcf", C.c_char_p), ("bed_files", C.c_char_p), ("reference", C.c_char_p),
        ("samples_file", C.c_char_p), ("pwm_file", C.c_char_p), ("pwm_threshold_dir", C.c_char_p),
        ("pwm_names", C.c_char_p), ("output", C.c_char_p), ("pwm_threshold", C.c_float), ("forward_only", C.c_int),
        ("min_maf", C.c_uint32), ("threads", C.c_uint32), ("after_position", C.c_uint64), ("tabix", C.c_int),
        ("verbose", C.c_int), ("device", C.c_int), ("regions_per_batch", C.c_uint32), ("devices", C.c_char_p),
        ("dipwm_file", C.c_char_p), ("hits_output", C.c_char_p), ("hits_mode", C.c_int),
        ("best_output", C.c_char_p), ("best_mode", C.c_int),
    ]


class tfbs_hit(C.Structure):
    _fields_ = [("region", C.c_uint32), ("haplotype", C.c_uint32), ("pattern", C.c_uint32), ("window", C.c_uint32),
                ("start", C.c_uint64), ("end", C.c_uint64), ("score", C.c_int32), ("reserved", C.c_uint32)]


class tfbs_best(C.Structure):
    _fields_ = [("region", C.c_uint32), ("haplotype", C.c_uint32), ("pattern", C.c_uint32), ("range", C.c_uint32),
                ("window", C.c_uint32), ("n_windows", C.c_uint32), ("score", C.c_int32), ("reserved", C.c_uint32),
                ("start", C.c_uint64), ("end", C.c_uint64)]


class tfbs_affinity(C.Structure):
    _fields_ = [("region", C.c_uint32), ("haplotype", C.c_uint32), ("pattern", C.c_uint32), ("range", C.c_uint32),
                ("n_windows", C.c_uint32), ("n_nonzero", C.c_uint32), ("sum", C.c_uint64)]


class tfbs_effect(C.Structure):
    _fields_ = [("region", C.c_uint32), ("variant", C.c_uint32), ("pattern", C.c_uint32), ("status", C.c_uint32),
                ("n_ref", C.c_uint32), ("ref_score", C.c_int32), ("ref_window", C.c_uint32),
                ("n_alt", C.c_uint32), ("alt_score", C.c_int32), ("alt_window", C.c_uint32),
                ("ref_start", C.c_uint64), ("ref_end", C.c_uint64), ("alt_start", C.c_uint64), ("alt_end", C.c_uint64)]


class tfbs_mutation(C.Structure):
    _fields_ = [("region", C.c_uint32), ("column", C.c_uint32), ("pattern", C.c_uint32), ("ref", C.c_uint8),
                ("alt", C.c_uint8), ("kind", C.c_uint8), ("reserved", C.c_uint8), ("pos", C.c_uint64),
                ("n_windows", C.c_uint32), ("ref_score", C.c_int32), ("ref_window", C.c_uint32),
                ("alt_score", C.c_int32), ("alt_window", C.c_uint32), ("reserved1", C.c_uint32),
                ("ref_start", C.c_uint64), ("ref_end", C.c_uint64), ("alt_start", C.c_uint64), ("alt_end", C.c_uint64)]


class tfbs_run_ext(C.Structure):
    _fields_ = [("size", C.c_uint32), ("effects_output", C.c_char_p), ("effects_mode", C.c_int)]


class tfbs_run_ext_scores(C.Structure):
    """tfbs_run_ext as the header has it since the score rows: the fields above, then the new ones
    at the end (tfbs_run_ex reads `size` bytes, so either layout is a valid argument)."""
    _fields_ = tfbs_run_ext._fields_ + [("scores_output", C.c_char_p), ("scores_min_spread", C.c_uint64)]


class tfbs_run_ext_pvalue(C.Structure):
    """tfbs_run_ext as the header has it since the p-value thresholds (pwm_pvalue at the end)."""
    _fields_ = tfbs_run_ext_scores._fields_ + [("pwm_pvalue", C.c_double)]


class tfbs_run_ext_mutscan(C.Structure):
    """tfbs_run_ext as the header has it since the mutation scan (its two fields at the end)."""
    _fields_ = tfbs_run_ext_pvalue._fields_ + [("mutscan_output", C.c_char_p), ("mutscan_kinds", C.c_uint32)]


class tfbs_run_ext_affinity(C.Structure):
    """tfbs_run_ext as the header has it since the binding affinity (its two fields at the end)."""
    _fields_ = tfbs_run_ext_mutscan._fields_ + [("affinity_output", C.c_char_p), ("affinity_mode", C.c_int)]


class tfbs_run_ext_affinity_rows(C.Structure):
    """tfbs_run_ext as the header has it since the affinity rows (their two fields at the end)."""
    _fields_ = tfbs_run_ext_affinity._fields_ + [("affinity_rows_output", C.c_char_p),
                                                 ("affinity_rows_min_spread", C.c_uint64)]


# (name, restype, argtypes) for every symbol in include/tfbs_amd.h
SIGNATURES = [
    ("tfbs_strerror", C.c_char_p, [C.c_int]),
    ("tfbs_last_error", C.c_char_p, []),
    ("tfbs_version", C.c_char_p, []),
    ("tfbs_patterns_create", C.c_int, [C.POINTER(tfbs_pattern_desc), C.c_size_t, C.POINTER(vp)]),
    ("tfbs_patterns_from_files", C.c_int, [C.c_char_p, C.c_char_p, C.c_float, C.c_char_p, C.c_int, C.POINTER(vp)]),
    ("tfbs_patterns_from_files_di", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_float, C.c_char_p, C.c_int,
                                              C.POINTER(vp)]),
    ("tfbs_patterns_count", C.c_size_t, [vp]),
    ("tfbs_patterns_get", C.c_int, [vp, C.c_size_t, C.POINTER(tfbs_pattern_desc)]),
    ("tfbs_patterns_name_of", C.c_char_p, [vp, C.c_uint16]),
    ("tfbs_patterns_max_length", C.c_uint32, [vp]),
    ("tfbs_patterns_destroy", None, [vp]),
    ("tfbs_patterns_plan_stats", C.c_int, [vp, C.c_uint32, C.c_int, C.POINTER(tfbs_plan_stats)]),
    ("tfbs_patterns_dinuc_stats", C.c_int, [vp, u32p, u32p, u64p]),
    ("tfbs_patterns_dinuc_lut_scores", C.c_int, [vp, C.c_size_t, u8p, C.c_size_t, i32p]),
    ("tfbs_patterns_mfma_bound", C.c_int, [vp, C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(tfbs_mfma_bound)]),
    ("tfbs_patterns_mfma_plan", C.c_int, [vp, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(tfbs_mfma_super), C.c_size_t, C.POINTER(C.c_size_t), i32p,
                                          C.c_size_t, C.POINTER(C.c_size_t)]),
    ("tfbs_patterns_lut_plan", C.c_int, [vp, C.c_uint32, C.c_int, C.POINTER(tfbs_lut_plan_buffers),
                                         C.POINTER(tfbs_lut_plan_sizes)]),
    ("tfbs_patterns_score_tails", C.c_int, [vp, C.c_int, C.c_size_t, i32p, C.c_size_t, u64p, u64p]),
    ("tfbs_patterns_pvalue_thresholds", C.c_int, [vp, C.c_int, C.c_double, i32p]),
    ("tfbs_patterns_with_min_scores", C.c_int, [vp, i32p, C.POINTER(vp)]),
    ("tfbs_patterns_from_files_pvalue", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double,
                                                  C.POINTER(vp)]),
    ("tfbs_pvalue_tile_widths", None, [u32p]),
    ("tfbs_parse_weight", C.c_int, [C.c_char_p, i32p]),
    ("tfbs_parse_threshold_file", C.c_int, [C.c_char_p, C.c_float, i32p]),
    ("tfbs_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("tfbs_ctx_create", C.c_int, [C.c_int, vp, C.POINTER(vp)]),
    ("tfbs_ctx_destroy", None, [vp]),
    ("tfbs_ctx_sync", C.c_int, [vp]),
    ("tfbs_ctx_set_host_threads", C.c_int, [vp, C.c_uint32]),
    ("tfbs_ctx_last_scan_ms", C.c_float, [vp]),
    ("tfbs_ctx_last_scan_launches", C.c_int, [vp]),
    ("tfbs_ctx_last_mfma_ms", C.c_float, [vp]),
    ("tfbs_ctx_window_lists", C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("tfbs_ctx_scan_counters", C.c_int, [vp, C.POINTER(C.c_uint64)]),
    ("tfbs_matches", C.c_int, [vp, u8p, u64p, C.c_size_t, u32p, u64p, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("tfbs_patch_haplotype", C.c_int, [C.c_uint64, C.c_uint64, C.c_size_t, u64p, u8p, u32p, u8p, u32p, u8p, u64p,
                                       C.c_size_t, u8p, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("tfbs_batch_create", C.c_int, [vp, C.c_uint32, C.c_int, C.POINTER(vp)]),
    ("tfbs_batch_destroy", None, [vp]),
    ("tfbs_batch_add_bed", C.c_int, [vp, C.c_char_p]),
    ("tfbs_batch_set_window_lmax", C.c_int, [vp, C.c_uint32]),
    ("tfbs_batch_set_build_device", C.c_int, [vp, C.c_int]),
    ("tfbs_batch_hold", C.c_int, [vp, C.c_int]),
    ("tfbs_batch_group_calls", C.c_int, [vp, u64p]),
    ("tfbs_batch_build_stats", C.c_int, [vp, u64p, u64p]),
    ("tfbs_grouper_create", C.c_int, [C.c_int, C.POINTER(vp)]),
    ("tfbs_grouper_destroy", None, [vp]),
    ("tfbs_grouper_group", C.c_int, [vp, C.c_uint32, C.c_size_t, u32p, u32p, u32p, u32p, u64p, u32p, C.c_size_t,
                                     C.POINTER(C.c_size_t), u16p]),
    ("tfbs_batch_patch_stats", C.c_int, [vp, u64p]),
    ("tfbs_batch_region_ext", C.c_int, [vp, C.c_uint64, C.c_uint64, u64p, u64p]),
    ("tfbs_batch_region_begin", C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("tfbs_batch_region_add_inner", C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_uint64]),
    ("tfbs_batch_region_add_record_gt", C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_char_p, C.c_char_p, i32p]),
    ("tfbs_batch_region_add_record_carriers", C.c_int, [vp, C.c_uint64, C.c_char_p, C.c_char_p, u32p, C.c_size_t]),
    ("tfbs_batch_region_end", C.c_int, [vp]),
    ("tfbs_batch_num_regions", C.c_size_t, [vp]),
    ("tfbs_batch_num_haplotypes", C.c_size_t, [vp]),
    ("tfbs_batch_num_windows", C.c_uint64, [vp]),
    ("tfbs_batch_num_effective_windows", C.c_uint64, [vp]),
    ("tfbs_batch_num_cell_ops", C.c_uint64, [vp]),
    ("tfbs_batch_num_scan_windows", C.c_uint64, [vp]),
    ("tfbs_batch_num_scan_cell_ops", C.c_uint64, [vp]),
    ("tfbs_batch_input_bytes", C.c_uint64, [vp]),
    ("tfbs_batch_output_bytes", C.c_uint64, [vp]),
    ("tfbs_batch_upload", C.c_int, [vp, vp]),
    ("tfbs_scan", C.c_int, [vp, vp]),
    ("tfbs_batch_download", C.c_int, [vp, vp]),
    ("tfbs_batch_reduce", C.c_int, [vp, vp]),
    ("tfbs_batch_assemble", C.c_int, [vp, vp]),
    ("tfbs_batch_assemble_wait", C.c_int, [vp, vp]),
    ("tfbs_step", C.c_int, [vp, vp]),
    ("tfbs_ctx_last_assemble_ms", C.c_float, [vp]),
    ("tfbs_ctx_assembly_trace", C.c_int, [vp, C.c_int]),
    ("tfbs_batch_assembly_paths", C.c_int, [vp, vp, u32p, C.c_uint32]),
    ("tfbs_ctx_region_asm", C.c_int, [vp, u32p, C.c_size_t, u32p, C.c_size_t, C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_size_t)]),
    ("tfbs_ctx_assembly_figures", C.c_int, [vp, u64p]),
    ("tfbs_ctx_post_figures", C.c_int, [vp, u64p]),
    ("tfbs_batch_region_layout", C.c_int, [vp, C.c_size_t, u32p]),
    ("tfbs_batch_region_hap_runs", C.c_int, [vp, C.c_size_t, C.c_uint32, C.POINTER(C.c_int), u32p, u32p, u32p,
                                            C.c_uint32]),
    ("tfbs_batch_region_hap_own_runs", C.c_int, [vp, C.c_size_t, C.c_uint32, C.POINTER(C.c_int), u32p, u32p, u32p,
                                                C.c_uint32]),
    ("tfbs_batch_encode",C.c_int, [vp, vp, C.c_size_t, C.c_size_t]),
    ("tfbs_batch_encode_flags", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_int]),
    ("tfbs_batch_encode_stats", C.c_int, [vp, u64p]),
    ("tfbs_ctx_rows_bgzf_seconds", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_ctx_rows_bgzf_blocks", C.c_int, [vp, u64p]),
    ("tfbs_batch_rows_bgzf", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint32, u32p, C.c_int,
                                       u64p, u64p, u64p]),
    ("tfbs_batch_region_num_keys", C.c_int, [vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("tfbs_batch_region_key", C.c_int, [vp, C.c_size_t, C.c_size_t, u32p, u64p, u64p, u16p, u32p, u32p]),
    ("tfbs_batch_rows", C.c_int, [vp, C.c_char_p, C.c_uint32, u32p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("tfbs_batch_region_rows", C.c_int, [vp, C.c_size_t, C.c_char_p, C.c_uint32, u32p, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_size_t)]),
    ("tfbs_batch_region_digest", C.c_int, [vp, C.c_size_t, u64p]),
    ("tfbs_batch_region_key_digest_sum", C.c_int, [vp, C.c_size_t, u64p]),
    ("tfbs_batch_region_input_digest", C.c_int, [vp, C.c_size_t, u64p]),
    ("tfbs_batch_region_digests", C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, u64p, u64p, u64p]),
    ("tfbs_batch_region_stats", C.c_int, [vp, C.c_size_t, u32p, u32p]),
    ("tfbs_batch_format_rows", C.c_int, [vp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, u64p,
                                         u64p]),
    ("tfbs_batch_prep_seconds", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_batch_hits", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("tfbs_batch_hits_count", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, u64p]),
    ("tfbs_ctx_last_hits_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_batch_region_haplotype", C.c_int, [vp, C.c_size_t, C.c_uint32, u8p, u64p, C.c_size_t,
                                              C.POINTER(C.c_size_t), u32p]),
    ("tfbs_batch_region_membership", C.c_int, [vp, C.c_size_t, u32p]),
    ("tfbs_batch_hits_tsv", C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int, C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_size_t)]),
    ("tfbs_batch_best", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("tfbs_batch_region_num_ranges", C.c_int, [vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("tfbs_batch_region_range", C.c_int, [vp, C.c_size_t, C.c_size_t, u64p, u64p]),
    ("tfbs_ctx_last_best_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_batch_best_tsv", C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int, C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_size_t)]),
    ("tfbs_affinity_weight", C.c_uint64, [C.c_uint64]),
    ("tfbs_patterns_affinity_tops", C.c_int, [vp, i32p]),
    ("tfbs_batch_affinity", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("tfbs_ctx_last_affinity_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_batch_affinity_tsv", C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_size_t)]),
    ("tfbs_batch_keep_variants", C.c_int, [vp, C.c_int]),
    ("tfbs_batch_region_variant", C.c_int, [vp, C.c_size_t, C.c_size_t, u64p, u8p, u8p, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), u32p, u32p, u32p]),
    ("tfbs_batch_effects", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("tfbs_ctx_last_effects_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_batch_effects_tsv", C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_size_t)]),
    ("tfbs_batch_mutscan", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_size_t)]),
    ("tfbs_batch_mutscan_count", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_uint32, u64p]),
    ("tfbs_mutscan_ring_max_length", C.c_uint32, []),
    ("tfbs_ctx_last_mutscan_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_batch_mutscan_tsv", C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_size_t)]),
    ("tfbs_scores_as_genotypes", C.c_int, [i32p, i32p, C.c_size_t, C.c_uint64, u32p, C.c_char_p, C.c_size_t,
                                           C.c_char_p, C.c_size_t]),
    ("tfbs_batch_score_rows", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint64, u32p,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), u64p]),
    ("tfbs_ctx_last_scores_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_affinity_mlog2", C.c_int, [u64p, C.c_size_t, C.c_int, i32p]),
    ("tfbs_affinity_as_genotypes", C.c_int, [u64p, u64p, C.c_size_t, C.c_int32, C.c_uint64, u32p, C.c_char_p,
                                             C.c_size_t, C.c_char_p, C.c_size_t]),
    ("tfbs_batch_affinity_rows", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint64, u32p,
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), u64p]),
    ("tfbs_ctx_last_affinity_rows_ms", C.c_int, [vp, C.POINTER(C.c_double)]),
    ("tfbs_free", None, [C.c_void_p]),
    ("tfbs_counts_as_genotypes", C.c_int, [u32p, u32p, C.c_size_t, u32p, C.c_char_p, C.c_size_t, C.c_char_p,
                                           C.c_size_t]),
    ("tfbs_run", C.c_int, [C.c_void_p]),
    ("tfbs_run_ex", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tfbs_bcf_open", C.c_int, [C.c_char_p, C.POINTER(vp)]),
    ("tfbs_inflate_raw", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    ("tfbs_bcf_close", None, [vp]),
    ("tfbs_bcf_select", C.c_int, [vp, C.POINTER(C.c_size_t), C.c_size_t]),
    ("tfbs_bcf_num_samples", C.c_size_t, [vp]),
    ("tfbs_bcf_indexed", C.c_int, [vp]),
    ("tfbs_bcf_sample_name", C.c_char_p, [vp, C.c_size_t]),
    ("tfbs_bcf_fetch", C.c_int, [vp, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_size_t)]),
    ("tfbs_bcf_set_carriers_mode", C.c_int, [vp, C.c_int]),
    ("tfbs_bcf_record_carriers", C.c_int, [vp, C.c_size_t, C.POINTER(u32p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("tfbs_bcf_record", C.c_int, [vp, C.c_size_t, u64p, u32p, u32p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                  C.POINTER(i32p)]),
    ("tfbs_fasta_fetch", C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_size_t)]),
    ("tfbs_bgzf_write_file", C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.c_int]),
    ("tfbs_bgzf_read_file", C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("tfbs_merge_ranges", C.c_int, [u64p, u64p, C.c_size_t, u64p, u64p, C.POINTER(C.c_size_t)]),
    ("tfbs_synth_write_pwms", C.c_int, [C.c_char_p, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("tfbs_synth_region_make", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(vp)]),
    ("tfbs_synth_region_destroy", None, [vp]),
    ("tfbs_synth_region_info", None, [vp, u64p, u64p, u64p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t)]),
    ("tfbs_synth_region_record", None, [vp, C.c_size_t, u64p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                        C.POINTER(u32p), C.POINTER(C.c_size_t)]),
    ("tfbs_synth_fill_batch", C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]),
    ("tfbs_ctx_group_pairs", C.c_int, [vp, C.c_int, u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("tfbs_ctx_share_entries", C.c_int, [vp, C.c_int, u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
]

_lib = None


class TfbsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (msg, code, _lib.tfbs_strerror(code).decode() if _lib else "?"))
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("find-tfbs_amd native library missing at %s: run `make` or "
                              "`python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc < 0:
        raise TfbsError(rc, lib().tfbs_last_error().decode(errors="replace"))
    return rc
