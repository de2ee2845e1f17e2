"""find-tfbs_amd: MI355X-native drop-in for find-tfbs's per-haplotype TFBS scoring path.

This module mirrors the reference's Rust interface for that path (names,
argument meaning, error behaviour) over the C ABI of include/tfbs_amd.h:

  reference (find-tfbs v1.0.1)                    here
  ----------------------------------------------  ---------------------------------
  pattern.rs:13-16   parse_weight                 parse_weight
  pattern.rs:18-35   parse_threshold_file         parse_threshold_file
  pattern.rs:37-87   parse_pwm_files              parse_pwm_files -> PatternSet
  pattern.rs:141-171 matches                      matches / Scanner.matches (GPU)
  haplotype.rs:94    patch_haplotype              patch_haplotype
  haplotype.rs:77    load_haplotypes  \
  main.rs:94         find_all_matches  >          RegionBatch (+ Scanner.scan, GPU)
  main.rs:500        count_matches_by_sample /    RegionBatch.keys
  main.rs:439        counts_as_genotypes          counts_as_genotypes
  main.rs:415-429    row emission                 RegionBatch.rows

The reference panics where TfbsError is raised.  The scan always runs on a HIP
device; without one, Scanner() raises TfbsError(TFBS_E_NODEVICE).
"""
import array
import contextlib
import ctypes as C
from collections import namedtuple

from . import _capi
from ._capi import TfbsError, check, lib, tfbs_pattern_desc  # noqa: F401

TFBS_OK = 0
TFBS_E_NODEVICE = -10
KIND_PWM, KIND_OTHER, KIND_DIPWM = 0, 1, 2
DIR_P, DIR_N = 0, 1
NUCLEOTIDES = "ACGTN"  # types.rs:5-8, the weight index order

# tfbs_hit as a numpy dtype (RegionBatch.hits), the hit list TSV's modes and header line
HIT_DTYPE = [("region", "<u4"), ("haplotype", "<u4"), ("pattern", "<u4"), ("window", "<u4"), ("start", "<u8"),
             ("end", "<u8"), ("score", "<i4"), ("reserved", "<u4")]
HITS_MODES = {"all": 0, "diff": 1}
HITS_HEADER = "#chrom\tregion\thaplotype\tcarriers\tkind\tname\tpattern_id\tstrand\tstart\tend\tscore\tcarrier_ids\n"
# tfbs_best as a numpy dtype (RegionBatch.best), the best-site TSV's modes and header line
BEST_DTYPE = [("region", "<u4"), ("haplotype", "<u4"), ("pattern", "<u4"), ("range", "<u4"), ("window", "<u4"),
              ("n_windows", "<u4"), ("score", "<i4"), ("reserved", "<u4"), ("start", "<u8"), ("end", "<u8")]
BEST_MODES = {"all": 0, "diff": 1}
BEST_HEADER = ("#chrom\tregion\tbed\tinner_start\tinner_end\tname\tpattern_id\thaplotype\tcarriers\tkind\tstrand\t"
               "start\tend\tscore\tdelta\tcarrier_ids\n")
# tfbs_affinity as a numpy dtype (RegionBatch.affinity), the affinity TSV's modes and header line
AFFINITY_DTYPE = [("region", "<u4"), ("haplotype", "<u4"), ("pattern", "<u4"), ("range", "<u4"), ("n_windows", "<u4"),
                  ("n_nonzero", "<u4"), ("sum", "<u8")]
AFFINITY_MODES = {"all": 0, "diff": 1}
AFFINITY_HEADER = ("#chrom\tregion\tbed\tinner_start\tinner_end\tname\tpattern_id\thaplotype\tcarriers\tkind\ttop\t"
                   "n_windows\taffinity\tdelta\tcarrier_ids\n")
# tfbs_effect as a numpy dtype (RegionBatch.effects), a record's statuses, the effect TSV's modes and header line
EFFECT_DTYPE = [("region", "<u4"), ("variant", "<u4"), ("pattern", "<u4"), ("status", "<u4"), ("n_ref", "<u4"),
                ("ref_score", "<i4"), ("ref_window", "<u4"), ("n_alt", "<u4"), ("alt_score", "<i4"),
                ("alt_window", "<u4"), ("ref_start", "<u8"), ("ref_end", "<u8"), ("alt_start", "<u8"),
                ("alt_end", "<u8")]
VAR_SCORED, VAR_MULTIALLELIC, VAR_NO_CARRIER, VAR_UNPATCHED = 0, 1, 2, 3
EFFECT_MODES = {"sites": 0, "all": 1}
EFFECTS_HEADER = ("#chrom\tregion\tvariant\tpos\tref\talt\tcarriers\tkind\tname\tpattern_id\tstrand\tref_start\t"
                  "ref_end\tref_score\talt_start\talt_end\talt_score\tdelta\n")
# tfbs_mutation as a numpy dtype (RegionBatch.mutscan), the kinds' mask bits and codes, the TSV's header line
MUTATION_DTYPE = [("region", "<u4"), ("column", "<u4"), ("pattern", "<u4"), ("ref", "u1"), ("alt", "u1"), ("kind", "u1"),
                  ("reserved", "u1"), ("pos", "<u8"), ("n_windows", "<u4"), ("ref_score", "<i4"), ("ref_window", "<u4"),
                  ("alt_score", "<i4"), ("alt_window", "<u4"), ("reserved1", "<u4"), ("ref_start", "<u8"),
                  ("ref_end", "<u8"), ("alt_start", "<u8"), ("alt_end", "<u8")]
MUT_GAIN, MUT_LOSS, MUT_CHANGE, MUT_SAME, MUT_NONE = 1, 2, 4, 8, 16
MUT_SITES, MUT_ALL = 7, 31
MUT_KINDS = ("gain", "loss", "change", "same", "none")  # a record's kind code indexes it; bit 1 << code in a mask
MUTSCAN_HEADER = ("#chrom\tregion\tpos\tref\talt\tkind\tname\tpattern_id\tstrand\tref_start\tref_end\tref_score\t"
                  "alt_start\talt_end\talt_score\tdelta\n")

Range = namedtuple("Range", "start end")  # range.rs:4-8, inclusive
NucleotidePos = namedtuple("NucleotidePos", "nuc pos")  # types.rs:23-27 (nuc as 'A'..'N')
Diff = namedtuple("Diff", "pos reference alternative")  # types.rs:39-44 (strings)
HaplotypeId = namedtuple("HaplotypeId", "sample_id side")  # types.rs:66-70, side 0 Left / 1 Right
Match = namedtuple("Match", "range pattern_id haplotype_ids")  # types.rs:32-37


class Weight:
    """types.rs:103-114: four milli-log-odds weights, N forced to 0."""

    __slots__ = ("acgtn",)

    def __init__(self, a, c, g, t):
        self.acgtn = [a, c, g, t, 0]

    def __eq__(self, o):
        return isinstance(o, Weight) and self.acgtn == o.acgtn

    def __repr__(self):
        return "Weight(%r)" % (self.acgtn,)


class Pattern:
    """types.rs:86-90: PWM (kind 0) or OtherPattern (kind 1); DiPWM (kind 2) is a
    dinucleotide PWM: weights = L - 1 rows of 16 ints indexed 4 a + b for the pair
    (base a, next base b), len() = L bases."""

    def __init__(self, name, pattern_id, weights=None, min_score=0, direction=DIR_P, kind=KIND_PWM):
        self.name = name
        self.pattern_id = pattern_id
        self.weights = list(weights or [])
        self.min_score = min_score
        self.direction = direction
        self.kind = kind

    @classmethod
    def PWM(cls, weights, name, pattern_id, min_score, direction=DIR_P):
        return cls(name, pattern_id, weights, min_score, direction, KIND_PWM)

    @classmethod
    def OtherPattern(cls, name, pattern_id):
        return cls(name, pattern_id, [], 0, DIR_P, KIND_OTHER)

    @classmethod
    def DiPWM(cls, rows16, name, pattern_id, min_score, direction=DIR_P):
        return cls(name, pattern_id, [list(r) for r in rows16], min_score, direction, KIND_DIPWM)

    def __len__(self):  # pattern_length (types.rs:92-101); a dinucleotide PWM counts bases
        if self.kind == KIND_DIPWM:
            return len(self.weights) + 1
        return len(self.weights) if self.kind == KIND_PWM else 0

    def __eq__(self, o):
        return (isinstance(o, Pattern) and (self.name, self.pattern_id, self.weights, self.min_score,
                                             self.direction, self.kind) ==
                (o.name, o.pattern_id, o.weights, o.min_score, o.direction, o.kind))

    def __repr__(self):
        return "Pattern(%s id=%d L=%d min=%d dir=%s)" % (self.name, self.pattern_id, len(self), self.min_score,
                                                         "+-"[self.direction])


def _u(x):
    return x.encode() if isinstance(x, str) else x


def parse_weight(s):
    v = C.c_int32()
    check(lib().tfbs_parse_weight(_u(s), C.byref(v)))
    return v.value


def parse_threshold_file(filename, pwm_threshold):
    v = C.c_int32()
    r = check(lib().tfbs_parse_threshold_file(_u(filename), pwm_threshold, C.byref(v)))
    return v.value if r == 1 else None


class PatternSet:
    """An immutable tfbs_patterns handle (Vec<Pattern> of the reference)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_patterns(cls, patterns):
        n = len(patterns)
        descs = (tfbs_pattern_desc * max(1, n))()
        keep = []
        for i, p in enumerate(patterns):
            if p.kind == KIND_DIPWM:
                if any(len(r) != 16 for r in p.weights):
                    raise ValueError("a dinucleotide PWM row has 16 weights")
                flat = [x for r in p.weights for x in r]
            else:
                flat = [x for w in p.weights for x in (w.acgtn if isinstance(w, Weight) else list(w)[:4] + [0])]
            arr = (C.c_int32 * max(1, len(flat)))(*flat)
            name = _u(p.name)
            keep.append((arr, name))
            descs[i] = tfbs_pattern_desc(p.pattern_id, p.direction, p.kind, len(p), arr, p.min_score, name)
        h = C.c_void_p()
        check(lib().tfbs_patterns_create(descs, n, C.byref(h)))
        return cls(h)

    def __del__(self):
        if getattr(self, "h", None):
            lib().tfbs_patterns_destroy(self.h)
            self.h = None

    def __len__(self):
        return lib().tfbs_patterns_count(self.h)

    def __getitem__(self, i):
        d = tfbs_pattern_desc()
        check(lib().tfbs_patterns_get(self.h, i, C.byref(d)))
        if d.kind == KIND_DIPWM:
            ws = [[d.weights[16 * j + c] for c in range(16)] for j in range(d.length - 1)]
        else:
            ws = [Weight(*(d.weights[5 * j + c] for c in range(4))) for j in range(d.length)]
        return Pattern(d.name.decode(), d.pattern_id, ws, d.min_score, d.direction, d.kind)

    def to_list(self):
        return [self[i] for i in range(len(self))]

    def name_of(self, pattern_id):
        s = lib().tfbs_patterns_name_of(self.h, pattern_id)
        return s.decode() if s is not None else None

    @property
    def max_length(self):
        return lib().tfbs_patterns_max_length(self.h)

    def mfma_bound(self, i, window):
        """The matrix-core bound of pattern i on one window ("ACGTN" string of the pattern's
        length): dict(eligible, q8, t8, scale, c); bound = c + scale * q8 / 8, candidate iff q8 > t8."""
        codes = (C.c_uint8 * max(1, len(window)))(*["ACGTN".index(ch) for ch in window])
        out = _capi.tfbs_mfma_bound()
        check(lib().tfbs_patterns_mfma_bound(self.h, i, codes, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def mfma_plan(self, lds_kb=0):
        """The matrix-core plan a Scanner uploads with TFBS_MFMA_LDS_KB=lds_kb (0: the default),
        copied and not interpreted (tfbs_patterns_mfma_plan, a diagnostic): dict(image = the
        super tiles' FP6 digit fragments as bytes, supers = [dict of tfbs_mfma_super's fields],
        meta = the tiles' rescoring fields, 384 ints per tile)."""
        nb, ns, nm = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib().tfbs_patterns_mfma_plan(self.h, lds_kb, None, 0, C.byref(nb), None, 0, C.byref(ns), None, 0,
                                            C.byref(nm)))
        img = (C.c_uint8 * max(1, nb.value))()
        sup = (_capi.tfbs_mfma_super * max(1, ns.value))()
        meta = (C.c_int32 * max(1, nm.value))()
        check(lib().tfbs_patterns_mfma_plan(self.h, lds_kb, img, nb.value, C.byref(nb), sup, ns.value, C.byref(ns),
                                            meta, nm.value, C.byref(nm)))
        return {"image": bytes(img)[:nb.value], "meta": list(meta[:nm.value]),
                "supers": [{n: getattr(sup[k], n) for n, _ in sup[k]._fields_} for k in range(ns.value)]}

    def lut_plan(self, tile_blocks=20, mfma=False):
        """The LUT and generic plan a Scanner uploads with TFBS_TILE_BLOCKS=tile_blocks and
        TFBS_MFMA=mfma, copied and not interpreted (tfbs_patterns_lut_plan, a diagnostic): dict(tiles,
        units, gen_tiles, gen_pats = [dict of the entry's fields, a unit's per-strand fields as
        lists], lut = the table blocks' ints (1024 per block) and gen_w = the generic weights (5 per
        column) as array('i'), slot_pid, slot_mfma = lists, one entry per count slot)."""
        sz = _capi.tfbs_lut_plan_sizes()
        check(lib().tfbs_patterns_lut_plan(self.h, tile_blocks, 1 if mfma else 0, None, C.byref(sz)))
        buf = _capi.tfbs_lut_plan_buffers()
        keep = {}
        for name, n, ctype in (("tiles", sz.n_tiles, _capi.tfbs_lut_tile), ("units", sz.n_units, _capi.tfbs_lut_unit),
                               ("lut", sz.lut_ints, C.c_int32), ("gen_tiles", sz.n_gen_tiles, _capi.tfbs_lut_tile),
                               ("gen_pats", sz.n_gen_pats, _capi.tfbs_lut_gen_pat), ("gen_w", sz.gen_w_ints, C.c_int32),
                               ("slot_pid", sz.n_slots, C.c_uint16), ("slot_mfma", sz.n_slots, C.c_uint8)):
            keep[name] = (ctype * max(1, n))()
            setattr(buf, name, keep[name])
            setattr(buf, name + "_cap", n)
        check(lib().tfbs_patterns_lut_plan(self.h, tile_blocks, 1 if mfma else 0, C.byref(buf), C.byref(sz)))

        def fields(x):
            return {n: (getattr(x, n) if isinstance(getattr(x, n), int) else list(getattr(x, n))) for n, _ in x._fields_}

        def ints(name, n):
            a = array.array("i")
            a.frombytes(bytes(keep[name])[:4 * n])
            return a

        assert array.array("i").itemsize == 4
        return {"tiles": [fields(keep["tiles"][k]) for k in range(sz.n_tiles)],
                "units": [fields(keep["units"][k]) for k in range(sz.n_units)],
                "gen_tiles": [fields(keep["gen_tiles"][k]) for k in range(sz.n_gen_tiles)],
                "gen_pats": [fields(keep["gen_pats"][k]) for k in range(sz.n_gen_pats)],
                "lut": ints("lut", sz.lut_ints), "gen_w": ints("gen_w", sz.gen_w_ints),
                "slot_pid": list(keep["slot_pid"][:sz.n_slots]), "slot_mfma": list(keep["slot_mfma"][:sz.n_slots])}

    def subset(self, keep_pattern_id):
        """A new PatternSet of the patterns whose pattern_id passes keep_pattern_id (both
        strands of a PWM share an id, so they stay together): a pattern shard of SURVEY.md
        8(e)'s region x PWM split.  Batches scanning it pass the whole set's max_length to
        RegionBatch(window_lmax=...) so their windows are the unsharded run's."""
        return PatternSet.from_patterns([p for p in self.to_list() if keep_pattern_id(p.pattern_id)])

    def plan_stats(self, tile_blocks=20, mfma=False):
        """Host-side summary of the device plan (octet/quad/generic/MFMA strands, tiles)."""
        st = _capi.tfbs_plan_stats()
        check(lib().tfbs_patterns_plan_stats(self.h, tile_blocks, 1 if mfma else 0, C.byref(st)))
        return {n: getattr(st, n) for n, _ in st._fields_}


    def dinuc_stats(self):
        """The dinucleotide part of the device plan: dict(n_strands, n_tiles, lut_bytes)."""
        ns, nt, nb = C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().tfbs_patterns_dinuc_stats(self.h, C.byref(ns), C.byref(nt), C.byref(nb)))
        return {"n_strands": ns.value, "n_tiles": nt.value, "lut_bytes": nb.value}

    def dinuc_lut_scores(self, i, windows):
        """The scores the dinucleotide kernel's lookup loop gives pattern i on `windows`,
        evaluated on the host from the plan's lookup tables (tfbs_patterns_dinuc_lut_scores).
        A window is 32 base codes 0-3: the window's bases, then whatever follows them."""
        n = len(windows)
        if any(len(w) != 32 for w in windows):
            raise ValueError("a dinucleotide window image has 32 base codes")
        flat = (C.c_uint8 * max(1, 32 * n))(*[c for w in windows for c in w])
        out = (C.c_int32 * max(1, n))()
        check(lib().tfbs_patterns_dinuc_lut_scores(self.h, i, flat, n, out))
        return list(out[:n])


    def score_tails(self, i, scores, device=0):
        """Exact tail(m) = #{x in {A,C,G,T}^L : score(x) >= m} of strand i for every m in scores, as
        Python ints; the p-value of "score >= m" is tail / 4 ** len(strand).  device: the HIP device
        that computes the table, -1: the host twin."""
        n = len(scores)
        sc = (C.c_int32 * max(1, n))(*scores)
        lo = (C.c_uint64 * max(1, n))()
        hi = (C.c_uint64 * max(1, n))()
        check(lib().tfbs_patterns_score_tails(self.h, device, i, sc, n, lo, hi))
        return [(hi[k] << 64) | lo[k] for k in range(n)]

    def pvalue_thresholds(self, p, device=0):
        """One min_score per strand in creation order for the p-value p (0 <= p < 1):
        max{m : tail(m) > floor(p * 4 ** L)}; an OtherPattern keeps its own."""
        n = len(self)
        out = (C.c_int32 * max(1, n))()
        check(lib().tfbs_patterns_pvalue_thresholds(self.h, device, p, out))
        return list(out[:n])

    def affinity_tops(self):
        """tfbs_patterns_affinity_tops: one value per strand in creation order, its pattern_id's
        reference score top (the highest sum any strand of the id can reach, an N adding 0), 0 for
        an OtherPattern; TfbsError (TFBS_E_ARG) when a strand's sums can wrap int32."""
        n = len(self)
        out = (C.c_int32 * max(1, n))()
        check(lib().tfbs_patterns_affinity_tops(self.h, out))
        return list(out[:n])

    def with_min_scores(self, ms):
        """A copy whose strand k has min_score ms[k]; ids, names, order and weights stay."""
        if len(ms) != len(self):
            raise ValueError("one min_score per strand")
        arr = (C.c_int32 * max(1, len(ms)))(*ms)
        h = C.c_void_p()
        check(lib().tfbs_patterns_with_min_scores(self.h, arr, C.byref(h)))
        return PatternSet(h)


def affinity_weight(d):
    """tfbs_affinity_weight: a(d) = floor(2^40 * exp(-d / 1000)) for an integer 0 <= d < 2^64."""
    return lib().tfbs_affinity_weight(d)


def pvalue_tile_widths():
    """The bins one workgroup takes in a gather step and in the suffix sum of the device path."""
    out = (C.c_uint32 * 2)()
    lib().tfbs_pvalue_tile_widths(out)
    return out[0], out[1]


def parse_pwm_files(pwm_file, threshold_dir, pwm_threshold, wanted_pwms, add_reverse_patterns=True, dipwm_file=None,
                    pvalue=None, device=0):
    """pattern.rs:37-87.  Returns a PatternSet (index it or .to_list() for Pattern objects).
    dipwm_file: a dinucleotide PWM file (rows of 16 weights, AA AC .. TT) whose pattern ids
    continue after pwm_file's; pwm_file may then be None.  pvalue: every named definition
    loads and its strands take PatternSet.pvalue_thresholds' min_score, computed on `device`
    (-1: the host); threshold_dir may then be None and pwm_threshold is ignored."""
    h = C.c_void_p()
    if pvalue is not None:
        check(lib().tfbs_patterns_from_files_pvalue(_u(pwm_file) if pwm_file is not None else None,
                                                    _u(dipwm_file) if dipwm_file is not None else None,
                                                    _u(",".join(wanted_pwms)), 1 if add_reverse_patterns else 0,
                                                    device, pvalue, C.byref(h)))
    elif dipwm_file is None:
        check(lib().tfbs_patterns_from_files(_u(pwm_file), _u(threshold_dir), pwm_threshold,
                                             _u(",".join(wanted_pwms)), 1 if add_reverse_patterns else 0,
                                             C.byref(h)))
    else:
        check(lib().tfbs_patterns_from_files_di(_u(pwm_file), _u(dipwm_file), _u(threshold_dir), pwm_threshold,
                                                _u(",".join(wanted_pwms)), 1 if add_reverse_patterns else 0,
                                                C.byref(h)))
    return PatternSet(h)


def device_count():
    n = C.c_int()
    rc = lib().tfbs_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _nuc_codes(hap):
    return [NUCLEOTIDES.index(n.nuc if isinstance(n, NucleotidePos) else n[0]) for n in hap]


def patch_haplotype(rng, diffs, ref_haplotype):
    """haplotype.rs:94-156 (host C++ in libtfbs_amd).  diffs: [Diff(pos, 'REF', 'ALT')]."""
    L = lib()
    nd = len(diffs)
    dref = [NUCLEOTIDES.index(c) for d in diffs for c in d.reference]
    dalt = [NUCLEOTIDES.index(c) for d in diffs for c in d.alternative]
    n = len(ref_haplotype)
    cap = n + sum(len(d.alternative) for d in diffs) + 8
    on = (C.c_uint8 * cap)()
    op = (C.c_uint64 * cap)()
    nout = C.c_size_t()
    check(L.tfbs_patch_haplotype(
        rng[0], rng[1], nd, (C.c_uint64 * max(1, nd))(*[d.pos for d in diffs]),
        (C.c_uint8 * max(1, len(dref)))(*dref), (C.c_uint32 * max(1, nd))(*[len(d.reference) for d in diffs]),
        (C.c_uint8 * max(1, len(dalt)))(*dalt), (C.c_uint32 * max(1, nd))(*[len(d.alternative) for d in diffs]),
        (C.c_uint8 * max(1, n))(*_nuc_codes(ref_haplotype)),
        (C.c_uint64 * max(1, n))(*[x[1] for x in ref_haplotype]), n, on, op, cap, C.byref(nout)))
    return [NucleotidePos(NUCLEOTIDES[on[i]], op[i]) for i in range(nout.value)]


def counts_as_genotypes(v1, v2, verbose=False):
    """main.rs:439-498 -> (distinct_counts, maf, freq0, freq1, freq2, genotypes) or None."""
    n = len(v1)
    maf = C.c_uint32()
    info = C.create_string_buffer(64 + 16 * n)
    gts = C.create_string_buffer(64 + 24 * n)
    r = check(lib().tfbs_counts_as_genotypes((C.c_uint32 * max(1, n))(*v1), (C.c_uint32 * max(1, n))(*v2), n,
                                             C.byref(maf), info, len(info), gts, len(gts)))
    if r != 1:
        return None
    s = info.value.decode()
    counts_part, freqs_part = s.split(";")
    counts = [int(x) for x in counts_part[len("COUNTS="):].split(",")]
    f0, f1, f2 = (int(x) for x in freqs_part[len("freqs="):].split("/"))
    return counts, maf.value, f0, f1, f2, gts.value.decode()


def scores_as_genotypes(left, right, min_spread=1):
    """tfbs_scores_as_genotypes (host only): the score rows' definition on one candidate row's
    per-sample values (the two haplotypes' best scores, int32) -> (maf, info, genotypes), info =
    "SCORES=<lo>,<hi>;freqs=<zero>/<one>/<two>", or None when there is no row."""
    n = len(left)
    maf = C.c_uint32()
    info = C.create_string_buffer(128)
    gts = C.create_string_buffer(16 + 11 * n)
    r = check(lib().tfbs_scores_as_genotypes((C.c_int32 * max(1, n))(*left), (C.c_int32 * max(1, n))(*right), n,
                                             min_spread, C.byref(maf), info, len(info), gts, len(gts)))
    if r != 1:
        return None
    return maf.value, info.value.decode(), gts.value.decode()


def affinity_mlog2(xs, device=-1):
    """tfbs_affinity_mlog2: floor(1000 * log2(x)) of every x (u64; -1 for x = 0) as a list of ints,
    on the host (device -1) or in one launch of the affinity rows' device function on HIP device
    `device`."""
    n = len(xs)
    out = (C.c_int32 * max(1, n))()
    check(lib().tfbs_affinity_mlog2((C.c_uint64 * max(1, n))(*xs), n, device, out))
    return list(out[:n])


def affinity_as_genotypes(left, right, top, min_spread=1):
    """tfbs_affinity_as_genotypes (host only): the affinity rows' definition on one candidate row's
    per-sample values (the two haplotypes' affinity sums, u64 below 2^63) -> (maf, info, genotypes),
    info = "LOG2AFF=<lo>,<hi>;AFF=<xlo>,<xhi>;TOP=<top>;freqs=<zero>/<one>/<two>", or None when
    there is no row."""
    n = len(left)
    maf = C.c_uint32()
    info = C.create_string_buffer(224)
    gts = C.create_string_buffer(16 + 11 * n)
    r = check(lib().tfbs_affinity_as_genotypes((C.c_uint64 * max(1, n))(*left), (C.c_uint64 * max(1, n))(*right), n, top,
                                               min_spread, C.byref(maf), info, len(info), gts, len(gts)))
    if r != 1:
        return None
    return maf.value, info.value.decode(), gts.value.decode()


# tfbs_batch_assembly_paths' bits (tfbs_amd.h TFBS_PATH_*)
PATH_BITS = {"FAST": 1 << 0, "BIG": 1 << 1, "WALK": 1 << 2, "STEPBITS": 1 << 3, "DIRTY_LISTED": 1 << 4,
             "COR_ARENA": 1 << 5, "LISTS_SLICED": 1 << 6, "RUNS_L2": 1 << 7, "HAP_GLOBAL": 1 << 8, "U32": 1 << 9,
             "CNT_ARENA": 1 << 10, "TICKET": 1 << 11, "GIVEUP": 1 << 12, "ASM": 1 << 16, "ASM_HAPS": 1 << 17,
             "ASM_RUNS": 1 << 18, "ASM_HITS": 1 << 19, "ASM_REFS": 1 << 20, "ASM_SCRATCH": 1 << 21}
PATH_WHY_SHIFT = 13


def path_why(word):
    """TFBS_PATH_WHY: key_fast_kernel's give-up reason of a word with GIVEUP set."""
    return (word >> PATH_WHY_SHIFT) & 7


class Scanner:
    """A device context: the pattern tables resident on one GPU (one per host thread)."""

    def __init__(self, patterns, device=0):
        self.patterns = patterns if isinstance(patterns, PatternSet) else PatternSet.from_patterns(patterns)
        self.h = C.c_void_p()
        check(lib().tfbs_ctx_create(device, self.patterns.h, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().tfbs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def rows_bgzf_blocks(self):
        """tfbs_ctx_rows_bgzf_blocks: the BGZF blocks of the last RegionBatch.rows_bgzf call on
        this scanner -- {"blocks" (written), "wave" (all rows staged: bgzf_wave_kernel; the
        others went to bgzf_block_kernel), "stored" (BTYPE 00)}."""
        out = (C.c_uint64 * 3)()
        check(lib().tfbs_ctx_rows_bgzf_blocks(self.h, out))
        return dict(zip(("blocks", "wave", "stored"), (int(x) for x in out)))

    def assembly_trace(self, on=True):
        """tfbs_ctx_assembly_trace: the assemblies enqueued from now on report each region's path
        (RegionBatch.assembly_paths)."""
        check(lib().tfbs_ctx_assembly_trace(self.h, 1 if on else 0))

    def region_asm(self):
        """tfbs_ctx_region_asm: the key assembly's static records of what was last uploaded --
        (region_asm, hap_reuse): per region (run0, nruns, lmax, 0), per haplotype its reuse
        descriptor (0xFFFFFFFF: none, else (run offset - run0) | runs << 16)."""
        nr, nh = C.c_size_t(0), C.c_size_t(0)
        check(lib().tfbs_ctx_region_asm(self.h, None, 0, None, 0, C.byref(nr), C.byref(nh)))
        ra = (C.c_uint32 * (4 * max(nr.value, 1)))()
        hr = (C.c_uint32 * max(nh.value, 1))()
        check(lib().tfbs_ctx_region_asm(self.h, ra, max(nr.value, 1), hr, max(nh.value, 1), C.byref(nr), C.byref(nh)))
        return ([tuple(ra[4 * r:4 * r + 4]) for r in range(nr.value)], list(hr[:nh.value]))

    def assembly_figures(self):
        """tfbs_ctx_assembly_figures of the last checked assembly: {"left" (regions left to
        key_asm_kernel), "arena" (arena words asked for), "spill" (spill records), "wide" /
        "leftover" (it launched the wide spill kernels / the leftover pass), and since the scanner
        was made "reruns" (lean assemblies run again in full), "reruns_wide" / "reruns_leftover"
        (those that needed the wide kernels / the leftover pass)}."""
        out = (C.c_uint64 * 8)()
        check(lib().tfbs_ctx_assembly_figures(self.h, out))
        return dict(zip(("left", "arena", "spill", "wide", "leftover", "reruns", "reruns_wide", "reruns_leftover"),
                        (int(x) for x in out)))

    def post_figures(self):
        """tfbs_ctx_post_figures of the last checked assembly: {"left_out" (it ran without the
        post-scan stage: no rescoring, no spill buckets), "reruns_post" (since the scanner was made:
        assemblies that had left it out, reported a spill record or a candidate past the lists and
        ran again in full), "fused" (the stage ran in the scan kernel's last workgroup), "cand" (the
        scan's candidates past the waves' lists), "in_place" (left out, and the assembly's kernels
        read the scan's spill records where they lay, up to TFBS_SPILL_INPLACE of them)}."""
        out = (C.c_uint64 * 4)()
        check(lib().tfbs_ctx_post_figures(self.h, out))
        left_out, reruns_post, how, cand = (int(x) for x in out)
        return {"left_out": left_out, "reruns_post": reruns_post, "fused": int(how == 1), "cand": cand,
                "in_place": int(how == 2)}

    def matches_all(self, haplotype):
        """pattern.rs:141-171 for every pattern: list (per pattern, creation order) of [(start, end)]."""
        n = len(haplotype)
        nucs = (C.c_uint8 * max(1, n))(*_nuc_codes(haplotype))
        pos = (C.c_uint64 * max(1, n))(*[x[1] for x in haplotype])
        npat = len(self.patterns)
        counts = (C.c_uint32 * max(1, npat))()
        total = C.c_size_t()
        cap = 64
        while True:
            s = (C.c_uint64 * cap)()
            e = (C.c_uint64 * cap)()
            rc = lib().tfbs_matches(self.h, nucs, pos, n, counts, s, e, cap, C.byref(total))
            if rc == -1 and total.value > cap:
                cap = total.value
                continue
            check(rc)
            break
        out, k = [], 0
        for i in range(npat):
            out.append([(s[k + j], e[k + j]) for j in range(counts[i])])
            k += counts[i]
        return out

    def matches(self, pattern_index, haplotype, haplotype_ids=()):
        p = self.patterns[pattern_index]
        ids = tuple(haplotype_ids)
        return [Match(Range(a, b), p.pattern_id, ids) for a, b in self.matches_all(haplotype)[pattern_index]]

    def last_scan_ms(self):
        return lib().tfbs_ctx_last_scan_ms(self.h)

    def last_best_ms(self):
        """tfbs_ctx_last_best_ms: (kernel ms from HIP events, copy-back + host ms) of the last best()."""
        out = (C.c_double * 2)()
        check(lib().tfbs_ctx_last_best_ms(self.h, out))
        return out[0], out[1]

    def last_affinity_ms(self):
        """tfbs_ctx_last_affinity_ms: (kernel ms from HIP events, copy-back + host ms) of the last affinity()."""
        out = (C.c_double * 2)()
        check(lib().tfbs_ctx_last_affinity_ms(self.h, out))
        return out[0], out[1]

    def last_affinity_rows_ms(self):
        """tfbs_ctx_last_affinity_rows_ms: (affinity kernel, fold + statistics, text kernel ms from HIP
        events, copy-back + host ms) of the last affinity_rows()."""
        out = (C.c_double * 4)()
        check(lib().tfbs_ctx_last_affinity_rows_ms(self.h, out))
        return tuple(out)

    def last_scores_ms(self):
        """tfbs_ctx_last_scores_ms: (best kernel, fold + statistics, text kernel ms from HIP events,
        copy-back + host ms) of the last score_rows()."""
        out = (C.c_double * 4)()
        check(lib().tfbs_ctx_last_scores_ms(self.h, out))
        return tuple(out)

    def last_effects_ms(self):
        """tfbs_ctx_last_effects_ms: (host prep ms, kernel ms from HIP events, copy-back + host ms)
        of the last effects()."""
        out = (C.c_double * 3)()
        check(lib().tfbs_ctx_last_effects_ms(self.h, out))
        return out[0], out[1], out[2]

    def last_mutscan_ms(self):
        """tfbs_ctx_last_mutscan_ms: (host packing ms, count pass + offset scan ms, fill pass ms from HIP
        events, copy-back + host ms) of the last mutscan() or mutscan_count()."""
        out = (C.c_double * 4)()
        check(lib().tfbs_ctx_last_mutscan_ms(self.h, out))
        return tuple(out)


def mutscan_ring_max_length():
    """tfbs_mutscan_ring_max_length: the longest strand the mutation-scan kernel's ring serves."""
    return lib().tfbs_mutscan_ring_max_length()


def mutscan_kinds_mask(kinds):
    """A mask of MUT_* from an int or from names ("gain,loss" or a list of them)."""
    if isinstance(kinds, int):
        return kinds
    names = kinds.split(",") if isinstance(kinds, str) else list(kinds)
    mask = 0
    for k in names:
        mask |= 1 << MUT_KINDS.index(k)
    return mask


def matches(pattern, haplotype, haplotype_ids=(), verbose=False):
    """pattern.rs:141-171 for one Pattern on one haplotype (GPU; builds a one-pattern Scanner)."""
    sc = Scanner([pattern])
    try:
        return sc.matches(0, haplotype, haplotype_ids)
    finally:
        sc.close()


GROUPER_HOST = -2  # TFBS_GROUPER_HOST: the host grouper (Grouper, RegionBatch(build_device=...))
GroupedRegion = namedtuple("GroupedRegion", "n_groups masks counts row")  # n_groups None: overflow


class Grouper:
    """tfbs_grouper_*: the haplotype grouper of RegionBatch(build_device=...) driven alone."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().tfbs_grouper_create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().tfbs_grouper_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def group(self, H, regions):
        """One launch.  regions: per region its records, each the ascending haplotype ids
        (< H) carrying it; a record's rank is its index.  -> one GroupedRegion per region:
        the distinct masks in the grouper's order, their carrier counts and the membership
        row (H entries)."""
        n_rec = [len(r) for r in regions]
        n_car = [len(c) for r in regions for c in r]
        ids = [h for r in regions for c in r for h in c]
        nr = len(regions)
        cap = 2047 * nr
        ng = (C.c_uint32 * max(1, nr))()
        masks = (C.c_uint64 * max(1, cap))()
        counts = (C.c_uint32 * max(1, cap))()
        rows = (C.c_uint16 * max(1, nr * H))()
        n = C.c_size_t()
        check(lib().tfbs_grouper_group(self.h, H, nr, (C.c_uint32 * max(1, nr))(*n_rec),
                                       (C.c_uint32 * max(1, len(n_car)))(*n_car),
                                       (C.c_uint32 * max(1, len(ids)))(*ids), ng, masks, counts, cap, C.byref(n),
                                       rows))
        out, at = [], 0
        for j in range(nr):
            row = list(rows[j * H:(j + 1) * H])
            if ng[j] == 0xFFFFFFFF:
                out.append(GroupedRegion(None, [], [], row))
                continue
            out.append(GroupedRegion(ng[j], list(masks[at:at + ng[j]]), list(counts[at:at + ng[j]]), row))
            at += ng[j]
        assert at == n.value
        return out


class RegionBatch:
    """load_haplotypes + find_all_matches + count_matches_by_sample over many merged regions."""

    VECTOR_END = -2147483647

    def __init__(self, patterns, n_samples, keep_membership=True, window_lmax=None, build_device=None,
                 keep_variants=False):
        self.patterns = patterns
        self.n_samples = n_samples
        self.h = C.c_void_p()
        check(lib().tfbs_batch_create(patterns.h, n_samples, 1 if keep_membership else 0, C.byref(self.h)))
        self.beds = []
        if window_lmax is not None:  # a pattern shard: the whole set's windows (tfbs_batch_set_window_lmax)
            check(lib().tfbs_batch_set_window_lmax(self.h, window_lmax))
        if build_device is not None:  # haplotype grouping on a device (tfbs_batch_set_build_device)
            check(lib().tfbs_batch_set_build_device(self.h, build_device))
        if keep_variants:  # the regions keep their records (tfbs_batch_keep_variants): variants(), effects()
            self.keep_variants(True)

    def keep_variants(self, on=True):
        """tfbs_batch_keep_variants: before the first region."""
        check(lib().tfbs_batch_keep_variants(self.h, 1 if on else 0))

    def build_stats(self):
        """(regions grouped on the device, regions built on the host)."""
        d, h = C.c_uint64(), C.c_uint64()
        check(lib().tfbs_batch_build_stats(self.h, C.byref(d), C.byref(h)))
        return d.value, h.value

    def group_calls(self):
        """Chunks of regions handed to the grouper so far (one launch each)."""
        n = C.c_uint64()
        check(lib().tfbs_batch_group_calls(self.h, C.byref(n)))
        return n.value

    def patch_stats(self):
        """Regions grouped on the device whose distinct groups the host patched."""
        p = C.c_uint64()
        check(lib().tfbs_batch_patch_stats(self.h, C.byref(p)))
        return p.value

    def __del__(self):
        if getattr(self, "h", None):
            lib().tfbs_batch_destroy(self.h)
            self.h = None

    def add_bed(self, basename):
        self.beds.append(basename)
        return check(lib().tfbs_batch_add_bed(self.h, _u(basename)))

    def ext(self, start, end):
        es, ee = C.c_uint64(), C.c_uint64()
        check(lib().tfbs_batch_region_ext(self.h, start, end, C.byref(es), C.byref(ee)))
        return es.value, ee.value

    def begin(self, start, end, ref_ascii):
        check(lib().tfbs_batch_region_begin(self.h, start, end, _u(ref_ascii), len(ref_ascii)))

    def add_inner(self, bed, start, end):
        check(lib().tfbs_batch_region_add_inner(self.h, bed, start, end))

    def add_record_gt(self, pos, n_alleles, ref, alt, gts):
        flat = [x for g in gts for x in (list(g[:2]) + [self.VECTOR_END] * (2 - len(g[:2])))]
        check(lib().tfbs_batch_region_add_record_gt(self.h, pos, n_alleles, _u(ref), _u(alt),
                                                    (C.c_int32 * max(1, len(flat)))(*flat)))

    def add_record_carriers(self, pos, ref, alt, hap_ids):
        hap_ids = list(hap_ids)
        check(lib().tfbs_batch_region_add_record_carriers(self.h, pos, _u(ref), _u(alt),
                                                          (C.c_uint32 * max(1, len(hap_ids)))(*hap_ids),
                                                          len(hap_ids)))

    def end(self):
        check(lib().tfbs_batch_region_end(self.h))

    @contextlib.contextmanager
    def hold(self):
        """tfbs_batch_hold: the regions ended inside the block are built together when it
        ends (several host threads, one grouper launch per chunk); until then they are
        not part of the batch."""
        check(lib().tfbs_batch_hold(self.h, 1))
        try:
            yield self
        finally:
            check(lib().tfbs_batch_hold(self.h, 0))

    def synth_fill(self, seed, first, count, indel_pct=0):
        check(lib().tfbs_synth_fill_batch(self.h, seed, first, count, indel_pct))
        if "synthetic.bed" not in self.beds:  # registered by the library on first use
            self.beds.append("synthetic.bed")

    @property
    def num_regions(self):
        return lib().tfbs_batch_num_regions(self.h)

    @property
    def num_haplotypes(self):
        return lib().tfbs_batch_num_haplotypes(self.h)

    @property
    def num_windows(self):
        return lib().tfbs_batch_num_windows(self.h)

    @property
    def num_cell_ops(self):
        return lib().tfbs_batch_num_cell_ops(self.h)

    @property
    def num_effective_windows(self):
        return lib().tfbs_batch_num_effective_windows(self.h)

    @property
    def num_scan_windows(self):
        """Windows the scan executes (reference-window reuse skips SNV-only haplotypes'
        windows equal to the reference's)."""
        return lib().tfbs_batch_num_scan_windows(self.h)

    @property
    def num_scan_cell_ops(self):
        return lib().tfbs_batch_num_scan_cell_ops(self.h)

    @property
    def input_bytes(self):
        return lib().tfbs_batch_input_bytes(self.h)

    @property
    def output_bytes(self):
        return lib().tfbs_batch_output_bytes(self.h)

    def region_stats(self, r):
        a, b = C.c_uint32(), C.c_uint32()
        check(lib().tfbs_batch_region_stats(self.h, r, C.byref(a), C.byref(b)))
        return a.value, b.value

    def scan(self, scanner, upload=True, download=True, reduce=False, encode=False):
        """tfbs_scan; then either download the dense counts or (reduce=True) classify the
        keys on the GPU and fetch only what row emission needs (tfbs_batch_reduce), and
        (encode=True) encode every varying key's per-sample totals on the GPU
        (tfbs_batch_encode) so rows format from codes."""
        if upload:
            check(lib().tfbs_batch_upload(scanner.h, self.h))
        check(lib().tfbs_scan(scanner.h, self.h))
        if reduce or encode:
            check(lib().tfbs_batch_reduce(scanner.h, self.h))
            if encode:
                self.encode(scanner)
        elif download:
            check(lib().tfbs_batch_download(scanner.h, self.h))

    def encode(self, scanner, r0=0, r1=None, device_codes=False):
        """tfbs_batch_encode for regions [r0, r1) (after a reduced scan); device_codes: keep the
        per-sample codes on the GPU (for rows_bgzf)."""
        check(lib().tfbs_batch_encode_flags(scanner.h, self.h, r0, self.num_regions if r1 is None else r1,
                                            1 if device_codes else 0))

    def encode_stats(self):
        """tfbs_batch_encode_stats: which path the varying keys of the last encode() took --
        {"keys", "w2", "w4", "w8" (encoded at that code width), "no_pairs" (the region's
        haplotype pairs were not listed), "range", "values" (left to the host for the total
        range / the number of distinct totals)}; keys is the sum of the others."""
        out = (C.c_uint64 * 7)()
        check(lib().tfbs_batch_encode_stats(self.h, out))
        return dict(zip(("keys", "w2", "w4", "w8", "no_pairs", "range", "values"), (int(x) for x in out)))

    def assembly_paths(self, scanner):
        """tfbs_batch_assembly_paths: the TFBS_PATH_* word of every region from the last checked
        assembly on a scanner with assembly_trace() on."""
        n = self.num_regions
        out = (C.c_uint32 * max(1, n))()
        check(lib().tfbs_batch_assembly_paths(scanner.h, self.h, out, n))
        return [int(x) for x in out[:n]]

    def layout(self, region):
        """tfbs_batch_region_layout: (hap_begin, hap_count, ref_hap or None, n_inner)."""
        out = (C.c_uint32 * 4)()
        check(lib().tfbs_batch_region_layout(self.h, region, out))
        return out[0], out[1], (None if out[2] == 0xFFFFFFFF else out[2]), out[3]

    def hap_runs(self, region, h):
        """tfbs_batch_region_hap_runs: (reuses the reference's hits, offset of its runs in the
        batch's run array, [(a, b)] its diff runs in the reference's columns)."""
        reuses, off, n = C.c_int(), C.c_uint32(), C.c_uint32()
        ab = (C.c_uint32 * 64)()
        check(lib().tfbs_batch_region_hap_runs(self.h, region, h, C.byref(reuses), C.byref(off), C.byref(n), ab, 32))
        return bool(reuses.value), off.value, [(ab[2 * k], ab[2 * k + 1]) for k in range(n.value)]

    def hap_own_runs(self, region, h):
        """tfbs_batch_region_hap_own_runs: (reuses the reference's hits, offset of its runs in the
        batch's run array, [(a, b)] its diff runs in its own columns: what the scan reads)."""
        reuses, off, n = C.c_int(), C.c_uint32(), C.c_uint32()
        ab = (C.c_uint32 * 64)()
        check(lib().tfbs_batch_region_hap_own_runs(self.h, region, h, C.byref(reuses), C.byref(off), C.byref(n), ab,
                                                   32))
        return bool(reuses.value), off.value, [(ab[2 * k], ab[2 * k + 1]) for k in range(n.value)]

    def keys(self, region):
        """count_matches_by_sample for one region: {(bed, (s, e), pattern_id): (L, R)}."""
        L = lib()
        n = C.c_size_t()
        check(L.tfbs_batch_region_num_keys(self.h, region, C.byref(n)))
        out = {}
        ns = self.n_samples
        for k in range(n.value):
            bed, s, e, pid = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint16()
            l = (C.c_uint32 * max(1, ns))()
            r = (C.c_uint32 * max(1, ns))()
            check(L.tfbs_batch_region_key(self.h, region, k, C.byref(bed), C.byref(s), C.byref(e), C.byref(pid), l,
                                          r))
            out[(self.beds[bed.value], (s.value, e.value), pid.value)] = (list(l[:ns]), list(r[:ns]))
        return out

    def keys_np(self, region):
        """keys() with numpy uint32 vectors (large sample counts)."""
        import numpy as np
        L = lib()
        n = C.c_size_t()
        check(L.tfbs_batch_region_num_keys(self.h, region, C.byref(n)))
        out = {}
        ns = self.n_samples
        for k in range(n.value):
            bed, s, e, pid = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint16()
            l = np.zeros(max(1, ns), dtype=np.uint32)
            r = np.zeros(max(1, ns), dtype=np.uint32)
            check(L.tfbs_batch_region_key(self.h, region, k, C.byref(bed), C.byref(s), C.byref(e), C.byref(pid),
                                          l.ctypes.data_as(_capi.u32p), r.ctypes.data_as(_capi.u32p)))
            out[(self.beds[bed.value], (s.value, e.value), pid.value)] = (l[:ns], r[:ns])
        return out

    def region_rows(self, region, chromosome, min_maf=0, fake_position=1):
        """Rows of one region (main.rs:415-429); returns (text, next fake_position)."""
        fp = C.c_uint32(fake_position)
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib().tfbs_batch_region_rows(self.h, region, _u(chromosome), min_maf, C.byref(fp), C.byref(p),
                                           C.byref(n)))
        try:
            text = C.string_at(p, n.value).decode()
        finally:
            lib().tfbs_free(p)
        return text, fp.value

    def digest(self, region):
        """tfbs_batch_region_digest: the region's keys at the distinct-haplotype level."""
        d = C.c_uint64()
        check(lib().tfbs_batch_region_digest(self.h, region, C.byref(d)))
        return d.value

    def key_digest_sum(self, region):
        """tfbs_batch_region_key_digest_sum: order-free; pattern shards add up to the whole."""
        d = C.c_uint64()
        check(lib().tfbs_batch_region_key_digest_sum(self.h, region, C.byref(d)))
        return d.value

    def region_digests(self, r0=0, r1=None, min_maf=0, threads=16, keys=True, rows=True):
        """tfbs_batch_region_digests over regions [r0, r1): numpy uint64 arrays (keys, rows,
        n_rows) -- the canonical sketch of each region's count_matches_by_sample vectors and
        XXH64 of its rows without POS, comparable with the oracle's orc_job_digests (None for
        a digest not asked for)."""
        import numpy as np
        r1 = self.num_regions if r1 is None else r1
        n = max(1, r1 - r0)
        k, r, c = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        p = C.POINTER(C.c_uint64)
        ptr = lambda a, on: a.ctypes.data_as(p) if on else None
        check(lib().tfbs_batch_region_digests(self.h, r0, r1, min_maf, threads, ptr(k, keys), ptr(r, rows),
                                              ptr(c, rows)))
        return (k[:r1 - r0] if keys else None), (r[:r1 - r0] if rows else None), (c[:r1 - r0] if rows else None)

    def input_digest(self, region):
        """tfbs_batch_region_input_digest: what the host prep packed for the region."""
        d = C.c_uint64()
        check(lib().tfbs_batch_region_input_digest(self.h, region, C.byref(d)))
        return d.value

    def format_rows(self, chromosome, min_maf=0, threads=1, r0=0, r1=None):
        """Format the rows of regions [r0, r1) on host threads and discard them: (rows, bytes)."""
        r, n = C.c_uint64(), C.c_uint64()
        check(lib().tfbs_batch_format_rows(self.h, _u(chromosome), min_maf, threads, r0,
                                           self.num_regions if r1 is None else r1, C.byref(r), C.byref(n)))
        return r.value, n.value

    def prep_seconds(self):
        """(generation CPU-s, build_region CPU-s, build + commit wall-s, fill wall-s) of synth_fill."""
        out = (C.c_double * 4)()
        check(lib().tfbs_batch_prep_seconds(self.h, out))
        return tuple(out)

    def rows_bgzf(self, scanner, chromosome, min_maf=0, fake_position=1, r0=0, r1=None, fd=None):
        """tfbs_batch_rows_bgzf: the rows of regions [r0, r1) as BGZF blocks built on the
        GPU (after encode over them), written to file descriptor fd; without fd they are
        returned.  Returns (bytes or bytes written, next fake_position, rows, text bytes)."""
        import os
        import tempfile
        fp = C.c_uint32(fake_position)
        nw, nr, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        tmp = None
        if fd is None:
            tmp = tempfile.TemporaryFile()
            fd_ = tmp.fileno()
        else:
            fd_ = fd
        try:
            check(lib().tfbs_batch_rows_bgzf(scanner.h, self.h, r0, self.num_regions if r1 is None else r1,
                                             _u(chromosome), min_maf, C.byref(fp), fd_, C.byref(nw), C.byref(nr),
                                             C.byref(nb)))
            if tmp is not None:
                tmp.seek(0)
                out = tmp.read()
            else:
                out = nw.value
        finally:
            if tmp is not None:
                tmp.close()
        return out, fp.value, nr.value, nb.value

    def upload(self, scanner):
        """tfbs_batch_upload: the packed batch resident on the scanner (what hits() needs)."""
        check(lib().tfbs_batch_upload(scanner.h, self.h))

    def _span(self, r0, r1):
        return 0 if r0 is None else r0, self.num_regions if r1 is None else r1

    def _records(self, call, ctype, dtype, *args):
        """A record call's malloc'd array of ctype (call(*args, &p, &n)) as a numpy structured array."""
        import numpy as np
        p = C.c_void_p()
        n = C.c_size_t()
        check(call(*args, C.byref(p), C.byref(n)))
        try:
            return np.frombuffer(C.string_at(p, n.value * C.sizeof(ctype)), dtype=dtype).copy()
        finally:
            lib().tfbs_free(p)

    def _tsv(self, call, arr, dtype, header_text, header, *args):
        """A *_tsv call's text for the records arr (call(batch, records, n, *args, &p, &n))."""
        import numpy as np
        arr = np.ascontiguousarray(arr, dtype=dtype)
        p = C.c_void_p()
        n = C.c_size_t()
        check(call(self.h, arr.ctypes.data_as(C.c_void_p), len(arr), *args, C.byref(p), C.byref(n)))
        try:
            text = C.string_at(p, n.value).decode()
        finally:
            lib().tfbs_free(p)
        return (header_text if header else "") + text

    def _by_sample(self, recs, region, field, what):
        """(recs[field], recs["n_windows"]) of one region as [2 * n_samples][n_patterns][n_ranges]."""
        import numpy as np
        mine = recs[recs["region"] == region]
        nh, nr = self.region_stats(region)[0], len(self.ranges(region))
        npat = len(mine) // (nh * nr) if nh * nr else 0
        if npat * nh * nr != len(mine) or (nh * nr and npat != len(self.patterns)):
            raise ValueError("%s does not hold region %d in full" % (what, region))
        memb = np.asarray(self.membership(region), dtype=np.int64)
        return mine[field].reshape(nh, npat, nr)[memb], mine["n_windows"].reshape(nh, npat, nr)[memb]

    def hits(self, scanner, r0=0, r1=None):
        """tfbs_batch_hits: find_all_matches (main.rs:94-154) for regions [r0, r1) of this batch,
        resident on the scanner (after an upload; no scan needed): a numpy structured array
        (HIT_DTYPE: region, haplotype, pattern, window, start, end, score) sorted by (region,
        haplotype, pattern, window)."""
        return self._records(lib().tfbs_batch_hits, _capi.tfbs_hit, HIT_DTYPE, scanner.h, self.h, *self._span(r0, r1))

    def hits_count(self, scanner, r0=0, r1=None):
        """tfbs_batch_hits_count: the hits of each region of [r0, r1) (numpy uint64), count pass only."""
        import numpy as np
        r1 = self.num_regions if r1 is None else r1
        out = np.zeros(max(1, r1 - r0), dtype=np.uint64)
        check(lib().tfbs_batch_hits_count(scanner.h, self.h, r0, r1, out.ctypes.data_as(_capi.u64p)))
        return out[:r1 - r0]

    def haplotype(self, region, h):
        """tfbs_batch_region_haplotype: (codes 0-4, positions, carrier ids' number) of distinct
        haplotype h of a region, as load_haplotypes made it."""
        n, car = C.c_size_t(), C.c_uint32()
        rc = lib().tfbs_batch_region_haplotype(self.h, region, h, None, None, 0, C.byref(n), C.byref(car))
        if rc != 0 and n.value == 0:
            check(rc)
        cap = n.value
        nucs = (C.c_uint8 * max(1, cap))()
        pos = (C.c_uint64 * max(1, cap))()
        check(lib().tfbs_batch_region_haplotype(self.h, region, h, nucs, pos, cap, C.byref(n), C.byref(car)))
        return tuple(nucs[:cap]), tuple(pos[:cap]), car.value

    def membership(self, region):
        """tfbs_batch_region_membership: list, [haplotype id 2 * sample + side] -> distinct index."""
        out = (C.c_uint32 * max(1, 2 * self.n_samples))()
        check(lib().tfbs_batch_region_membership(self.h, region, out))
        return list(out[:2 * self.n_samples])

    def hits_tsv(self, hits, chromosome, mode="diff", header=False):
        """tfbs_batch_hits_tsv: the TSV of a hits() result over whole regions; mode "all" (one
        `hit` line per hit) or "diff" (every region of the batch: `hap` lines, the baseline's
        `base` lines, the others' `gain` / `loss` lines); header: HITS_HEADER first."""
        return self._tsv(lib().tfbs_batch_hits_tsv, hits, HIT_DTYPE, HITS_HEADER, header, _u(chromosome), HITS_MODES[mode])

    def best(self, scanner, r0=None, r1=None):
        """tfbs_batch_best: the best-scoring site per (distinct haplotype, pattern strand, inner
        range) of regions [r0, r1) of this batch, resident on the scanner (after an upload; no
        scan needed): a dense numpy structured array (BEST_DTYPE) sorted by (region, haplotype,
        pattern, range); a region's block reshapes to [n_haplotypes][n_patterns][n_ranges]."""
        return self._records(lib().tfbs_batch_best, _capi.tfbs_best, BEST_DTYPE, scanner.h, self.h, *self._span(r0, r1))

    def score_rows(self, scanner, chromosome, min_maf=0, min_spread=1, fake_position=1, r0=None, r1=None):
        """tfbs_batch_score_rows: the score rows of regions [r0, r1) of this batch, resident on the
        scanner (after an upload; no scan needed; the batch keeps its membership) -> (text, n_rows,
        next_position).  fake_position None: counted only -> ("", n_rows, None)."""
        return self._rows_text(lib().tfbs_batch_score_rows, scanner, chromosome, min_maf, min_spread, fake_position, r0, r1)

    def affinity_rows(self, scanner, chromosome, min_maf=0, min_spread=1, fake_position=1, r0=None, r1=None):
        """tfbs_batch_affinity_rows: the affinity rows of regions [r0, r1) of this batch, as
        score_rows (min_spread in milli-bits) -> (text, n_rows, next_position)."""
        return self._rows_text(lib().tfbs_batch_affinity_rows, scanner, chromosome, min_maf, min_spread, fake_position, r0, r1)

    def _rows_text(self, call, scanner, chromosome, min_maf, min_spread, fake_position, r0, r1):
        p = C.c_void_p()
        n = C.c_size_t()
        rows = C.c_uint64()
        a, z = 0 if r0 is None else r0, self.num_regions if r1 is None else r1
        if fake_position is None:
            check(call(scanner.h, self.h, a, z, _u(chromosome), min_maf, min_spread, None, None, None, C.byref(rows)))
            return "", rows.value, None
        fp = C.c_uint32(fake_position)
        check(call(scanner.h, self.h, a, z, _u(chromosome), min_maf, min_spread, C.byref(fp), C.byref(p), C.byref(n),
                   C.byref(rows)))
        try:
            text = C.string_at(p, n.value).decode()
        finally:
            lib().tfbs_free(p)
        return text, rows.value, fp.value

    def ranges(self, region):
        """The region's distinct non-empty inner ranges [(start, end)] in ascending order: what
        a best record's `range` indexes."""
        n = C.c_size_t()
        check(lib().tfbs_batch_region_num_ranges(self.h, region, C.byref(n)))
        out = []
        for k in range(n.value):
            s, e = C.c_uint64(), C.c_uint64()
            check(lib().tfbs_batch_region_range(self.h, region, k, C.byref(s), C.byref(e)))
            out.append((s.value, e.value))
        return out

    def best_tsv(self, best, chromosome, mode="diff", header=False):
        """tfbs_batch_best_tsv: the TSV of a best() result over whole regions; mode "all" (one
        `best` line per (key, pattern_id, haplotype)) or "diff" (`hap` lines, then `base` and
        `alt` lines where a haplotype's best differs from the baseline's); header: BEST_HEADER first."""
        return self._tsv(lib().tfbs_batch_best_tsv, best, BEST_DTYPE, BEST_HEADER, header, _u(chromosome), BEST_MODES[mode])

    def best_by_sample(self, best, region):
        """(scores, n_windows): int32 / uint32 arrays [2 * n_samples][n_patterns][n_ranges] of one
        region, row id = the records of the distinct haplotype that haplotype id 2 * sample + side
        carries (membership); `best` must hold that region in full."""
        return self._by_sample(best, region, "score", "best")

    def affinity(self, scanner, r0=None, r1=None):
        """tfbs_batch_affinity: the total binding affinity per (distinct haplotype, pattern strand,
        inner range) of regions [r0, r1) of this batch, resident on the scanner (after an upload; no
        scan needed): a dense numpy structured array (AFFINITY_DTYPE) sorted by (region, haplotype,
        pattern, range); `sum` is the exact integer sum of affinity_weight(top - score) over the
        range's windows."""
        return self._records(lib().tfbs_batch_affinity, _capi.tfbs_affinity, AFFINITY_DTYPE, scanner.h, self.h,
                             *self._span(r0, r1))

    def affinity_tsv(self, aff, chromosome, mode="diff", header=False):
        """tfbs_batch_affinity_tsv: the TSV of an affinity() result over whole regions; mode "all"
        (one `aff` line per (key, pattern_id, haplotype)) or "diff" (`hap` lines, then `base` and
        `alt` lines where a haplotype's sum differs from the baseline's); header: AFFINITY_HEADER first."""
        return self._tsv(lib().tfbs_batch_affinity_tsv, aff, AFFINITY_DTYPE, AFFINITY_HEADER, header, _u(chromosome),
                         AFFINITY_MODES[mode])

    def affinity_by_sample(self, aff, region):
        """(sums, n_windows): uint64 / uint32 arrays [2 * n_samples][n_patterns][n_ranges] of one
        region, row id = the records of the distinct haplotype that haplotype id 2 * sample + side
        carries (membership); `aff` must hold that region in full."""
        return self._by_sample(aff, region, "sum", "aff")

    def variants(self, region):
        """tfbs_batch_region_variant: the region's records in BCF order as (pos, ref, alt, n_alleles,
        carriers, status) -- ref / alt as ACGTN text, carriers the number of carrier ids, status one
        of VAR_SCORED, VAR_MULTIALLELIC, VAR_NO_CARRIER, VAR_UNPATCHED.  Needs keep_variants."""
        out = []
        for v in range(self.region_stats(region)[1]):
            pos = C.c_uint64()
            nr, na = C.c_size_t(), C.c_size_t()
            nal, car, st = C.c_uint32(), C.c_uint32(), C.c_uint32()
            rc = lib().tfbs_batch_region_variant(self.h, region, v, None, None, None, 0, C.byref(nr), C.byref(na),
                                                 None, None, None)
            if rc != 0 and nr.value == 0 and na.value == 0:
                check(rc)
            cap = max(nr.value, na.value)
            ref, alt = (C.c_uint8 * max(1, cap))(), (C.c_uint8 * max(1, cap))()
            check(lib().tfbs_batch_region_variant(self.h, region, v, C.byref(pos), ref, alt, cap, C.byref(nr),
                                                  C.byref(na), C.byref(nal), C.byref(car), C.byref(st)))
            out.append((pos.value, "".join("ACGTN"[c] for c in ref[:nr.value]),
                        "".join("ACGTN"[c] for c in alt[:na.value]), nal.value, car.value, st.value))
        return out

    def effects(self, scanner, r0=None, r1=None):
        """tfbs_batch_effects: per (record, pattern strand) of regions [r0, r1) the best site touching
        the record on the REF and on the ALT allele, on a scanner made from this batch's patterns
        (no upload, no scan needed): a dense numpy structured array (EFFECT_DTYPE) sorted by
        (region, variant, pattern); a region's block reshapes to [n_variants][n_patterns]."""
        return self._records(lib().tfbs_batch_effects, _capi.tfbs_effect, EFFECT_DTYPE, scanner.h, self.h, *self._span(r0, r1))

    def effects_tsv(self, eff, chromosome, mode="sites", header=False):
        """tfbs_batch_effects_tsv: the TSV of an effects() result over whole regions; per record a
        `var` line, then per pattern strand mode "sites": its `gain`, `loss` and `change` lines, or
        "all": `same` and `none` lines too; header: EFFECTS_HEADER first."""
        return self._tsv(lib().tfbs_batch_effects_tsv, eff, EFFECT_DTYPE, EFFECTS_HEADER, header, _u(chromosome),
                         EFFECT_MODES[mode])

    def mutscan(self, scanner, r0=None, r1=None, kinds=MUT_SITES):
        """tfbs_batch_mutscan: per (pattern strand, column of the region's reference window, other
        base) of regions [r0, r1) the best site covering the column before and after the substitution
        and the record's kind, for the kinds in the mask, on a scanner made from this batch's patterns
        (no upload, no scan needed; needs keep_variants): a sparse numpy structured array
        (MUTATION_DTYPE) sorted by (region, pattern, column, alt)."""
        return self._records(lib().tfbs_batch_mutscan, _capi.tfbs_mutation, MUTATION_DTYPE, scanner.h, self.h,
                             *self._span(r0, r1), mutscan_kinds_mask(kinds))

    def mutscan_count(self, scanner, r0=None, r1=None, kinds=MUT_SITES):
        """tfbs_batch_mutscan_count: len(mutscan(...)) from the count pass alone."""
        n = C.c_uint64()
        check(lib().tfbs_batch_mutscan_count(scanner.h, self.h, 0 if r0 is None else r0,
                                             self.num_regions if r1 is None else r1, mutscan_kinds_mask(kinds),
                                             C.byref(n)))
        return n.value

    def mutscan_tsv(self, m, chromosome, header=False):
        """tfbs_batch_mutscan_tsv: one line per record of a mutscan() result (any subset, in its
        order); header: MUTSCAN_HEADER first."""
        return self._tsv(lib().tfbs_batch_mutscan_tsv, m, MUTATION_DTYPE, MUTSCAN_HEADER, header, _u(chromosome))

    def rows(self, chromosome, min_maf=0, fake_position=1):
        """Rows for every region (main.rs:415-429); returns (text, next fake_position)."""
        fp = C.c_uint32(fake_position)
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib().tfbs_batch_rows(self.h, _u(chromosome), min_maf, C.byref(fp), C.byref(p), C.byref(n)))
        try:
            text = C.string_at(p, n.value).decode()
        finally:
            lib().tfbs_free(p)
        return text, fp.value


class SynthRegion:
    """A synthetic phased region."""

    def __init__(self, seed, index, n_samples, lmax, indel_pct=0):
        L = lib()
        self.h = C.c_void_p()
        check(L.tfbs_synth_region_make(seed, index, n_samples, lmax, indel_pct, C.byref(self.h)))
        ms, me, es = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ref = C.c_char_p()
        nref, nrec = C.c_size_t(), C.c_size_t()
        L.tfbs_synth_region_info(self.h, C.byref(ms), C.byref(me), C.byref(es), C.byref(ref), C.byref(nref),
                                 C.byref(nrec))
        self.merged = (ms.value, me.value)
        self.ext_start = es.value
        self.ref = C.string_at(ref, nref.value).decode()
        self.records = []
        for i in range(nrec.value):
            pos = C.c_uint64()
            r, a = C.c_char_p(), C.c_char_p()
            car = C.POINTER(C.c_uint32)()
            n = C.c_size_t()
            L.tfbs_synth_region_record(self.h, i, C.byref(pos), C.byref(r), C.byref(a), C.byref(car), C.byref(n))
            self.records.append((pos.value, r.value.decode(), a.value.decode(), list(car[:n.value])))
        L.tfbs_synth_region_destroy(self.h)
        self.h = None


def synth_write_pwms(directory, n_pwms, length_config, seed):
    p = C.c_void_p()
    check(lib().tfbs_synth_write_pwms(_u(directory), n_pwms, length_config, seed, C.byref(p)))
    try:
        names = C.string_at(p).decode().split(",")
    finally:
        lib().tfbs_free(p)
    return names


def range_overlaps(a, b):
    """range.rs:18-21: asymmetric -- are b's endpoints inside a?"""
    return a[0] <= b[0] <= a[1] or a[0] <= b[1] <= a[1]


def select_inner_peaks(merged, beds):
    """main.rs:62-72: [(bed index, start, end)] of every bed range p with p.overlaps(merged)."""
    out = []
    for bi, (_, ranges) in enumerate(beds):
        for (s, e) in ranges:
            if range_overlaps((s, e), merged):
                out.append((bi, s, e))
    return out


def run(chromosome, bcf, bed_files, reference_genome_file, wanted_samples, pwm_file, pwm_threshold_directory,
        pwm_threshold, wanted_pwms, output_file, forward_only=False, run_tabix=False, min_maf=0, threads=1,
        after_position=0, verbose=False, device=0, regions_per_batch=0, devices=None, dipwm_file=None,
        hits_output=None, hits_mode="diff", best_output=None, best_mode="diff", effects_output=None,
        effects_mode="sites", scores_output=None, scores_min_spread=1, pwm_pvalue=None, mutscan_output=None,
        mutscan_kinds=0, affinity_output=None, affinity_mode="diff", affinity_rows_output=None,
        affinity_rows_min_spread=1):
    """main.rs:234-393 `run` with the reference's argument order; writes the BGZF VCF.
    devices: list of HIP devices; batch g of merged regions runs on devices[g % n] (same
    text for any list; a device may repeat).  hits_output: also write every region's hit
    list there as BGZF TSV (HITS_HEADER, then RegionBatch.hits_tsv's lines in hits_mode "all"
    or "diff"); best_output: the same for every region's best sites (BEST_HEADER, then
    RegionBatch.best_tsv's lines in best_mode); effects_output: the same for every region's variant
    effects (EFFECTS_HEADER, then RegionBatch.effects_tsv's lines in effects_mode "sites" or "all");
    scores_output: also write the score rows (RegionBatch.score_rows with min_maf and
    scores_min_spread, POS from 1) there as a second BGZF VCF under the main output's #CHROM line;
    the main output does not change.  pwm_pvalue: the patterns load as parse_pwm_files(pvalue=...)
    loads them, on the run's first device; pwm_threshold_directory may then be None.  mutscan_output:
    also write every region's mutation scan there as BGZF TSV (MUTSCAN_HEADER, then
    RegionBatch.mutscan_tsv's lines for the kinds of mutscan_kinds: a mask of MUT_* or names; 0 means
    gain and loss).  affinity_output: also write every region's binding affinities there as BGZF TSV
    (AFFINITY_HEADER, then RegionBatch.affinity_tsv's lines in affinity_mode "all" or "diff").
    affinity_rows_output: also write the affinity rows (RegionBatch.affinity_rows with min_maf and
    affinity_rows_min_spread, POS from 1) there as a further BGZF VCF under the main output's #CHROM
    line."""
    a = _capi.tfbs_run_args()
    keep = [_u(x) if x is not None else None for x in (chromosome, bcf, ",".join(bed_files), reference_genome_file,
                                                        wanted_samples, pwm_file, pwm_threshold_directory,
                                                        ",".join(wanted_pwms), output_file)]
    (a.chromosome, a.bcf, a.bed_files, a.reference, a.samples_file, a.pwm_file, a.pwm_threshold_dir, a.pwm_names,
     a.output) = keep
    a.pwm_threshold = pwm_threshold
    a.forward_only = 1 if forward_only else 0
    a.min_maf = min_maf
    a.threads = threads
    a.after_position = after_position
    a.tabix = 1 if run_tabix else 0
    a.verbose = 1 if verbose else 0
    a.device = device
    a.regions_per_batch = regions_per_batch
    dev = _u(",".join(str(int(d)) for d in devices)) if devices else None
    a.devices = dev
    di = _u(dipwm_file) if dipwm_file is not None else None
    a.dipwm_file = di
    ho = _u(hits_output) if hits_output is not None else None
    a.hits_output = ho
    a.hits_mode = HITS_MODES[hits_mode]
    bo = _u(best_output) if best_output is not None else None
    a.best_output = bo
    a.best_mode = BEST_MODES[best_mode]
    # the full tfbs_run_ext layout whatever is asked for (the shorter ones of _capi serve older callers)
    x = _capi.tfbs_run_ext_affinity_rows()
    x.size = C.sizeof(x)
    opt = [_u(v) if v is not None else None for v in (effects_output, scores_output, mutscan_output, affinity_output,
                                                      affinity_rows_output)]
    x.effects_output, x.scores_output, x.mutscan_output, x.affinity_output, x.affinity_rows_output = opt
    x.effects_mode = EFFECT_MODES[effects_mode]
    x.scores_min_spread = scores_min_spread
    x.pwm_pvalue = pwm_pvalue or 0.0
    x.mutscan_kinds = mutscan_kinds_mask(mutscan_kinds)
    x.affinity_mode = AFFINITY_MODES[affinity_mode]
    x.affinity_rows_min_spread = affinity_rows_min_spread
    check(lib().tfbs_run_ex(C.byref(a), C.byref(x)))


class BcfReader:
    """Streaming BCF2 reader (f2): IndexedReader::from_path + fetch + records (raw GT).
    fetch() with nondecreasing beg on one contig reads the file once."""

    def __init__(self, path):
        self.h = C.c_void_p()
        check(lib().tfbs_bcf_open(_u(path), C.byref(self.h)))
        n = lib().tfbs_bcf_num_samples(self.h)
        self.samples = [lib().tfbs_bcf_sample_name(self.h, i).decode() for i in range(n)]
        self.selected = list(range(n))
        self.indexed = bool(lib().tfbs_bcf_indexed(self.h))

    def select(self, idx):
        """Decode GT only for these sample indices, in this order."""
        idx = [int(i) for i in idx]
        arr = (C.c_size_t * max(1, len(idx)))(*idx)
        check(lib().tfbs_bcf_select(self.h, arr, len(idx)))
        self.selected = idx

    def set_carriers_mode(self, on=True):
        """Records keep load_diffs' carrier ids (and the ploidy check) instead of raw GT."""
        check(lib().tfbs_bcf_set_carriers_mode(self.h, 1 if on else 0))
        self.carriers_mode = bool(on)

    def __del__(self):
        if getattr(self, "h", None):
            lib().tfbs_bcf_close(self.h)
            self.h = None

    def fetch(self, chrom, beg, end):
        n = C.c_size_t()
        check(lib().tfbs_bcf_fetch(self.h, _u(chrom), beg, end, C.byref(n)))
        out = []
        ns = len(self.selected)
        for i in range(n.value):
            pos, rlen, na = C.c_uint64(), C.c_uint32(), C.c_uint32()
            ref, alt = C.c_char_p(), C.c_char_p()
            gt = _capi.i32p()
            check(lib().tfbs_bcf_record(self.h, i, C.byref(pos), C.byref(rlen), C.byref(na), C.byref(ref),
                                        C.byref(alt), C.byref(gt)))
            rec = {"pos0": pos.value, "rlen": rlen.value, "n_alleles": na.value, "ref": ref.value.decode(),
                   "alt": alt.value.decode() if alt.value is not None else None}
            if getattr(self, "carriers_mode", False):
                ids, nc, st = _capi.u32p(), C.c_size_t(), C.c_int()
                check(lib().tfbs_bcf_record_carriers(self.h, i, C.byref(ids), C.byref(nc), C.byref(st)))
                rec["carriers"] = [ids[k] for k in range(nc.value)]
                rec["gt_status"] = st.value
            else:
                rec["gt"] = [[gt[2 * s], gt[2 * s + 1]] for s in range(ns)]
            out.append(rec)
        return out


def fasta_fetch(path, chrom, start, stop):
    p = C.c_void_p()
    n = C.c_size_t()
    check(lib().tfbs_fasta_fetch(_u(path), _u(chrom), start, stop, C.byref(p), C.byref(n)))
    try:
        return C.string_at(p, n.value).decode()
    finally:
        lib().tfbs_free(p)


def bgzf_write(path, text, flushes=0):
    b = _u(text)
    check(lib().tfbs_bgzf_write_file(_u(path), b, len(b), flushes))


def bgzf_read(path):
    p = C.c_void_p()
    n = C.c_size_t()
    check(lib().tfbs_bgzf_read_file(_u(path), C.byref(p), C.byref(n)))
    try:
        return C.string_at(p, n.value).decode()
    finally:
        lib().tfbs_free(p)


def merge_ranges(ranges):
    n = len(ranges)
    os_, oe = (C.c_uint64 * max(1, n))(), (C.c_uint64 * max(1, n))()
    m = C.c_size_t()
    check(lib().tfbs_merge_ranges((C.c_uint64 * max(1, n))(*[r[0] for r in ranges]),
                                  (C.c_uint64 * max(1, n))(*[r[1] for r in ranges]), n, os_, oe, C.byref(m)))
    return [(os_[i], oe[i]) for i in range(m.value)]
