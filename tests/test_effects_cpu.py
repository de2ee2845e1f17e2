"""Host side of the variant effects, no GPU: the kept records (tfbs_batch_keep_variants,
tfbs_batch_region_variant) on the host build paths, the four statuses, the untouched batch without
them, the record's layout, tfbs_run_ext, the command line's help and tfbs_batch_effects_tsv against
effects_ref.format_tsv on hand-made records.  Integer work and text: every comparison is exact."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import dinuc_cases as K
import effects_ref as E
from helpers import T, build_batch

CHROM = "7"
E_ARG, E_STATE = -1, -14


def status_region():
    """One region of lmax 8 holding the four statuses: a scored SNV; a multi-allelic record; a
    record without carriers; a deletion and, inside it, a bad-REF SNV with the same carriers (the
    overlapping diff truncates the haplotype without a REF check, so the region builds; alone the
    SNV is refused)."""
    s, e = 5000, 5029
    lmax = 8
    es, ee = s + 1 - lmax, e + lmax - 1
    ref = ("ACGTTGCA" * 8)[:ee - es + 1]
    bad = "ACGT"[("ACGT".index(ref[22]) + 1) % 4]
    recs = [("car", es + 5, ref[5], "ACGT"[("ACGT".index(ref[5]) + 2) % 4], [0, 2]),
            ("gt", es + 9, 3, ref[9], "ACGT"[("ACGT".index(ref[9]) + 1) % 4], [(4, 5), (4, 5), (0, 2)]),
            ("car", es + 12, ref[12], "ACGT"[("ACGT".index(ref[12]) + 1) % 4], []),
            ("car", es + 20, ref[20:25], ref[20], [3]),
            ("car", es + 22, bad, "ACGT"[("ACGT".index(bad) + 1) % 4], [3])]
    return {"merged": (s, e), "ref": ref, "es": es, "ee": ee, "records": recs}, lmax


@functools.lru_cache(None)
def status_case():
    reg, lmax = status_region()
    w = [[(7 * i + 3 * j) % 11 - 4 for j in range(4)] for i in range(lmax)]
    pats = [T.Pattern.PWM([T.Weight(*x) for x in w], "m8", 0, 3),
            T.Pattern.PWM([T.Weight(*x) for x in w[:3]], "m3", 1, 2, T.DIR_N),
            T.Pattern.OtherPattern("other", 2)]
    return {"pats": pats, "n": 3, "regions": [reg], "beds": [("a.bed", [reg["merged"]])]}


def test_keep_variants_only_before_the_first_region():
    case = status_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    b = build_batch(ps, case["n"], case["beds"], case["regions"])
    with pytest.raises(T.TfbsError) as ei:
        b.keep_variants(True)
    assert ei.value.code == E_STATE
    with pytest.raises(T.TfbsError) as ei:  # and the kept records are not there
        b.variants(0)
    assert ei.value.code == E_STATE
    b2 = T.RegionBatch(ps, case["n"])
    b2.keep_variants(True)
    b2.keep_variants(False)
    b2.add_bed("a.bed")
    reg = case["regions"][0]
    b2.begin(reg["merged"][0], reg["merged"][1], reg["ref"])
    with pytest.raises(T.TfbsError) as ei:  # a region is open
        b2.keep_variants(True)
    assert ei.value.code == E_STATE


def test_the_four_statuses():
    case = status_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    reg = case["regions"][0]
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])  # the region builds
    got = b.variants(0)
    assert got == E.variants(reg)
    assert [v[5] for v in got] == [T.VAR_SCORED, T.VAR_MULTIALLELIC, T.VAR_NO_CARRIER, T.VAR_SCORED, T.VAR_UNPATCHED]
    assert (T.VAR_SCORED, T.VAR_MULTIALLELIC, T.VAR_NO_CARRIER, T.VAR_UNPATCHED) == (0, 1, 2, 3)
    assert [v[4] for v in got] == [2, 0, 0, 1, 1] and [v[3] for v in got] == [2, 3, 2, 2, 2]
    assert b.region_stats(0)[1] == 5
    # its count path is untouched: the same packed inputs as the batch that keeps nothing
    plain = build_batch(ps, case["n"], case["beds"], case["regions"])
    assert plain.input_digest(0) == b.input_digest(0)
    assert plain.region_stats(0) == b.region_stats(0)
    assert [plain.haplotype(0, h) for h in range(plain.region_stats(0)[0])] == \
           [b.haplotype(0, h) for h in range(b.region_stats(0)[0])]
    # a short capacity tells the need
    L = T.lib()
    nr, na = C.c_size_t(), C.c_size_t()
    rc = L.tfbs_batch_region_variant(b.h, 0, 3, None, None, None, 0, C.byref(nr), C.byref(na), None, None, None)
    assert rc == E_ARG and (nr.value, na.value) == (5, 1)
    for region, v in ((1, 0), (0, 5)):
        assert L.tfbs_batch_region_variant(b.h, region, v, None, None, None, 0, C.byref(nr), C.byref(na), None, None,
                                           None) == E_ARG


@pytest.mark.parametrize("name", ["case_all_kernels", "case_n_and_indels", "case_geometry"])
def test_variants_equal_the_records(name):
    case = getattr(K, name)()
    pats = sorted(case.get("mono", []) + case["pats"], key=lambda p: p.pattern_id)
    ps = T.PatternSet.from_patterns(pats)
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
    plain = build_batch(ps, case["n"], case["beds"], case["regions"])
    assert b.num_regions == len(case["regions"])
    for r, reg in enumerate(case["regions"]):
        got = b.variants(r)
        assert got == E.variants(reg) and len(got) == b.region_stats(r)[1] == len(reg["records"])
        assert [(v[0], v[1], v[2], v[4]) for v in got] == [(x[1], x[2], x[3], len(x[4])) for x in reg["records"]]
        assert plain.input_digest(r) == b.input_digest(r)


def test_variants_of_a_synthetic_fill(monkeypatch):
    """tfbs_synth_fill_batch: chunks built while the previous chunk commits (the build paths'
    other caller; without a device its regions take the grouping's host path)."""
    case = status_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    n, count = 30, 70  # more than one chunk of 64 regions per thread
    monkeypatch.setenv("TFBS_HOST_THREADS", "1")
    b = T.RegionBatch(ps, n, keep_variants=True)
    b.synth_fill(9, 0, count, 25)
    plain = T.RegionBatch(ps, n)
    plain.synth_fill(9, 0, count, 25)
    assert b.num_regions == count
    seen = set()
    for j in range(count):
        r = T.SynthRegion(9, j, n, ps.max_length, 25)
        es, ee = b.ext(*r.merged)
        reg = {"merged": r.merged, "ref": r.ref, "es": es, "ee": ee,
               "records": [("car", pos, ref, alt, car) for pos, ref, alt, car in r.records]}
        assert b.variants(j) == E.variants(reg)
        seen |= {v[5] for v in b.variants(j)}
        assert plain.input_digest(j) == b.input_digest(j)
    assert T.VAR_SCORED in seen


def test_record_layout():
    assert C.sizeof(T._capi.tfbs_effect) == 72
    dt = np.dtype(T.EFFECT_DTYPE)
    assert dt.itemsize == 72
    assert [n for n, _ in T._capi.tfbs_effect._fields_] == list(dt.names) == list(E.FIELDS)
    for name, _ in T._capi.tfbs_effect._fields_:
        assert dt.fields[name][1] == getattr(T._capi.tfbs_effect, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(T._capi.tfbs_effect, name).size, name
    assert dt.fields["ref_start"][1] == 40 and dt.fields["ref_score"][0] == np.dtype("<i4")
    assert [n for n, _ in T._capi.tfbs_run_ext._fields_] == ["size", "effects_output", "effects_mode"]
    assert T.EFFECT_MODES == {"sites": 0, "all": 1}
    # tfbs_run_args did not grow: its last field is still best_mode
    assert [n for n, _ in T._capi.tfbs_run_args._fields_][-4:] == ["hits_output", "hits_mode", "best_output",
                                                                   "best_mode"]
    hdr = open(os.path.join(os.path.dirname(T.__file__), "..", "include", "tfbs_amd.h")).read()
    assert '#define TFBS_EFFECTS_HEADER "%s"' % T.EFFECTS_HEADER.replace("\t", "\\t").replace("\n", "\\n") in hdr
    assert T.EFFECTS_HEADER == E.HEADER and T.EFFECTS_HEADER.count("\t") == 17


def test_help_names_the_effects_flags():
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--effects_output" in r.stderr and "--effects_mode sites|all" in r.stderr
    r = subprocess.run([exe, "--effects_mode", "some"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--effects_mode is sites or all" in r.stderr


def hand_made():
    """status_case's records by the reference, some of them doctored so that every kind and every
    "." field is met: (variant 0, strand 0) passes on both sides with equal scores (same), (0, 1)
    with different ones (change); (3, 0) only on alt (gain), (3, 1) only on ref (loss); a side
    without a window beside one that passes."""
    case = status_case()
    pats = case["pats"]
    rows, _ = E.expected_effects(pats, case["regions"])
    thr = [p.min_score for p in pats]
    out = []
    for x in rows:
        x = list(x)
        v, pi = x[1], x[2]
        if (v, pi) == (0, 0):
            x[5] = x[8] = thr[0] + 5
        elif (v, pi) == (0, 1):
            x[5], x[8] = thr[1] + 1, thr[1] + 1000
        elif (v, pi) == (3, 0):
            x[5], x[8] = E.INT32_MIN, 2 ** 31 - 1  # (a genuine INT32_MIN beside n_ref > 0; delta beyond int32)
        elif (v, pi) == (3, 1):
            x[5], x[8] = thr[1] + 7, thr[1] - 1
        out.append(tuple(x))
    return case, pats, out


@pytest.mark.parametrize("mode", ["sites", "all"])
def test_tsv_against_the_restatement(mode):
    case, pats, rows = hand_made()
    ps = T.PatternSet.from_patterns(pats)
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
    want = E.format_tsv(CHROM, pats, case["regions"], rows, mode)
    got = b.effects_tsv(E.as_array(rows), CHROM, mode)
    assert got == want
    assert b.effects_tsv(E.as_array(rows), CHROM, mode, header=True) == T.EFFECTS_HEADER + want
    lines = [l.split("\t") for l in got.splitlines()]
    assert all(len(l) == 18 for l in lines)
    var = [l for l in lines if l[7] == "var"]
    assert [l[8] for l in var] == ["scored", "multiallelic", "no_carrier", "scored", "unpatched"]
    assert all(l[9:] == ["."] * 9 and l[0] == CHROM and l[1] == "5000-5029" for l in var)
    assert [l[2] for l in var] == ["0", "1", "2", "3", "4"] and var[3][4:7] == [case["regions"][0]["ref"][20:25],
                                                                               case["regions"][0]["ref"][20], "1"]
    kinds = [l[7] for l in lines if l[7] != "var"]
    if mode == "sites":
        assert sorted(kinds) == ["change", "gain", "loss"]
    else:
        assert set(kinds) == {"change", "gain", "loss", "same"} or set(kinds) == {"change", "gain", "loss", "same",
                                                                                   "none"}
        assert "same" in kinds
    # no line for the TFBS_KIND_OTHER strand (no window on either side) nor under an unscored record
    assert not any(l[8] == "other" for l in lines)
    assert all(l[2] in ("0", "3") for l in lines if l[7] != "var")
    change = next(l for l in lines if l[7] == "change")
    assert int(change[17]) == int(change[16]) - int(change[13]) == 999
    gain = next(l for l in lines if l[7] == "gain")
    assert int(gain[17]) == 2 ** 32 - 1  # a signed 64-bit difference


def test_tsv_dot_fields_and_none():
    """A side without a window writes "." three times and "." for delta; `none` in mode all only."""
    case, pats, rows = hand_made()
    ps = T.PatternSet.from_patterns(pats)
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
    out = []
    for x in rows:
        x = list(x)
        if (x[1], x[2]) == (0, 0):  # no alt window, ref passes: a loss with "." fields
            x[7:10] = list(E.EMPTY_SIDE)
            x[12] = x[13] = 0
        if (x[1], x[2]) == (3, 1):  # neither side passes
            x[5] = x[8] = pats[1].min_score
        out.append(tuple(x))
    for mode in ("sites", "all"):
        got = b.effects_tsv(E.as_array(out), CHROM, mode)
        assert got == E.format_tsv(CHROM, pats, case["regions"], out, mode)
        lines = [l.split("\t") for l in got.splitlines()]
        loss = [l for l in lines if l[7] == "loss" and l[2] == "0"]
        assert len(loss) == 1 and loss[0][14:] == ["."] * 4 and "." not in loss[0][11:14]
        assert ("none" in [l[7] for l in lines]) == (mode == "all")


def test_tsv_and_effects_need_the_kept_variants():
    case, pats, rows = hand_made()
    ps = T.PatternSet.from_patterns(pats)
    plain = build_batch(ps, case["n"], case["beds"], case["regions"])
    with pytest.raises(T.TfbsError) as ei:
        plain.effects_tsv(E.as_array(rows), CHROM)
    assert ei.value.code == E_STATE
    L = T.lib()
    p, n = C.c_void_p(), C.c_size_t()
    assert L.tfbs_batch_effects(None, plain.h, 0, 1, C.byref(p), C.byref(n)) == E_ARG  # (no ctx without a device)
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
    with pytest.raises(T.TfbsError) as ei:  # not a whole region
        b.effects_tsv(E.as_array(rows[:-1]), CHROM)
    assert ei.value.code == E_ARG
    with pytest.raises(KeyError):
        b.effects_tsv(E.as_array(rows), CHROM, "diff")
    assert b.effects_tsv(E.as_array([]), CHROM) == ""
