"""Host side of the best sites, no GPU: tfbs_batch_best_tsv against best_ref.format_tsv on
hand-made records (best_ref's, some of them doctored so that every rule of the text is met),
the regions' distinct ranges, the record's layout and the command line's help.  Integer work
and text: every comparison is exact."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import best_ref as R
import dinuc_cases as K
import hits_ref as H
from helpers import T, build_batch

CHROM = "7"


@functools.lru_cache(None)
def small():
    """case_reduction's dinucleotide set (four pattern_ids of two strands) on its two regions:
    region 1's a.bed lists one range twice, and this batch hands region 1 an empty inner range
    (end < start) on top.  Built once, never modified."""
    case = K.case_reduction()
    pats = case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    beds = case["beds"]
    regions = []
    for k, reg in enumerate(case["regions"]):
        reg = dict(reg)
        reg["inner"] = T.select_inner_peaks(reg["merged"], beds)
        if k == 1:
            reg["inner"] = reg["inner"] + [(1, reg["merged"][0] + 9, reg["merged"][0] + 8)]
        regions.append(reg)
    b = T.RegionBatch(ps, case["n"])
    for name, _ in beds:
        b.add_bed(name)
    for reg in regions:
        b.begin(reg["merged"][0], reg["merged"][1], reg["ref"])
        for bi, a, z in reg["inner"]:
            b.add_inner(bi, a, z)
        for rec in reg["records"]:
            b.add_record_carriers(rec[1], rec[2], rec[3], rec[4])
        b.end()
    order = [H.library_order(b, r) for r in range(b.num_regions)]
    recs = R.expected_best(pats, regions, beds, order)
    return case, pats, b, regions, beds, order, recs


def baseline(order, seqs):
    ids = H.carrier_ids(seqs)
    return min(range(len(order)), key=lambda h: (-len(ids[order[h]]), ids[order[h]][0]))


def doctored():
    """The records with three (region 1, range 0) cells rewritten by hand:
    pattern_id A: every haplotype gets haplotype 0's records (nothing differs);
    pattern_id B: the baseline's strands lose their windows (a "none" baseline);
    pattern_id C: on one haplotype both strands score the same, above everything else (a tie)."""
    case, pats, b, regions, beds, order, recs = small()
    pids = sorted({p.pattern_id for p in pats})
    A, Bp, Cp = pids[0], pids[1], pids[2]
    base = baseline(order[1], case["seqs"][1])
    tied = next(h for h in range(len(order[1])) if h != base)
    first = {}
    out = []
    for x in recs:
        r, h, pi, k = x[:4]
        pid = pats[pi].pattern_id
        if r == 1 and k == 0:
            if pid == A:
                x = (r, h, pi, k) + first.setdefault(pi, x[4:])
            elif pid == Bp and h == base:
                x = (r, h, pi, k, R.UINT32_MAX, 0, R.INT32_MIN, 0, 0)
            elif pid == Cp and h == tied:
                x = x[:5] + (max(1, x[5]), K.INT32_MAX) + x[7:]
        out.append(x)
    return out, (A, Bp, Cp), base, tied


@pytest.mark.parametrize("mode", ["all", "diff"])
def test_tsv_against_the_restatement(mode):
    case, pats, b, regions, beds, order, _ = small()
    recs, (A, Bp, Cp), base, tied = doctored()
    seqs = case["seqs"]
    want = R.format_tsv(CHROM, pats, regions, beds, order, seqs, recs, mode)
    got = b.best_tsv(R.as_array(recs), CHROM, mode)
    assert got == want
    assert b.best_tsv(R.as_array(recs), CHROM, mode, header=True) == T.BEST_HEADER + want
    assert T.BEST_HEADER == R.HEADER and T.BEST_HEADER.count("\t") == 15
    rows = [l.split("\t") for l in got.splitlines()]
    assert all(len(l) == 16 for l in rows) and len(rows) > 100
    s1, e1 = regions[1]["merged"]
    r1 = [l for l in rows if l[1] == "%d-%d" % (s1, e1)]
    rng0 = R.region_ranges(regions[1], beds)[0]
    cell = lambda pid, kind=None: [l for l in r1 if l[2] != "." and (int(l[3]), int(l[4])) == rng0 and
                                   l[6] == str(pid) and (kind is None or l[9] == kind)]
    # the empty inner range writes nothing; the range a.bed lists twice is written once per line
    assert not any(l[3] != "." and int(l[4]) < int(l[3]) for l in rows)
    twice = [(a, z) for bi, a, z in regions[1]["inner"] if bi == 0]
    assert len(twice) == 2 and twice[0] == twice[1] == (s1, e1)
    n_hap = len(order[1])
    if mode == "all":
        assert {l[9] for l in rows} == {"best"}
        for pid in (A, Bp, Cp):
            keyed = [l for l in r1 if l[2] == "a.bed" and (int(l[3]), int(l[4])) == (s1, e1) and l[6] == str(pid)]
            assert len(keyed) == n_hap
        assert [l[10:14] for l in cell(Bp) if l[7] == str(base)] == [["."] * 4] * len({l[2] for l in cell(Bp)})
        assert all(l[14] == "." and l[15] == "." for l in rows)
    else:
        kinds = {l[9] for l in rows}
        assert kinds == {"hap", "base", "alt"}
        haps = [l for l in r1 if l[9] == "hap"]
        assert len(haps) == n_hap and all(l[2:7] == ["."] * 5 and l[10:15] == ["."] * 5 for l in haps)
        assert [l[15] for l in haps if l[7] == str(base)] == ["*"]
        assert cell(A) == []  # nothing differs: no line
        bl = cell(Bp, "base")
        assert bl and all(l[10:15] == ["."] * 5 for l in bl)  # a "none" baseline
        alts = cell(Bp, "alt")
        assert alts and all(l[14] == "." and l[13] != "." for l in alts)
        # somewhere a delta is a number, and it is the two scores' difference
        nums = [l for l in rows if l[9] == "alt" and l[14] != "."]
        assert nums and all(int(l[14]) != 0 for l in nums)
    # the tie: both strands of pattern_id C hold INT32_MAX there; the strand created first wins
    mine = [l for l in cell(Cp) if l[7] == str(tied) and l[9] in ("best", "alt")]
    strands = [pi for pi, p in enumerate(pats) if p.pattern_id == Cp]
    assert len(strands) == 2 and mine
    first = next(x for x in recs if x[:4] == (1, tied, strands[0], 0))
    for l in mine:
        assert l[13] == str(K.INT32_MAX) and l[10] == ("-" if pats[strands[0]].direction == T.DIR_N else "+")
        assert (int(l[11]), int(l[12])) == (first[7], first[8])


def test_tsv_one_region_at_a_time_and_refusals():
    """The text of whole regions is the concatenation of the regions' texts; a partial region, an
    unsorted block, a foreign region and an unknown mode are refused."""
    case, pats, b, regions, beds, order, recs = small()
    a = R.as_array(recs)
    for mode in ("all", "diff"):
        parts = [b.best_tsv(a[a["region"] == r], CHROM, mode) for r in range(b.num_regions)]
        assert all(parts) and "".join(parts) == b.best_tsv(a, CHROM, mode)
    assert b.best_tsv(a[:0], CHROM, "diff") == ""
    with pytest.raises(T.TfbsError):
        b.best_tsv(a[:-1], CHROM, "all")
    swapped = a.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(T.TfbsError):
        b.best_tsv(swapped, CHROM, "all")
    foreign = a[a["region"] == 1].copy()
    foreign["region"] = b.num_regions
    with pytest.raises(T.TfbsError):
        b.best_tsv(foreign, CHROM, "diff")
    p, n = C.c_void_p(), C.c_size_t()
    assert T.lib().tfbs_batch_best_tsv(b.h, a.ctypes.data_as(C.c_void_p), len(a), b"7", 2, C.byref(p),
                                       C.byref(n)) == -1  # TFBS_E_ARG


@pytest.mark.parametrize("name", ["case_reduction", "case_all_kernels", "case_geometry"])
def test_ranges_ascend_and_match_select_inner_peaks(name):
    case = getattr(K, name)()
    ps = T.PatternSet.from_patterns(sorted(case.get("mono", []) + case["pats"], key=lambda p: p.pattern_id))
    b = build_batch(ps, case["n"], case["beds"], case["regions"])
    several = 0
    for r, reg in enumerate(case["regions"]):
        got = b.ranges(r)
        assert got == sorted(set(got)) and all(z >= a for a, z in got)
        assert got == sorted({(a, z) for _, a, z in T.select_inner_peaks(reg["merged"], case["beds"]) if z >= a})
        several += len(got) > 1
    assert several
    with pytest.raises(T.TfbsError):
        b.ranges(b.num_regions)
    s, e = C.c_uint64(), C.c_uint64()
    assert T.lib().tfbs_batch_region_range(b.h, 0, len(b.ranges(0)), C.byref(s), C.byref(e)) == -1  # TFBS_E_ARG
    _, _, bb, regions, beds, _, _ = small()  # the empty inner range is no range
    assert bb.ranges(1) == R.region_ranges(regions[1], beds) and len(regions[1]["inner"]) > len(bb.ranges(1)) + 1


def test_record_layout():
    """sizeof(tfbs_best) == 48 through ctypes; the numpy dtype has the same offsets."""
    st = T._capi.tfbs_best
    assert C.sizeof(st) == 48
    dt = np.dtype(T.BEST_DTYPE)
    assert dt.itemsize == 48
    assert [n for n, _ in st._fields_] == list(dt.names)
    for name, _ in st._fields_:
        assert getattr(st, name).offset == dt.fields[name][1], name
        assert getattr(st, name).size == dt.fields[name][0].itemsize, name
    assert T.BEST_MODES == {"all": 0, "diff": 1}
    args = T._capi.tfbs_run_args
    names = [n for n, _ in args._fields_]
    assert names[-4:] == ["hits_output", "hits_mode", "best_output", "best_mode"]


def test_help_names_the_flags():
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--best_output" in r.stderr and "--best_mode" in r.stderr
