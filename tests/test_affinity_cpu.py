"""Host side of the binding affinity, no GPU: the weight a(d) against 80-digit decimals on all of
[0, 30000) and far beyond, the committed tables against their generator, the pattern_ids'
reference scores, tfbs_batch_affinity_tsv and affinity_by_sample against affinity_ref on
hand-made records of a batch built on the host, the record's layout and the command line's help.
Integer work and text: every comparison is exact."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess
from decimal import ROUND_FLOOR, Context, Decimal

import numpy as np
import pytest

import affinity_ref as A
import best_ref as R
import dinuc_cases as K
import hits_ref as H
from helpers import TD, T

CHROM = "7"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def generator():
    spec = importlib.util.spec_from_file_location("gen_affinity_tables", os.path.join(ROOT, "tools", "gen_affinity_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ the weight
def test_weight_equals_the_definition_everywhere():
    got = [T.affinity_weight(d) for d in range(30000)]
    bad = [d for d in range(30000) if got[d] != A.weight_exact(d)]
    assert bad == []
    assert got[0] == 1 << 40 and got[27725] == 1 and got[27726] == 0
    assert all(got[d + 1] <= got[d] for d in range(29999))
    assert got[1] < got[0] and sum(1 for x in got if x) == 27726
    for d in (1 << 31, (1 << 32) - 1, 1 << 40, (1 << 64) - 1):
        assert T.affinity_weight(d) == A.weight(d) == 0


def test_committed_tables_are_the_generators():
    G = generator()
    text = open(G.HEADER).read()
    assert text == G.render()
    vals = [int(x, 16) for x in re.findall(r"0x([0-9A-F]{16})ull", text)]
    assert len(vals) == 1028
    ctx = Context(prec=80)  # (recomputed here, not through the generator)
    fl = lambda x: int(ctx.multiply(Decimal(1 << 63), ctx.exp(x)).to_integral_value(ROUND_FLOOR, context=ctx))
    assert vals[:1000] == [fl(ctx.divide(Decimal(-r), Decimal(1000))) for r in range(1000)]
    assert vals[1000:] == [fl(Decimal(-q)) for q in range(28)]
    t1, t2 = vals[:1000], vals[1000:]
    assert all(G.weight(d, t1, t2) == A.weight_exact(d) for d in (0, 1, 999, 1000, 21722, 27725, 27726))


# ------------------------------------------------------------------ the reference scores
def tops_of(pats):
    got = T.PatternSet.from_patterns(pats).affinity_tops()
    assert got == A.tops(pats)
    return got


def test_tops():
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    assert len(ps) == 2 and ps.affinity_tops() == [4000, 4000]  # the reference's test PWM, both strands
    W = lambda *cols: [T.Weight(*c) for c in cols]
    # an all-negative column adds 0; a column's best base counts whatever the others are
    assert tops_of([T.Pattern.PWM(W([5, -3, 2, 0], [-7, -1, -2, -9], [0, 0, 0, 0], [-4, 11, 3, 2]), "m", 0, 0)]) == [16]
    # a dinucleotide strand: per row the best of 16, a negative row adds 0
    rows = [[-5] * 16, list(range(-8, 8)), [3] * 15 + [40]]
    assert tops_of([T.Pattern.DiPWM(rows, "d", 0, 0)]) == [7 + 40]
    # an id whose strands have different sums takes the larger, for both; other ids keep theirs; OtherPattern: 0
    pats = [T.Pattern.PWM(W([10, 0, 0, 0], [0, 20, 0, 0]), "a", 3, 0, T.DIR_P),
            T.Pattern.OtherPattern("o", 5),
            T.Pattern.PWM(W([1, 2, 3, 4]), "b", 4, 0, T.DIR_P),
            T.Pattern.PWM(W([0, 0, 50, 0], [-1, -1, -1, -1], [0, 0, 0, 7]), "a", 3, 0, T.DIR_N)]
    assert tops_of(pats) == [57, 0, 4, 57]
    assert T.PatternSet.from_patterns([T.Pattern.OtherPattern("o", 0)]).affinity_tops() == [0]
    # the largest sums that cannot wrap pass; one more is refused
    edge = [T.Pattern.PWM(W([K.INT32_MAX - 5, 0, 0, 0], [0, -5, 0, 0]), "edge", 0, 0)]
    assert tops_of(edge) == [K.INT32_MAX - 5]
    over = [T.Pattern.PWM(W([K.INT32_MAX - 5, 0, 0, 0], [0, -6, 0, 0]), "over", 0, 0, T.DIR_N)]
    with pytest.raises(T.TfbsError) as ei:
        T.PatternSet.from_patterns(over).affinity_tops()
    assert ei.value.code == -1 and "the scores of strand 'over' (-) can wrap int32" in str(ei.value)
    with pytest.raises(ValueError):
        A.tops(over)


def test_tops_refuse_case_wrap_and_name_the_strand():
    pats = K.case_wrap()["pats"]
    cols = lambda p: sum(max(abs(min(r)), abs(max(r))) for r in p.weights)
    first = next(p for p in pats if cols(p) > K.INT32_MAX)
    with pytest.raises(T.TfbsError) as ei:
        T.PatternSet.from_patterns(pats).affinity_tops()
    assert ei.value.code == -1  # TFBS_E_ARG
    assert "the scores of strand '%s' (+) can wrap int32" % first.name in str(ei.value)
    with pytest.raises(ValueError) as ev:
        A.tops(pats)
    assert "'%s'" % first.name in str(ev.value)


# ------------------------------------------------------------------ the TSV and the fold by sample
@functools.lru_cache(None)
def small():
    """case_reduction's dinucleotide set (four pattern_ids of two strands) on its two regions;
    region 1's a.bed lists one range twice, and this batch hands region 1 an empty inner range
    (end < start) on top.  Built on the host once, never modified."""
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
    recs = A.expected(pats, regions, beds, order)
    return case, pats, b, regions, beds, order, recs


def baseline(order, seqs):
    ids = H.carrier_ids(seqs)
    return min(range(len(order)), key=lambda h: (-len(ids[order[h]]), ids[order[h]][0]))


def doctored():
    """The model's records rewritten by hand:
    region 0: every haplotype gets haplotype 0's records (nothing differs: `hap` lines only);
    region 1, range 0, pattern_id A: the baseline's strands lose their windows (a "none" baseline);
    pattern_id B: one haplotype's two strands swap their sums and counts (a tie: the same A and N);
    pattern_id C: one haplotype's first strand holds 7 less than the baseline's (a negative delta),
    its second strand the baseline's; pattern_id D: one haplotype is "none"."""
    case, pats, b, regions, beds, order, recs = small()
    pids = sorted({p.pattern_id for p in pats})
    Ap, Bp, Cp, Dp = pids[:4]
    base = baseline(order[1], case["seqs"][1])
    other = next(h for h in range(len(order[1])) if h != base)
    per = {x[:4]: x for x in recs}
    strands = {pid: [pi for pi, p in enumerate(pats) if p.pattern_id == pid] for pid in pids}
    assert all(len(s) == 2 for s in strands.values())
    out = []
    for x in recs:
        r, h, pi, k = x[:4]
        pid = pats[pi].pattern_id
        if r == 0:
            x = (r, h, pi, k) + per[(0, 0, pi, k)][4:]
        elif k == 0:
            s0, s1 = strands[pid]
            if pid == Ap and h == base:
                x = (r, h, pi, k, 0, 0, 0)
            elif pid == Bp and h == other:
                x = (r, h, pi, k) + per[(r, base, s1 if pi == s0 else s0, k)][4:]
            elif pid == Cp and h == other:
                bx = per[(r, base, pi, k)]
                assert bx[6] > 7
                x = (r, h, pi, k, bx[4], bx[5], bx[6] - 7 if pi == s0 else bx[6])
            elif pid == Dp and h == other:
                x = (r, h, pi, k, 0, 0, 0)
        out.append(x)
    return out, (Ap, Bp, Cp, Dp), base, other


@pytest.mark.parametrize("mode", ["all", "diff"])
def test_tsv_against_the_restatement(mode):
    case, pats, b, regions, beds, order, _ = small()
    recs, (Ap, Bp, Cp, Dp), base, other = doctored()
    want = A.format_tsv(CHROM, pats, regions, beds, order, case["seqs"], recs, mode)
    got = b.affinity_tsv(A.as_array(recs), CHROM, mode)
    assert got == want
    assert b.affinity_tsv(A.as_array(recs), CHROM, mode, header=True) == T.AFFINITY_HEADER + want
    assert T.AFFINITY_HEADER == A.HEADER and T.AFFINITY_HEADER.count("\t") == 14
    rows = [l.split("\t") for l in got.splitlines()]
    assert all(len(l) == 15 for l in rows) and len(rows) > 50
    name = lambda reg: "%d-%d" % reg["merged"]
    r0 = [l for l in rows if l[1] == name(regions[0])]
    r1 = [l for l in rows if l[1] == name(regions[1])]
    rng0 = R.region_ranges(regions[1], beds)[0]
    cell = lambda pid, kind=None: [l for l in r1 if l[2] != "." and (int(l[3]), int(l[4])) == rng0 and
                                   l[6] == str(pid) and (kind is None or l[9] == kind)]
    tops = dict(zip((p.pattern_id for p in pats), A.tops(pats)))
    assert not any(l[3] != "." and int(l[4]) < int(l[3]) for l in rows)  # the empty inner range writes nothing
    assert all(l[10] == str(tops[int(l[6])]) for l in rows if l[9] != "hap")
    if mode == "all":
        assert {l[9] for l in rows} == {"aff"} and all(l[13] == "." and l[14] == "." for l in rows)
        keys0 = {(a, z, bi) for bi, a, z in regions[0]["inner"] if z >= a}  # each once whatever its multiplicity
        assert len(r0) == len(order[0]) * len(tops) * len(keys0)
        none = [l for l in cell(Ap) if l[7] == str(base)] + [l for l in cell(Dp) if l[7] == str(other)]
        assert none and all(l[11:13] == [".", "."] for l in none)
        tie = {l[7]: l[11:13] for l in cell(Bp) if l[2] == cell(Bp)[0][2]}
        assert tie[str(other)] == tie[str(base)] and tie[str(base)][0] != "."
    else:
        # region 0: nothing differs, only `hap` lines
        assert len(r0) == len(order[0]) and {l[9] for l in r0} == {"hap"}
        assert all(l[2:7] == ["."] * 5 and l[10:14] == ["."] * 4 for l in r0)
        assert [l[14] for l in r1 if l[9] == "hap" and l[7] == str(base)] == ["*"]
        assert {l[9] for l in r1} == {"hap", "base", "alt"}
        bl = cell(Ap, "base")
        assert bl and all(l[11:14] == ["."] * 3 for l in bl)  # a "none" baseline
        assert cell(Ap, "alt") and all(l[13] == "." and l[12] != "." for l in cell(Ap, "alt"))
        assert not [l for l in cell(Bp) if l[7] == str(other)]  # the tie: no line for it
        neg = [l for l in cell(Cp, "alt") if l[7] == str(other)]
        assert neg and all(l[13] == "-7" for l in neg)  # a negative delta
        gone = [l for l in cell(Dp, "alt") if l[7] == str(other)]
        assert gone and all(l[11:14] == ["."] * 3 for l in gone)  # a "none" alternative
        nums = [int(l[13]) for l in rows if l[9] == "alt" and l[13] != "."]
        assert any(x > 0 for x in nums) and any(x < 0 for x in nums)


def test_tsv_one_region_at_a_time_and_refusals():
    case, pats, b, regions, beds, order, recs = small()
    a = A.as_array(recs)
    for mode in ("all", "diff"):
        parts = [b.affinity_tsv(a[a["region"] == r], CHROM, mode) for r in range(b.num_regions)]
        assert all(parts) and "".join(parts) == b.affinity_tsv(a, CHROM, mode)
    assert b.affinity_tsv(a[:0], CHROM, "diff") == ""
    with pytest.raises(T.TfbsError):
        b.affinity_tsv(a[:-1], CHROM, "all")
    swapped = a.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(T.TfbsError):
        b.affinity_tsv(swapped, CHROM, "all")
    foreign = a[a["region"] == 1].copy()
    foreign["region"] = b.num_regions
    with pytest.raises(T.TfbsError):
        b.affinity_tsv(foreign, CHROM, "diff")
    p, n = C.c_void_p(), C.c_size_t()
    assert T.lib().tfbs_batch_affinity_tsv(b.h, a.ctypes.data_as(C.c_void_p), len(a), b"7", 2, C.byref(p),
                                           C.byref(n)) == -1  # TFBS_E_ARG


def test_sums_near_2_63_and_their_delta():
    """A folded sum just below 2^63 prints in full, and a delta is a signed 64-bit difference."""
    case, pats, b, regions, beds, order, recs = small()
    base = baseline(order[1], case["seqs"][1])
    big = (1 << 62) - 1
    a = A.as_array([x[:4] + ((1, 1, big) if x[0] == 1 and x[1] == base else (1, 0, 0)) for x in recs])
    rows = [l.split("\t") for l in b.affinity_tsv(a[a["region"] == 1], CHROM, "diff").splitlines()]
    assert {l[12] for l in rows if l[9] == "base"} == {str(2 * big)}
    assert {l[13] for l in rows if l[9] == "alt"} == {str(-2 * big)} and {l[12] for l in rows if l[9] == "alt"} == {"0"}


def test_by_sample():
    case, pats, b, regions, beds, order, recs = small()
    a = A.as_array(recs)
    tp = A.tops(pats)
    for r, reg in enumerate(regions):
        sums, counts = b.affinity_by_sample(a, r)
        ranges = R.region_ranges(reg, beds)
        assert sums.shape == counts.shape == (2 * case["n"], len(pats), len(ranges))
        assert sums.dtype == np.uint64 and counts.dtype == np.uint32
        for x, (codes, pos) in enumerate(case["seqs"][r]):
            for pi, p in enumerate(pats):
                for k in (0, len(ranges) - 1):
                    nw, _, s = A.record_of(p, tp[pi], codes, pos, ranges[k])
                    assert (int(sums[x, pi, k]), int(counts[x, pi, k])) == (s, nw), (r, x, pi, k)
    with pytest.raises(ValueError):
        b.affinity_by_sample(a[1:], 0)


def test_record_layout_and_help():
    st = T._capi.tfbs_affinity
    assert C.sizeof(st) == 32
    dt = np.dtype(T.AFFINITY_DTYPE)
    assert dt.itemsize == 32 and [n for n, _ in st._fields_] == list(dt.names)
    for name, _ in st._fields_:
        assert getattr(st, name).offset == dt.fields[name][1] and getattr(st, name).size == dt.fields[name][0].itemsize
    assert T.AFFINITY_MODES == {"all": 0, "diff": 1}
    ext = [n for n, _ in T._capi.tfbs_run_ext_affinity._fields_]
    assert ext[-2:] == ["affinity_output", "affinity_mode"] and ext[:-2] == [n for n, _ in T._capi.tfbs_run_ext_mutscan._fields_]
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--affinity_output" in r.stderr and "--affinity_mode" in r.stderr
    r = subprocess.run([exe, "--affinity_mode", "some"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--affinity_mode is all or diff" in r.stderr
