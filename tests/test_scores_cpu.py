"""tfbs_scores_as_genotypes, the host-only definition of a score row (include/tfbs_amd.h, "Score
rows"), against its plain Python restatement (score_ref.py): every d of the small spreads, the
quartile boundaries, the half-even ties, t rounding to 0 and to 20000 away from the extremes,
the int32 limits, min_spread, the three maf branches and the buffer caps.  Integer work: every
comparison is exact."""
import ctypes as C
import random

import pytest

import score_ref as S
from helpers import T

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
HUGE = (1 << 33) - 2


def pairs_of(ds, spread):
    """left / right int32 values whose sums are lo + d for the given d, lo and lo + spread among
    them whatever ds holds (so that the spread is the one meant)."""
    ds = list(ds) + [0, spread]
    if spread <= INT32_MAX:
        base = random.Random(spread).randrange(INT32_MIN, INT32_MAX - spread + 1)
        return [base + d for d in ds], [-7] * len(ds)
    left = [INT32_MIN + min(d, (1 << 32) - 1) for d in ds]
    return left, [INT32_MIN + d - (l - INT32_MIN) for d, l in zip(ds, left)]


def both(left, right, min_spread=1):
    assert all(INT32_MIN <= v <= INT32_MAX for v in left + right)
    got, want = T.scores_as_genotypes(left, right, min_spread), S.genotypes(left, right, min_spread)
    assert got == want
    return got


@pytest.mark.parametrize("spread", [1, 2, 3, 4, 7, 8, 40000])
def test_every_d(spread):
    left, right = pairs_of(range(spread + 1), spread)
    maf, info, gts = both(left, right)
    fields = gts.split("\t")[1:]
    assert len(fields) == spread + 3
    assert fields[0] == "0|0:0.0" and fields[spread] == "1|1:2.0"
    assert info.startswith("SCORES=%d,%d;" % (left[0] + right[0], left[0] + right[0] + spread))
    if spread % 4 == 0:  # the quartile boundaries: 4 d == spread is `one`, 4 d == 3 spread is `two`
        q = spread // 4
        assert fields[q].startswith("0|1:") and fields[3 * q - 1].startswith("0|1:")
        assert fields[3 * q].startswith("1|1:") and (q == 1 or fields[q - 1].startswith("0|0:"))
    if spread == 40000:  # 20000 d / 40000 = d / 2: a tie at every odd d, down (to an even t) and up
        assert fields[1] == "0|0:0.0000" and fields[3] == "0|0:0.0002" and fields[5] == "0|0:0.0002"
        assert fields[39999] == "1|1:2.0000" and fields[39997] == "1|1:1.9998" and fields[39995] == "1|1:1.9998"
        assert fields[20001] == "0|1:1.0000" and fields[20003] == "0|1:1.0002"


def test_widest_spread():
    """Spread 2^33 - 2, from INT32_MIN + INT32_MIN to INT32_MAX + INT32_MAX.  Every d is out of
    reach (8.6e9 of them); these are the d at which the definition can go wrong there: the ends
    and their neighbours (t rounds to 0 and to 20000 away from the extremes), the quartile
    boundaries (4 d against spread and 3 spread, either side), the d on either side of the
    rounding boundaries (k + 1/2) spread / 20000 for k at the ends, in the middle and at random
    (20000 d reaches 2^48 there), the largest values of either operand, and random d.  No d is a
    half-even tie at this spread: 40000 d = (2 k + 1) spread has no solution, spread / 2 =
    2^32 - 1 being odd and 20000 even."""
    rnd = random.Random(33)
    ds = {0, 1, 2, 3, HUGE - 3, HUGE - 2, HUGE - 1, HUGE, (1 << 32) - 2, (1 << 32) - 1, 1 << 32}
    for num, den in ((1, 4), (1, 2), (3, 4)):
        c = HUGE * num // den
        ds |= {c - 2, c - 1, c, c + 1, c + 2}
    ks = {0, 1, 2, 9999, 10000, 19997, 19998, 19999} | {rnd.randrange(20000) for _ in range(200)}
    for k in ks:
        c = (2 * k + 1) * HUGE // 40000
        ds |= {c - 1, c, c + 1, c + 2}
    ds |= {rnd.randrange(HUGE + 1) for _ in range(2000)}
    ds = sorted(d for d in ds if 0 <= d <= HUGE)
    left, right = pairs_of(ds, HUGE)
    assert INT32_MIN in left and INT32_MAX in left and INT32_MIN in right and INT32_MAX in right
    maf, info, gts = both(left, right)
    fields = gts.split("\t")[1:]
    assert info.startswith("SCORES=%d,%d;" % (2 * INT32_MIN, 2 * INT32_MAX))
    assert fields[ds.index(1)] == "0|0:0.0000" and fields[ds.index(HUGE - 1)] == "1|1:2.0000"
    assert fields[ds.index(0)] == "0|0:0.0" and fields[ds.index(HUGE)] == "1|1:2.0"


def test_no_row():
    assert both([], []) is None
    assert both([5], [5]) is None  # one sample: no spread
    assert both([3, 4, 5], [5, 4, 3]) is None  # all sums equal
    assert both([INT32_MIN] * 3, [INT32_MAX] * 3) is None


@pytest.mark.parametrize("spread", [1, 2, 1000, HUGE])
def test_min_spread(spread):
    left, right = pairs_of([], spread)
    assert both(left, right, spread - 1) is not None
    assert both(left, right, spread) is not None
    assert both(left, right, spread + 1) is None
    assert both(left, right, 0) is not None  # (a spread of 0 never makes a row)
    assert both(left, right, (1 << 64) - 1) is None


@pytest.mark.parametrize("counts, maf", [((3, 1, 1), 2), ((2, 1, 2), 3), ((2, 2, 1), 3), ((1, 1, 3), 2),
                                         ((1, 2, 2), 3), ((1, 3, 1), 2), ((1, 3, 2), 3), ((1, 0, 1), 1)])
def test_maf(counts, maf):
    """zero the largest (ties with one, with two), two the largest (a tie with one), one the largest."""
    zero, one, two = counts
    sums = [0] * zero + [2] * one + [4] * two  # spread 4: d = 2 is `one`
    random.Random(sum(counts)).shuffle(sums)
    got = both(sums, [0] * len(sums))
    assert got[0] == maf == S.maf_of(*counts)
    assert got[1] == "SCORES=0,4;freqs=%d/%d/%d" % counts


def test_caps():
    L = T.lib()
    left, right = (C.c_int32 * 3)(0, 1, 7), (C.c_int32 * 3)(0, 0, 0)
    want = S.genotypes([0, 1, 7], [0, 0, 0])
    maf = C.c_uint32()

    def call(info_cap, gt_cap):
        info, gts = C.create_string_buffer(max(info_cap, 1)), C.create_string_buffer(max(gt_cap, 1))
        rc = L.tfbs_scores_as_genotypes(left, right, 3, 1, C.byref(maf), info, info_cap, gts, gt_cap)
        return rc, info.value.decode(), gts.value.decode()

    ni, ng = len(want[1]), len(want[2])
    assert call(ni + 1, ng + 1) == (1, want[1], want[2]) and maf.value == want[0]
    for caps in ((ni, ng + 1), (ni + 1, ng), (0, 0)):
        assert call(*caps)[0] == -1  # TFBS_E_ARG
    assert L.tfbs_scores_as_genotypes(left, right, 3, 8, C.byref(maf), None, 0, None, 0) == 0  # no row: no buffer needed
    assert L.tfbs_scores_as_genotypes(None, None, 3, 1, C.byref(maf), None, 0, None, 0) == -1


# ------------------------------------------------------------ the GPU tests' cases bite
import score_cases as SC  # noqa: E402


def rows_of(case, **kw):
    return [S.region_rows(case["pats"], reg, case["beds"], seqs, **kw) for reg, seqs in zip(case["regions"], case["seqs"])]


@pytest.mark.parametrize("n", SC.SAMPLE_COUNTS)
def test_sample_case_mixes_field_lengths(n):
    rows = rows_of(SC.sample_case(n))[0]
    if n == 1:
        assert rows == []  # one sample has no spread
        return
    assert rows
    if n < 63:
        return
    best = 0
    for row in rows:
        lens = [len(f) + 1 for f in row[5].split("\t")[1:]]
        assert len(lens) == n and set(lens) <= {8, 11}
        if all(len(set(lens[k:k + 64])) == 2 for k in range(0, n - 63, 64)):
            best = max(best, sum(1 for x, y in zip(lens, lens[1:]) if x != y))
    assert best >= n // 4  # a row whose every 64 samples hold both lengths, changing all along


def test_haplotype_count_cases():
    assert rows_of(SC.haps_case("one")) == [[]] and len(set(SC.haps_case("one")["seqs"][0])) == 1
    assert len(set(SC.haps_case("two")["seqs"][0])) == 2 and rows_of(SC.haps_case("two"))[0]
    seqs = SC.haps_case("pairs")["seqs"][0]
    pairs = [(seqs[2 * s], seqs[2 * s + 1]) for s in range(6)]
    assert len(set(pairs)) == 6 and len(set(seqs)) == 4 and rows_of(SC.haps_case("pairs"))[0]


def test_patterns_case():
    case = SC.patterns_case()
    pats = case["pats"]
    rows = [r for rr in rows_of(case) for r in rr]
    assert {"fr", "tie", "long"} <= {r[1] for r in rows} and any(r[1].startswith("di") for r in rows)
    assert not any(r[1] == "other" for r in rows)
    assert len(pats[6]) == 36 and pats[-1].kind == T.KIND_OTHER
    fwd = rev = 0
    import best_ref as R
    for reg, seqs in zip(case["regions"], case["seqs"]):
        for rng in R.region_ranges(reg, case["beds"]):
            for codes, pos in set(seqs):
                f, r = R.best_of(pats[0], codes, pos, rng)[2], R.best_of(pats[1], codes, pos, rng)[2]
                fwd += f > r
                rev += r > f
    assert fwd > 0 and rev > 0


def test_extreme_case():
    case = SC.extreme_case()
    (row,) = rows_of(case)[0]
    assert row[4] == "SCORES=%d,%d;freqs=1/1/1" % (2 * INT32_MIN, 2 * INT32_MAX)
    assert row[5] == "\t1|1:2.0\t0|0:0.0\t0|1:1.0000"
    assert 2 * INT32_MAX - 2 * INT32_MIN == HUGE


def test_none_case():
    case = SC.none_case()
    reg, seqs = case["regions"][0], case["seqs"][0]
    rows = rows_of(case)[0]
    assert [r[0] for r in rows] == ["w.bed"]
    narrow = reg["inner"][0][1:]
    vals = {sq: S.value(case["pats"], 0, sq[0], sq[1], narrow) for sq in set(seqs)}
    gone = [sq for sq, v in vals.items() if v is None]
    assert gone == [seqs[5]] and seqs[8] == seqs[5]  # the deletion haplotype alone
    assert len({v for v in vals.values() if v is not None}) > 1  # the others would make a row


def test_keys_case():
    case = SC.keys_case()
    reg = case["regions"][0]
    import best_ref as R
    assert len(R.region_ranges(reg, case["beds"])) == 42
    rows = rows_of(case)[0]
    keys = [(r[0], r[2], r[3]) for r in rows]
    s = reg["merged"][0]
    assert keys == sorted(keys, key=lambda k: (k[1], k[2], k[0]))  # (a.bed before b.bed)
    assert ("a.bed", s + 15, s + 35) in keys and ("b.bed", s + 15, s + 35) in keys
    assert len(set((k, r[1]) for k, r in zip(keys, rows))) == len(rows)  # the duplicated range once
    assert len({k for k in keys if k[0] == "a.bed"}) >= 20 and not any(k[2] < k[1] for k in keys)


def test_fallback_case():
    case = SC.fallback_case()
    seqs = case["seqs"][0]
    assert case["n"] >= 8193 and len(set(seqs)) == 91
    assert len({(seqs[2 * s], seqs[2 * s + 1]) for s in range(case["n"])}) == 8193
    assert rows_of(case)[0]


def test_multi_case():
    case = SC.multi_case()
    rows = rows_of(case)
    assert all(rows[r] for r in range(4)) and rows[4] == []
    assert len(case["regions"][2]["records"]) == 70


# ------------------------------------------------------------ the run arguments and the command line
def test_run_ext_grew_at_its_end():
    import os
    import subprocess
    old, new = T._capi.tfbs_run_ext, T._capi.tfbs_run_ext_scores
    names = [n for n, _ in new._fields_]
    assert names[:len(old._fields_)] == [n for n, _ in old._fields_]
    assert names[len(old._fields_):] == ["scores_output", "scores_min_spread"]
    for n, _ in old._fields_:  # the earlier layout is a prefix: a caller built against it goes on working
        assert getattr(old, n).offset == getattr(new, n).offset
    assert new.scores_output.offset >= C.sizeof(old) - 8 and new.scores_min_spread.size == 8
    hdr = open(os.path.join(os.path.dirname(T.__file__), "..", "include", "tfbs_amd.h")).read()
    ext = hdr[hdr.index("typedef struct tfbs_run_ext {"):hdr.index("} tfbs_run_ext;")]
    assert ext.index("effects_mode;") < ext.index("scores_output;") < ext.index("scores_min_spread;")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--scores_output FILE" in r.stderr and "--scores_min_spread N" in r.stderr
    r = subprocess.run([exe, "--scores_output"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--scores_output needs a value" in r.stderr
