"""The affinity rows' host side against the plain Python model (affinity_rows_ref.py): the committed
table of the logarithm, tfbs_affinity_mlog2 on the host, tfbs_affinity_as_genotypes, and -- with
affinity_ref.py and the model alone -- that every case of test_gpu_affinity_rows.py bites.  Integer
work: every comparison is exact."""
import importlib.util
import os

import pytest

import affinity_rows_cases as AC
import affinity_rows_ref as M
import score_cases as SC
from helpers import T

ROOT = AC.ROOT


def test_committed_table_is_the_integer_root_table():
    """P[j] is the least p with p^1000 >= 2^(63000 + j): both sides of the bound, for all 1 000 j."""
    P = AC.committed_table()
    for j, p in enumerate(P):
        assert p ** 1000 >= 1 << (63000 + j) and (p - 1) ** 1000 < 1 << (63000 + j), j
    assert P[0] == 1 << 63 and P[999] < 1 << 64 and all(a < b for a, b in zip(P, P[1:]))
    spec = importlib.util.spec_from_file_location("gen_affinity_tables", os.path.join(ROOT, "tools", "gen_affinity_tables.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    assert G.LOG_HEADER == AC.TABLE
    assert "kAffLogP[1000]" in open(AC.TABLE).read()


def test_host_mlog2_equals_the_model():
    xs = AC.boundary_values()
    assert len(xs) > 20000
    got = T.affinity_mlog2(xs)
    bad = [(x, g, M.mlog2(x)) for x, g in zip(xs, got) if g != M.mlog2(x)]
    assert bad == []
    assert T.affinity_mlog2([0, 1, 2, 3, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]) == [-1, 0, 1000, 1584, 62999, 63000, 63999]
    assert T.affinity_mlog2([]) == []
    # a boundary is a step: b - 1 lies one milli-bit below b wherever it shares b's exponent
    P = AC.committed_table()
    for e in AC.BOUNDARY_EXPONENTS:
        for j in (1, 500, 999):
            b = (P[j] + (1 << (63 - e)) - 1) >> (63 - e)
            if (b - 1).bit_length() == b.bit_length() and M.mlog2(b) == 1000 * e + j:
                assert T.affinity_mlog2([b - 1, b]) == [1000 * e + j - 1, 1000 * e + j]


def first_with(y):
    """The least x with mlog2(x) >= y."""
    lo, hi = 0, (1 << 64) - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if M.mlog2(mid) >= y:
            hi = mid
        else:
            lo = mid
    return hi


def both(left, right, top=1234, min_spread=1):
    """The host function's row, checked against the model's."""
    got = T.affinity_as_genotypes(left, right, top, min_spread)
    assert got == M.genotypes(left, right, top, min_spread)
    return got


def test_as_genotypes_equals_the_model():
    # all five field rules: lo 2^10, hi 2^14 (spread 4000), d = 500 (0|0), 1000 and 2999 (0|1), 3000 (1|1)
    xs = [1 << 10, 1 << 14, first_with(10500), first_with(11000), first_with(12999), first_with(13000)]
    assert [M.mlog2(x) for x in xs] == [10000, 14000, 10500, 11000, 12999, 13000]
    maf, info, gts = both(xs, [0] * 6)
    assert gts == "\t0|0:0.0\t1|1:2.0\t0|0:0.2500\t0|1:0.5000\t0|1:1.4995\t1|1:1.5000"
    assert info == "LOG2AFF=10000,14000;AFF=1024,16384;TOP=1234;freqs=2/2/2" and maf == 4
    # the sum is split over the two haplotypes any way
    assert both([x // 2 for x in xs], [x - x // 2 for x in xs]) == (maf, info, gts)
    # half-even ties: spread 64, t = 312.5 d: d = 1 -> 312 (down to even), d = 3 -> 938 (up to even)
    xs = [first_with(40000 + d) for d in (0, 64, 1, 3)]
    assert [M.mlog2(x) for x in xs] == [40000, 40064, 40001, 40003]
    assert both(xs, [0] * 4)[2] == "\t0|0:0.0\t1|1:2.0\t0|0:0.0312\t0|0:0.0938"
    # x = 0 as the minimum: lo = -1
    maf, info, gts = both([0, 1, 0, 1 << 20], [0, 0, 2, 1 << 20], top=-5)
    assert info.startswith("LOG2AFF=-1,21000;AFF=0,2097152;TOP=-5;") and gts.startswith("\t0|0:0.0\t0|0:0.0001\t")
    # all x equal; y equal although x differs: no row
    assert both([7, 3, 5], [0, 4, 2]) is None
    assert M.mlog2(1 << 40) == M.mlog2((1 << 40) + 1) and both([1 << 40, (1 << 40) + 1], [0, 0]) is None
    # min_spread at and one above the spread; 0 counts as 1
    assert both([1, 2], [0, 0], min_spread=1000) is not None and both([1, 2], [0, 0], min_spread=1001) is None
    assert both([1, 2], [0, 0], min_spread=0) == both([1, 2], [0, 0], min_spread=1)
    # the largest values: each side just below 2^63
    top = (1 << 63) - 1
    assert both([top, 1], [top, 0], top=(1 << 31) - 1)[1].startswith("LOG2AFF=0,63999;AFF=1,18446744073709551614;TOP=2147483647;")
    # no sample
    assert both([], []) is None
    # a value of 2^63 or more
    for l, r in (([1 << 63, 1], [0, 0]), ([1, 2], [0, (1 << 64) - 1])):
        with pytest.raises(T.TfbsError) as ei:
            T.affinity_as_genotypes(l, r, 0)
        assert ei.value.code == -1  # TFBS_E_ARG


def rows(case, **kw):
    return [M.region_rows(case["pats"], reg, case["beds"], seqs, **kw) for reg, seqs in zip(case["regions"], case["seqs"])]


def lengths(gts):
    return {len(f) + 1 for f in gts.split("\t")[1:]}


@pytest.mark.parametrize("n", SC.SAMPLE_COUNTS)
def test_sample_case_bites(n):
    """One sample alone has spread 0: no row.  From two samples on there are rows, and from 63 on
    every row mixes 8- and 11-byte fields."""
    got = [r for reg in rows(SC.sample_case(n)) for r in reg]
    assert (got == []) == (n == 1)
    if n >= 63:
        assert all(lengths(r[5]) == {8, 11} for r in got)


def test_cases_bite():
    """Each GPU case writes at least one row where it can, and what the case is about shows in them."""
    assert [len(r) for r in rows(SC.haps_case("one"))] == [0]  # (one distinct haplotype: spread 0)
    for kind in ("two", "pairs"):
        assert sum(len(r) for r in rows(SC.haps_case(kind))) >= 1, kind
    pat = [r for reg in rows(SC.patterns_case()) for r in reg]
    names = {r[1] for r in pat}
    # (its 36-column strand's windows all lie beyond the weight's cutoff: sums of 0, no row; long_case has one that bites)
    assert names == {"fr", "tie", "di2"}
    assert {"long", "m6"} == {r[1] for r in rows(AC.long_case())[0]}
    none = rows(SC.none_case())[0]
    assert {r[0] for r in none} == {"w.bed"}
    keys = rows(SC.keys_case())[0]
    assert len({(r[0], r[2], r[3]) for r in keys}) > 40 and not any(r[3] < r[2] for r in keys)
    with pytest.raises(ValueError):
        rows(SC.extreme_case())
    zero = rows(AC.zero_case())[0]
    assert [(r[4], r[5]) for r in zero] == [("LOG2AFF=-1,41000;AFF=0,2199023255552;TOP=0;freqs=1/0/2",
                                              "\t1|1:2.0\t0|0:0.0\t1|1:1.9512")]
    large = rows(AC.large_case())[0]
    assert len(large) == 1 and int(large[0][4].split(";")[1].split(",")[1]) > 500 << 40
    assert lengths(large[0][5]) == {8, 11}
    multi = rows(SC.multi_case())
    assert sum(len(r) for r in multi) >= 8 and multi[4] == []
    spreads = sorted({int(r[4].split(";")[0].split(",")[1]) - int(r[4].split("=")[1].split(",")[0]) for reg in multi for r in reg})
    assert len(spreads) > 3
    fb = rows(SC.fallback_case())[0]
    assert len(fb) >= 1 and all(len(r[5].split("\t")) == 1 + SC.fallback_case()["n"] for r in fb)
