"""The unit kernel's pair pool (scan_mfma.hip, scan_pool; TFBS_SCAN_UNIT, TFBS_SCAN_UNIT_WORDS): a
workgroup keeps the descriptors of its unit of G haplotype groups in the LDS and, per super
tile, hands the window pairs of ALL its groups to its waves from one counter -- no barrier
between the groups; a wave drains its queue when its next pair is another group's; a group's
words come from the unit's LDS copy ("lds": as many of the unit's first groups as fit) or
from global memory ("global").

Every case runs with G = 1, 2, 4 x words = lds, global and must give the oracle's keys and
rows in both download modes each time, the same hit pairs + spill records in all of them, and
the candidates of G = 1 (which windows share a tile does not depend on G).

Groups are small (TFBS_MFMA_HAPS_PER_BLOCK = 4, 5 or 16).  The device orders a region's
distinct haplotypes by their diff lists (ascending, a prefix first), the reference last
(batch.cpp).  A group's list of a depth class is cut into tiles of 32 windows and pairs of
two tiles; where the case fixes the pairs per group it states them and reads them back
(tfbs_ctx_group_pairs).  With TFBS_DEDUP=0 every haplotype lists every window, len - lmin + 1
of them (lmin: the class's shortest strand), so the haplotypes' lengths fix the pairs."""
import ctypes
import random

import pytest

import assembly_cases as A
from helpers import T, build_batch, run_oracle, synth_patterns

pytestmark = pytest.mark.gpu

UNITS = ("1", "2", "4")
WORDS = ("lds", "global")
BOTH_MODES = ((False, False), (True, True))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """The pattern sets of test_gpu_scan_units.py, built once: both depth classes, class 0 only
    (L <= 15), class 1 only (L >= 25)."""
    def make(name, n, config, seed):
        ps, _ = synth_patterns(tmp_path_factory.mktemp(name), n, config, seed, thr=0.05)
        return ps
    out = {"both": make("both", 300, 3, 131), "c0": make("c0", 24, 2, 17), "c1": make("c1", 24, 5, 19)}
    spans = {k: _class_spans(v) for k, v in out.items()}
    assert spans["both"][0] and spans["both"][1], spans
    assert spans["c0"][0] and not spans["c0"][1], spans
    assert spans["c1"][1] and not spans["c1"][0], spans
    return out


def _class_spans(ps):
    """Per depth class of the matrix-core tiles (strands in ascending length, 64 per tile; a
    tile of strands of up to 16 columns is class 0, else class 1): (shortest, longest)
    strand, or None."""
    lens = sorted(len(p.weights) for p in ps.to_list() if 0 < len(p.weights) <= 32)
    cl = [[], []]
    for t in range(0, len(lens), 64):
        tile = lens[t:t + 64]
        cl[1 if max(tile) > 16 else 0].extend(tile)
    return [(min(c), max(c)) if c else None for c in cl]


def _counters(sc):
    lc = (ctypes.c_uint64 * 5)()
    T.check(T.lib().tfbs_ctx_scan_counters(sc.h, lc))
    return {"spill_records": lc[0], "candidates_overflow": lc[1], "candidates": lc[2], "hit_pairs": lc[4]}


def _group_pairs(sc):
    """[class][group]: the pairs of window tiles of the resident batch's lists."""
    out = []
    for c in (0, 1):
        n = ctypes.c_size_t()
        T.check(T.lib().tfbs_ctx_group_pairs(sc.h, c, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_uint32 * max(1, n.value))()
        T.check(T.lib().tfbs_ctx_group_pairs(sc.h, c, buf, n.value, ctypes.byref(n)))
        out.append(list(buf[:n.value]))
    return out


def _pairs_of(windows):
    return ((windows + 31) // 32 + 1) // 2


def _check(monkeypatch, ps, n_samples, beds, regions, hpb=4, env=(), shares=("1",), units=UNITS, words=WORDS,
           pairs=None):
    """Oracle == product for every unit size, words source, sharing mode and download mode;
    hit pairs + spill records equal in all of them, the candidates those of G = 1.  pairs:
    f([class][group] pair counts), the case's statement about them (checked once per
    sharing mode: the lists do not depend on the unit).  Returns {(share, unit, words):
    counters}."""
    okeys, orows, _ = run_oracle(ps, n_samples, beds, regions)
    monkeypatch.setenv("TFBS_MFMA_HAPS_PER_BLOCK", str(hpb))
    for k, v in env:
        monkeypatch.setenv(k, v)
    out = {}
    for share in shares:
        monkeypatch.setenv("TFBS_SHARE", share)  # (read at the upload)
        for unit in units:
            for w in words:
                monkeypatch.setenv("TFBS_SCAN_UNIT", unit)  # (both read when the scanner is made)
                monkeypatch.setenv("TFBS_SCAN_UNIT_WORDS", w)
                sc = T.Scanner(ps)
                try:
                    for reduce, encode in BOTH_MODES:
                        b = build_batch(ps, n_samples, beds, regions)
                        b.scan(sc, reduce=reduce, encode=encode)
                        for i, want in enumerate(okeys):
                            assert b.keys(i) == want, (share, unit, w, reduce, i)
                        rows, _ = b.rows("chr1", 0)
                        assert rows == orows, (share, unit, w, reduce, encode)
                    out[(share, unit, w)] = _counters(sc)
                    if pairs is not None and unit == units[0] and w == words[0]:
                        gp = _group_pairs(sc)
                        print("pairs per group", share, gp)
                        pairs(gp)
                finally:
                    sc.close()
        ref = out[(share, units[0], words[0])]
        for unit in units:
            for w in words:
                c = out[(share, unit, w)]
                print("TFBS_SHARE", share, "TFBS_SCAN_UNIT", unit, "TFBS_SCAN_UNIT_WORDS", w, c)
                assert c["hit_pairs"] + c["spill_records"] == ref["hit_pairs"] + ref["spill_records"], (share, unit, w)
                assert c["candidates"] == ref["candidates"], (share, unit, w)
    return out


def _own_region(ps, start, n, seed):
    """A region of n random bases (extended start to extended end)."""
    rnd = random.Random(seed)
    lmax = ps.max_length
    assert n >= 2 * lmax
    ref = "".join(rnd.choice("ACGT") for _ in range(n))
    return ref, (start, start + n - 2 * lmax + 1), start - lmax + 1


def _snv(ref, es, p, car, k=1):
    return ("car", es + p, ref[p], "ACGT"[("ACGT".index(ref[p]) + k) % 4], sorted(car))


def _region(ref, merged, es, recs):
    return {"merged": merged, "ref": ref, "records": sorted(recs, key=lambda x: x[1])}


def _snv_region(ps, start, n, cols, seed):
    """len(cols) + 1 haplotypes: one SNV each at column cols[t] on haplotype id t + 1, and the
    reference (every other id)."""
    ref, m, es = _own_region(ps, start, n, seed)
    return _region(ref, m, es, [_snv(ref, es, p, [t + 1]) for t, p in enumerate(cols)])


def _beds(regs):
    return [("synthetic.bed", [r["merged"] for r in regs])]


# ---------------------------------------------------------------------------------------
# empty ranges in the pool's table

@pytest.mark.parametrize("K,n_h,gap", [(8, 8, 40), (4, 4, 20), (16, 4, 40), (16, 16, 20)])
def test_groups_without_windows(sets, monkeypatch, K, n_h, gap):
    """test_gpu_scan_units.py's construction with K donors and n_h sharers: sites s < x < K
    pairs (a_k, b_k = a_k + gap); D_j = {s, x, a_j, b_(j + K/2)} (K haplotypes, ordered first)
    list every a's and b's windows, H_k = {s, a_k, b_k} (the next n_h) share them: with gap 40,
    more than the longer class's span, H_k lists nothing; with gap 20 nothing in class 0.  Groups
    of 4, the reference last:
      (8, 8, 40)   D D H H ref   a unit of four whose last two groups have no pair at all, a unit
                                 of two with none (G = 2: H H)
      (4, 4, 20)   D H ref       the middle group has no pair in class 0
      (16, 4, 40)  D D D D H ref the second unit's first group has no pair, its last has
      (16, 16, 20) D x 4, H x 4, ref   a whole unit of four without a pair in class 0"""
    ps = sets["both"]
    (_, s0), (_, s1) = _class_spans(ps)
    assert s0 < 20 < s1 < 32
    ref, m, es = _own_region(ps, 9000, 320, 5)
    s, x, step = 10, 55, 144 // K
    a = [100 + step * k for k in range(K)]
    b = [p + gap for p in a]
    assert len(set(a + b)) == 2 * K and b[-1] + 32 < len(ref)
    for j in range(K):  # D_j's sites: more than the longer span apart
        d = sorted([s, x, a[j], b[(j + K // 2) % K]])
        assert min(q - p for p, q in zip(d, d[1:])) > s1
    recs = [_snv(ref, es, s, range(K + n_h)), _snv(ref, es, x, range(K))]
    cars_a = {k: [k] + ([K + k] if k < n_h else []) for k in range(K)}
    cars_b = {k: [(k + K - K // 2) % K] + ([K + k] if k < n_h else []) for k in range(K)}
    for k in range(K):
        recs.append(_snv(ref, es, a[k], cars_a[k]))
        recs.append(_snv(ref, es, b[k], cars_b[k]))
    reg = _region(ref, m, es, recs)
    empty = range(K // 4, (K + n_h) // 4)  # H's groups

    def pairs(gp):
        assert len(gp[0]) == (K + n_h) // 4 + 1
        for g in range(len(gp[0])):
            assert (gp[0][g] == 0) == (g in empty), (g, gp)
            assert (gp[1][g] == 0) == (g in empty and gap == 40), (g, gp)
    _check(monkeypatch, ps, (K + n_h) // 2 + 4, _beds([reg]), [reg], pairs=pairs)


# ---------------------------------------------------------------------------------------
# one-tile pairs

def test_groups_of_one_tile(sets, monkeypatch):
    """SNVs at columns 1 .. 11 of one region, one haplotype each: haplotype t lists windows
    0 .. t of either class (t + 1 windows: those whose first columns meet the site).  Groups of 4:
    14 and 30 windows -- one tile each, so one pair of ONE tile, followed in the unit's pool by
    the next group's pair --, then haplotypes 9 .. 11 and the reference."""
    ps = sets["both"]
    reg = _snv_region(ps, 5000, 200, list(range(1, 12)), 3)

    def pairs(gp):
        for c in (0, 1):
            assert gp[c][:2] == [1, 1] and gp[c][2] >= 1 and len(gp[c]) == 3, gp
    _check(monkeypatch, ps, 10, _beds([reg]), [reg], pairs=pairs)


# ---------------------------------------------------------------------------------------
# fewer pairs than waves, and many more

def _whole_regions(ps, lens_haps, seed=50):
    """Regions of (n bases, h haplotypes: h - 1 SNVs in the middle and the reference)."""
    regs = []
    for j, (n, h) in enumerate(lens_haps):
        regs.append(_snv_region(ps, 5000 + 20000 * j, n, [n // 2 - 3 + 2 * t for t in range(h - 1)], seed + j))
    return regs


@pytest.mark.parametrize("which,total", [("c0", 1), ("c0", 7), ("c0", 8), ("c0", 9), ("c0", 64), ("both", 8)])
def test_pairs_against_waves(sets, monkeypatch, which, total):
    """TFBS_DEDUP=0: every haplotype lists its len - lmin + 1 windows, so the lengths fix the
    pairs.  Regions of 4 haplotypes are one group each (groups of 4); n = the shortest region
    there is (2 lmax bases).  A unit of four holds `total` pairs of the set's first class:
      1   one region of n bases and 2 haplotypes (a short group): 1 pair
      7   three regions of n bases x 4 haplotypes (2 pairs each), one of 2 haplotypes (1)
      8   four of n x 4
      9   the first region long enough for 3 pairs, then three of n x 4
      64  four regions of 260 bases x 4 (16 pairs each): eight per wave
    ("both": four regions of n x 4 -- the counts of both classes from the same formula.)
    A workgroup has 8 waves."""
    ps = sets[which]
    spans = _class_spans(ps)
    c = 0 if spans[0] else 1
    lmin = spans[c][0]
    n = 2 * ps.max_length
    two = _pairs_of(4 * (n - lmin + 1))
    if which == "c0":
        assert two == 2 and _pairs_of(2 * (n - lmin + 1)) == 1, (n, lmin)
    n3 = next((k for k in range(n, 400) if _pairs_of(4 * (k - lmin + 1)) == 3), None)  # (total 9)
    shape = {1: [(n, 2)], 7: [(n, 4)] * 3 + [(n, 2)], 8: [(n, 4)] * 4, 9: [(n3, 4)] + [(n, 4)] * 3,
             64: [(260, 4)] * 4}[total]
    regs = _whole_regions(ps, shape)

    def pairs(gp):
        for cc in (0, 1):
            want = [_pairs_of(h * (k - spans[cc][0] + 1)) if spans[cc] else 0 for k, h in shape]
            assert gp[cc] == want, (cc, gp, want)
        if which == "c0":
            assert sum(gp[0]) == total, gp
    _check(monkeypatch, ps, 6, _beds(regs), regs, env=(("TFBS_DEDUP", "0"),), pairs=pairs)


# ---------------------------------------------------------------------------------------
# hits on both sides of a group change

def _motif_spec(name, seed, dense):
    """A region of the literal-motif set (assembly_cases.py: only the planted motifs hit): plants
    in its first and in its last columns -- dense: 70 one-column 'A' hits at either end, every
    lane of two whole window tiles fires --, three SNVs on blank columns in the middle, 4
    haplotypes."""
    lay = A.Layout("full", 120, seed)
    st = A.strands("full")
    by_len = {}
    for i, s in enumerate(st):
        by_len.setdefault(s[2], i)
    if dense:
        one = A.strand_of("full", 1)
        for k in range(70):
            lay.plant(one, k)
            lay.plant(one, lay.n - 70 + k)
    else:
        col = 0
        for L in (8, 17, 32):
            lay.plant(by_len[L], col)
            col += L + 1
        col = lay.n
        for L in (9, 16, 31):
            col -= L
            lay.plant(by_len[L], col)
            col -= 1
    mid = lay.n // 2
    sites = [lay.snv(lay.free(mid - 6 + 4 * t, 1)) for t in range(3)]
    A._default_ranges(lay, lay.m, lay.n - 1 - lay.m)
    return A._spec(name, lay, [()] + [(v,) for v in sites])


@pytest.mark.parametrize("dense", [False, True])
def test_hits_at_group_changes(monkeypatch, dense):
    """Eight regions of 4 haplotypes (one group each, TFBS_DEDUP=0: every window scanned) with true
    hits in the first windows of every group's first haplotype and the last windows of its last:
    the last pair of group k and the first pair of group k + 1 both hold hits, and a wave that
    scores both must label each record with its own group (its queue is drained between them).
    dense: 70 hits in a row at either end fill the wave's 64-record queue inside a pair.  The
    literal set's strands share one tile (class 1, shortest strand 1): a haplotype of n bases
    lists n windows."""
    specs = [_motif_spec("pool_%d_%d" % (dense, j), 70 + j, dense) for j in range(8)]
    ps, n_samples, beds, regions = A.materialize(specs)
    n = len(specs[0]["ref"])

    def pairs(gp):
        assert gp[0] == [0] * 8 and gp[1] == [_pairs_of(4 * n)] * 8, gp
    out = _check(monkeypatch, ps, n_samples, beds, regions, env=(("TFBS_DEDUP", "0"),), pairs=pairs)
    c = out[("1", "4", "global")]
    # (a hit counts once per inner range it overlaps; columns 31 .. 69 of the dense plants lie under one)
    assert c["hit_pairs"] + c["spill_records"] >= (8 * 4 * 39 if dense else 1), c


# ---------------------------------------------------------------------------------------
# narrow and wide groups, regions and tails

def test_narrow_and_wide_groups_in_one_unit(sets, monkeypatch):
    """Regions of 4 haplotypes, groups of 4: 240 bases (16-bit list entries), 1 500 bases (more
    than 1 024: 32-bit entries), 240 bases -- a unit of four draws pairs of both kinds of list
    from one pool."""
    ps = sets["both"]
    regs = [_snv_region(ps, 3000, 240, [40, 120, 200], 8), _snv_region(ps, 20000, 1500, [40, 700, 1400], 9),
            _snv_region(ps, 40000, 240, [50, 110, 190], 10)]
    _check(monkeypatch, ps, 6, _beds(regs), regs)


def test_units_over_regions_and_short_tails(sets, monkeypatch):
    """Three regions of 3 haplotypes, groups of 4: groups of 4, 4 and 1 -- the first two span two
    regions each, the last group is short, and so is the last unit of two (one group) and the
    only unit of four (three groups)."""
    ps = sets["both"]
    regs = [_snv_region(ps, 5000 + 3000 * j, 200 + 9 * j, [60, 130], 20 + j) for j in range(3)]

    def pairs(gp):
        assert len(gp[0]) == 3, gp
    _check(monkeypatch, ps, 6, _beds(regs), regs, pairs=pairs)


def test_words_that_do_not_fit(sets, monkeypatch):
    """Sixteen haplotypes of 16 000 bases with an insertion each (no reuse: scanned whole) in one
    group of 16: the group's packed words are 64 KB, more than the LDS has beside the image under
    80 KB, so with TFBS_SCAN_UNIT_WORDS=lds the host gives no group LDS words and the unit reads
    global memory -- the same results as "global"."""
    ps = sets["c0"]
    n = 16000
    ref, m, es = _own_region(ps, 50000, n, 77)
    recs = [("car", es + 500 + 900 * t, ref[500 + 900 * t], ref[500 + 900 * t] + "ACG", [t + 1]) for t in range(16)]
    reg = _region(ref, m, es, recs)
    assert 16 * (n // 16) * 4 > 60 * 1024
    _check(monkeypatch, ps, 10, _beds([reg]), [reg], hpb=16, units=("1", "4"))


# ---------------------------------------------------------------------------------------
# replay and sharing

@pytest.mark.parametrize("words", WORDS)
def test_step_graph_replay(sets, monkeypatch, words):
    """Three tfbs_step calls in a row (the captured graph replays from the third) with units of
    four and of two, then the reduction: the keys of the plain scan, the oracle's."""
    ps = sets["both"]
    reg = _snv_region(ps, 5000, 260, [10 + 13 * t for t in range(17)], 3)
    beds = _beds([reg])
    okeys, _, _ = run_oracle(ps, 20, beds, [reg])
    monkeypatch.setenv("TFBS_MFMA_HAPS_PER_BLOCK", "5")
    monkeypatch.setenv("TFBS_SCAN_UNIT_WORDS", words)
    for unit in ("4", "2"):
        monkeypatch.setenv("TFBS_SCAN_UNIT", unit)
        sc = T.Scanner(ps)
        try:
            b = build_batch(ps, 20, beds, [reg])
            b.scan(sc, reduce=True)
            assert [b.keys(0)] == okeys
            plain = _counters(sc)
            for _ in range(3):
                T.check(T.lib().tfbs_step(sc.h, b.h))
            T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
            assert [b.keys(0)] == okeys
            c = _counters(sc)
            assert c["hit_pairs"] + c["spill_records"] == plain["hit_pairs"] + plain["spill_records"]
            assert c["candidates"] == plain["candidates"]
        finally:
            sc.close()


def test_sharing_on_and_off(sets, monkeypatch):
    """test_gpu_scan_units.py's sharing case (seven far sites in 100 combinations: donors and
    sharers in different groups of a unit and in different units) with TFBS_SHARE 1 and 0."""
    ps = sets["both"]
    s1 = _class_spans(ps)[1][1]
    ref, m, es = _own_region(ps, 7000, 300, 6)
    sites = [20 + (s1 + 3) * t for t in range(7)]
    assert sites[-1] + 32 < len(ref)
    recs = [_snv(ref, es, p, [h for h in range(1, 101) if (h * 37 % 128) >> t & 1]) for t, p in enumerate(sites)]
    reg = _region(ref, m, es, recs)
    out = _check(monkeypatch, ps, 60, _beds([reg]), [reg], shares=("1", "0"))
    assert out[("1", "4", "lds")]["hit_pairs"] + out[("1", "4", "lds")]["spill_records"] > 0
