"""Units of the merged matrix-core scan (scan_mfma.hip, scan_mfma_all_kernel<.., UNIT>;
TFBS_SCAN_UNIT): one workgroup scans G = 1, 2 or 4 consecutive haplotype groups per staged
super tile image, restaging only a group's descriptors and words, and rescores the
candidates of the whole unit once.  Every case runs with G = 1, 2 and 4 and must give the
oracle's keys and rows each time (dense download, and the device reduction + encoding).

Groups are made small (TFBS_MFMA_HAPS_PER_BLOCK = 4 or 5), so a few dozen haplotypes
make many groups.  The device orders a region's distinct haplotypes by their diff lists
(ascending, a prefix first), the reference group last (batch.cpp), which the hand-built
regions below rely on to place haplotypes in groups and units."""
import ctypes
import random

import pytest

from helpers import T, build_batch, make_regions_synth, run_oracle, synth_patterns

pytestmark = pytest.mark.gpu

UNITS = ("1", "2", "4")
BOTH_MODES = ((False, False), (True, True))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """The pattern sets, built once: both depth classes (300 PWMs: strands of 8-22 and of
    23-30 columns), class 0 only (L <= 15), class 1 only (L >= 25), and a small set with a
    high threshold (many candidates and hits)."""
    def make(name, n, config, seed, thr):
        ps, _ = synth_patterns(tmp_path_factory.mktemp(name), n, config, seed, thr=thr)
        return ps
    out = {"both": make("both", 300, 3, 131, 0.05), "c0": make("c0", 24, 2, 17, 0.05),
           "c1": make("c1", 24, 5, 19, 0.05), "dense": make("dense", 12, 3, 41, 0.05)}
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


def _check(monkeypatch, ps, n_samples, beds, regions, hpb=4, env=(), shares=("1",), modes=BOTH_MODES, units=UNITS,
           groups=None):
    """Oracle == product for every unit size, sharing mode and download mode.  groups: the
    haplotype groups the batch must make.  Returns {(share, unit): scan counters}."""
    okeys, orows, _ = run_oracle(ps, n_samples, beds, regions)
    monkeypatch.setenv("TFBS_MFMA_HAPS_PER_BLOCK", str(hpb))
    for k, v in env:
        monkeypatch.setenv(k, v)
    out = {}
    for share in shares:
        monkeypatch.setenv("TFBS_SHARE", share)  # (read at the upload)
        for unit in units:
            monkeypatch.setenv("TFBS_SCAN_UNIT", unit)  # (read when the scanner is made)
            sc = T.Scanner(ps)
            try:
                for reduce, encode in modes:
                    b = build_batch(ps, n_samples, beds, regions)
                    if groups is not None:  # (a reference group in every region: no helper copies)
                        assert (b.num_haplotypes + hpb - 1) // hpb == groups, (b.num_haplotypes, hpb)
                    b.scan(sc, reduce=reduce, encode=encode)
                    for i, want in enumerate(okeys):
                        assert b.keys(i) == want, (share, unit, reduce, i)
                    rows, _ = b.rows("chr1", 0)
                    assert rows == orows, (share, unit, reduce, encode)
                out[(share, unit)] = _counters(sc)
            finally:
                sc.close()
    return out


def _own_region(ps, start, n, seed):
    """A region of n random bases (extended start to extended end)."""
    rnd = random.Random(seed)
    lmax = ps.max_length
    ref = "".join(rnd.choice("ACGT") for _ in range(n))
    return ref, (start, start + n - 2 * lmax + 1), start - lmax + 1


def _snv(ref, es, p, car, k=1):
    return ("car", es + p, ref[p], "ACGT"[("ACGT".index(ref[p]) + k) % 4], sorted(car))


def _region(ref, merged, es, recs):
    return {"merged": merged, "ref": ref, "records": sorted(recs, key=lambda x: x[1])}


def _single_snv_region(ps, start, n, n_distinct, seed):
    """n_distinct haplotypes: one SNV each on haplotype ids 1 .. n_distinct - 1, and the
    reference (every other id)."""
    ref, m, es = _own_region(ps, start, n, seed)
    step = (n - 20) // n_distinct
    return _region(ref, m, es, [_snv(ref, es, 10 + step * t, [t]) for t in range(1, n_distinct)])


@pytest.mark.parametrize("groups,n_distinct", [(1, 3), (2, 7), (3, 10), (5, 18), (9, 35)])
def test_unit_tails(sets, monkeypatch, groups, n_distinct):
    """1, 2, 3, 5 and 9 groups of 4: the last group and the last unit are short."""
    ps = sets["both"]
    reg = _single_snv_region(ps, 5000, 260, n_distinct, 3)
    _check(monkeypatch, ps, 20, [("synthetic.bed", [reg["merged"]])], [reg], groups=groups)


def test_group_and_unit_span_regions(sets, monkeypatch):
    """Five regions of three haplotypes, groups of 4: group 0 spans two regions, a unit of
    two groups three, a unit of four all five."""
    ps = sets["both"]
    regs = [_single_snv_region(ps, 5000 + 2000 * j, 200 + 7 * j, 3, 10 + j) for j in range(5)]
    _check(monkeypatch, ps, 10, [("synthetic.bed", [r["merged"] for r in regs])], regs, groups=4)


@pytest.mark.parametrize("gap", [20, 40])
def test_units_without_windows(sets, monkeypatch, gap):
    """Haplotypes that list no window of their own.  Sites s < x < 16 pairs (a_k, b_k = a_k +
    gap).  D_j = {s, x, a_j, b_(j + 8)} (16 haplotypes, ordered first: x precedes every a)
    list every a's and b's windows; H_k = {s, a_k, b_k} (the next 16: one whole unit of
    four groups, two units of two, four of one) share them.  With gap 40, more than the
    longer class's span, H_k lists nothing in either class; with gap 20, between the two
    spans, nothing in class 0 and only the windows over both sites in class 1.  Any two
    sites of one haplotype are more than the longer span apart (but a_k, b_k at gap 20).
    The reference comes last."""
    ps = sets["both"]
    (_, s0), (_, s1) = _class_spans(ps)
    assert s0 < 20 < s1 < 32
    ref, m, es = _own_region(ps, 9000, 320, 5)
    K = 16
    s, x = 10, 55
    a = [100 + 9 * k for k in range(K)]
    b = [p + gap for p in a]
    assert len(set(a + b)) == 2 * K and b[-1] + 32 < len(ref)
    for j in range(K):  # D_j's sites
        d = sorted([s, x, a[j], b[(j + 8) % K]])
        assert min(q - p for p, q in zip(d, d[1:])) > s1
    recs = [_snv(ref, es, s, range(2 * K)), _snv(ref, es, x, range(K))]
    for k in range(K):
        recs.append(_snv(ref, es, a[k], [k, K + k]))
        recs.append(_snv(ref, es, b[k], [(k + 8) % K, K + k]))
    reg = _region(ref, m, es, recs)
    _check(monkeypatch, ps, 30, [("synthetic.bed", [m])], [reg], groups=9)  # 32 + the reference


@pytest.mark.parametrize("which", ["c0", "c1"])
def test_single_depth_class(sets, monkeypatch, which):
    """Only class-0 strands (L <= 16), only class-1 strands: the other class's lists and
    super tiles do not exist."""
    ps = sets[which]
    regs = make_regions_synth(7, 0, 2, 12, ps.max_length, 0)
    _check(monkeypatch, ps, 12, [("synthetic.bed", [r["merged"] for r in regs])], regs)


def test_several_super_tiles_per_class(sets, monkeypatch):
    """A 12 KiB image budget: several super tiles per depth class, each staged once per
    unit with the unit's groups inside."""
    ps = sets["both"]
    st = ps.plan_stats(mfma=True)
    reg = _single_snv_region(ps, 5000, 260, 18, 3)
    _check(monkeypatch, ps, 20, [("synthetic.bed", [reg["merged"]])], [reg], env=(("TFBS_MFMA_LDS_KB", "12"),), groups=5)
    assert st["n_mfma_strands"] >= 512  # (8+ tiles of 1.5-6 KiB: more than two images of 12 KiB)


def test_sharing_across_groups_and_units(sets, monkeypatch):
    """Seven sites at least the longer span + 3 apart ("far site pairs"), carried in 100
    combinations: a window's donor and its sharers lie in different groups of a unit and in
    different units; the same with TFBS_SHARE=0."""
    ps = sets["both"]
    s1 = _class_spans(ps)[1][1]
    ref, m, es = _own_region(ps, 7000, 300, 6)
    sites = [20 + (s1 + 3) * t for t in range(7)]
    assert sites[-1] + 32 < len(ref)
    recs = [_snv(ref, es, p, [h for h in range(1, 101) if (h * 37 % 128) >> t & 1]) for t, p in enumerate(sites)]
    reg = _region(ref, m, es, recs)
    out = _check(monkeypatch, ps, 60, [("synthetic.bed", [m])], [reg], shares=("1", "0"))
    assert out[("1", "4")]["hit_pairs"] + out[("1", "4")]["spill_records"] > 0


def test_other_haplotype_kinds_in_one_unit(sets, monkeypatch):
    """A short region with an indel haplotype and a haplotype with N, a region of more
    than 1024 bases (scanned whole, 32-bit list entries) and a region of the generator with
    30 % indels: with groups of 4 the first unit of four holds haplotypes of all three."""
    ps = sets["both"]
    ref, m, es = _own_region(ps, 3000, 240, 8)
    recs = [_snv(ref, es, 120, [0, 1, 10, 12]), _snv(ref, es, 200, [1, 2, 11, 13]),
            ("car", es + 160, ref[160], ref[160] + "AC", [10, 11]), ("car", es + 180, ref[180], "N", [12, 13])]
    short = _region(ref, m, es, recs)
    ref2, m2, es2 = _own_region(ps, 20000, 1500, 9)
    long_ = _region(ref2, m2, es2, [_snv(ref2, es2, p, [h]) for h, p in enumerate((40, 700, 1400))])
    synth = make_regions_synth(11, 40, 1, 12, ps.max_length, 30)
    regs = [short, long_] + synth
    _check(monkeypatch, ps, 12, [("synthetic.bed", [r["merged"] for r in regs])], regs)


def test_list_limits(sets, monkeypatch):
    """A high threshold with 8 candidate entries per wave and group and 16 overflow
    entries: candidates pass the LDS list, the wave's global list and the overflow list
    (the scan grows it and runs again), hit pairs spill (as test_gpu_parity.py's last
    case).  The one-group kernel itself overflows; a unit's waves hold four groups'
    candidates in four groups' room."""
    ps = sets["dense"]
    regs = make_regions_synth(31, 0, 3, 30, ps.max_length, 0)
    out = _check(monkeypatch, ps, 30, [("synthetic.bed", [r["merged"] for r in regs])], regs,
                 env=(("TFBS_CAND_CAP", "64"), ("TFBS_CAND_OVER_CAP", "16")))
    for unit in UNITS:
        c = out[("1", unit)]
        print("TFBS_SCAN_UNIT", unit, c)
        assert c["candidates"] == out[("1", "1")]["candidates"]
    ref = out[("1", "1")]
    assert ref["candidates_overflow"] > 16 and ref["spill_records"] > 0, ref


def test_step_graph_replay(sets, monkeypatch):
    """Five tfbs_step calls (the captured step graph) with units of four, then the
    reduction: the oracle's keys."""
    ps = sets["both"]
    reg = _single_snv_region(ps, 5000, 260, 18, 3)
    beds = [("synthetic.bed", [reg["merged"]])]
    okeys, _, _ = run_oracle(ps, 20, beds, [reg])
    monkeypatch.setenv("TFBS_MFMA_HAPS_PER_BLOCK", "5")
    monkeypatch.setenv("TFBS_SCAN_UNIT", "4")
    sc = T.Scanner(ps)
    try:
        b = build_batch(ps, 20, beds, [reg])
        b.scan(sc, reduce=True)
        assert [b.keys(0)] == okeys
        for _ in range(5):
            T.check(T.lib().tfbs_step(sc.h, b.h))
        T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
        assert [b.keys(0)] == okeys
    finally:
        sc.close()
