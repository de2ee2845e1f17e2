"""The rescoring behind the matrix-core scan (scan_mfma.hip, rescore_list / score_candidate): a
pass scores 64 candidates with its loads in two rounds (the first four diff runs and the first
inner ranges among them), lists the hits' own pairs and expands the donors' hits to their
sharers over the pass's flattened entry space, 64 share entries of any donors a round.

Hand-built regions on one random reference of 640 bases.  Sites P_j = 40 + D j, D = the longer
depth class's span + 5: no window of either class holds two of them, so a site's S dirty windows
are listed once, for the lowest-indexed haplotype that carries it (its donor: the device orders
a region's haplotypes by their diff lists, a prefix first, the reference last), and every other
carrier is one share entry of that donor.  Planted beside the 300 random PWMs (threshold 0.05:
hits everywhere, thousands of candidates per wave, so every wave makes several passes from
its global list): literal 12-column PWMs that only the alternative allele at P_0, P_1, P_3, P_4
and P_15 completes (a hit of the donor in the shared windows, for certain), and a literal
6-column PWM on the reference's bases P_0 - 10 .. P_0 - 5: its window is listed for a carrier
of P_0 (within the class span of the site) but its columns meet no diff run, so the rescoring
drops it and the hit comes back through the reference's.

Every case checks: keys and rows equal the oracle's with TFBS_SHARE=1 and with TFBS_SHARE=0;
hit_pairs + spill_records (tfbs_ctx_scan_counters) is the same for TFBS_SCAN_UNIT = 1, 2, 4
and for the default and a small TFBS_CAND_CAP (8 candidates and 32 hit pairs per wave: the
LDS list, the global list and the overflow list are all used, and the hit lists fill in the
middle of an expansion round) -- the total cannot depend on the lists' geometry; the window
lists' sizes and the donors' share entries (tfbs_ctx_share_entries) are the construction's."""
import ctypes
import random

import pytest

from helpers import T, build_batch, depth_classes, run_oracle, synth_patterns, window_list_entries

pytestmark = pytest.mark.gpu

N_REF = 640
UNITS = ("1", "2", "4")
SMALL_CAP = "64"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


class World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The reference, the sites and the pattern set (built once)."""
    w = World()
    ps0, _ = synth_patterns(tmp_path_factory.mktemp("rescore_expand"), 300, 3, 131, thr=0.05)
    classes, longer = depth_classes(ps0)
    assert classes[0] and classes[1] and not longer, classes
    w.D = classes[1][1] + 5
    rnd = random.Random(20)
    w.ref = "".join(rnd.choice("ACGT") for _ in range(N_REF))
    w.P = [40 + w.D * j for j in range(16)]
    assert w.P[-1] + 40 < N_REF
    pats = ps0.to_list()
    pid = max(p.pattern_id for p in pats) + 1

    def literal(word, name):
        nonlocal pid
        rows = [T.Weight(*[100 if ch == b else -100 for b in "ACGT"]) for ch in word]
        pats.append(T.Pattern.PWM(rows, name, pid, 100 * len(word) - 1))
        pid += 1

    for j in (0, 1, 3, 4, 15):  # completed by the alternative allele at P_j (column 4 of 12)
        p = w.P[j]
        literal(w.ref[p - 4:p] + _alt(w.ref, p) + w.ref[p + 1:p + 8], "ALT%d" % j)
    literal(w.ref[w.P[0] - 10:w.P[0] - 4], "CLEAN")  # the reference's bases, columns short of P_0
    w.ps = T.PatternSet.from_patterns(pats)
    w.classes, longer = depth_classes(w.ps)
    assert w.ps.max_length == ps0.max_length and not longer
    assert w.classes[1][1] + 5 == w.D and w.classes[0][1] >= 12  # CLEAN's window at P_0 - 10 is listed in class 0
    return w


def _alt(ref, p, k=1):
    return "ACGT"[("ACGT".index(ref[p]) + k) % 4]


def _snv(ref, es, p, car, k=1):
    return ("car", es + p, ref[p], _alt(ref, p, k), sorted(car))


def _place(w, start, n=N_REF):
    """The region of the reference's first n bases at `start`: (merged, extended start)."""
    lmax = w.ps.max_length
    return (start, start + n - 2 * lmax + 1), start - lmax + 1


def _region(w, start, site_carriers, n=N_REF, extra=()):
    """site_carriers: {site: haplotype ids}."""
    m, es = _place(w, start, n)
    recs = [_snv(w.ref, es, p, car) for p, car in sorted(site_carriers.items()) if car] + list(extra)
    return {"merged": m, "ref": w.ref[:n], "es": es, "records": sorted(recs, key=lambda x: x[1])}


def _counters(sc):
    lc = (ctypes.c_uint64 * 5)()
    T.check(T.lib().tfbs_ctx_scan_counters(sc.h, lc))
    return {"spill_records": lc[0], "candidates_overflow": lc[1], "candidates": lc[2], "hit_pairs": lc[4]}


def _share_entries(sc):
    """Per depth class: the share entries of every haplotype of the resident batch as a donor."""
    out = []
    for c in range(2):
        n = ctypes.c_size_t()
        T.check(T.lib().tfbs_ctx_share_entries(sc.h, c, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_uint32 * max(1, n.value))()
        T.check(T.lib().tfbs_ctx_share_entries(sc.h, c, buf, n.value, ctypes.byref(n)))
        out.append(list(buf[:n.value]))
    return out


def _check(monkeypatch, w, n_samples, beds, regions, hpb=None):
    """The three checks of the module docstring.  Returns (window-list entries with sharing,
    share entries per class, {(unit, cap): counters}, the last batch)."""
    ps = w.ps
    okeys, orows, _ = run_oracle(ps, n_samples, beds, regions)
    if hpb is not None:
        monkeypatch.setenv("TFBS_MFMA_HAPS_PER_BLOCK", str(hpb))
    monkeypatch.delenv("TFBS_SCAN_UNIT", raising=False)
    monkeypatch.delenv("TFBS_CAND_CAP", raising=False)

    def run(sc, reduce, encode, tag):
        b = build_batch(ps, n_samples, beds, regions)
        b.scan(sc, reduce=reduce, encode=encode)
        for i, want in enumerate(okeys):
            assert b.keys(i) == want, (tag, i)
        rows, _ = b.rows("chr1", 0)
        assert rows == orows, tag
        return b

    lists = entries = None
    for share in ("0", "1"):
        monkeypatch.setenv("TFBS_SHARE", share)  # (read at the upload)
        sc = T.Scanner(ps)
        try:
            run(sc, False, False, ("share", share))
            if share == "1":
                lists, entries = window_list_entries(sc), _share_entries(sc)
        finally:
            sc.close()
    out, b = {}, None
    for unit in UNITS:
        monkeypatch.setenv("TFBS_SCAN_UNIT", unit)  # (read when the scanner is made)
        for cap in (None, SMALL_CAP):
            if cap is None:
                monkeypatch.delenv("TFBS_CAND_CAP", raising=False)
            else:
                monkeypatch.setenv("TFBS_CAND_CAP", cap)
            sc = T.Scanner(ps)
            try:
                b = run(sc, True, True, (unit, cap))
                out[(unit, cap)] = _counters(sc)
            finally:
                sc.close()
            print("TFBS_SCAN_UNIT", unit, "TFBS_CAND_CAP", cap, out[(unit, cap)])
    totals = {k: v["hit_pairs"] + v["spill_records"] for k, v in out.items()}
    assert len(set(totals.values())) == 1 and totals[("1", None)] > 0, totals
    for cap in (None, SMALL_CAP):
        assert len({out[(u, cap)]["candidates"] for u in UNITS}) == 1, out
    small = out[("1", SMALL_CAP)]
    assert small["candidates_overflow"] > 0 and small["spill_records"] > 0, small  # all three lists, full hit lists
    n_groups = (b.num_haplotypes + (hpb or 64) - 1) // (hpb or 64)
    assert out[("1", None)]["candidates"] > 64 * 8 * n_groups  # some wave makes a second pass (from its global list)
    monkeypatch.delenv("TFBS_SCAN_UNIT", raising=False)
    monkeypatch.delenv("TFBS_CAND_CAP", raising=False)
    print("window lists", lists, "share entries", [sorted(e, reverse=True)[:6] for e in entries])
    return lists, entries, out, b


def _subset_sites(w, carriers, first_far=2):
    """{far site: ids}: carrier j of `carriers` (haplotype id, subset number) also carries far
    site P_(first_far + t) for every set bit t of its subset number."""
    out = {}
    for hid, j in carriers:
        for t in range(7):
            if (j >> t) & 1:
                out.setdefault(w.P[first_far + t], []).append(hid)
    return out


def _expect_lists(w, n, n_sites):
    """The reference's windows and S dirty windows per site, per class."""
    return [n - w.classes[c][0] + 1 + n_sites * w.classes[c][1] for c in range(2)]


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 127])
def test_entries_per_donor(world, monkeypatch, k):
    """P_0 carried by k + 1 haplotypes, told apart by subsets of up to 7 far sites: {P_0}
    alone is the lowest-indexed and the donor of k entries -- none, one, a round less one, a
    whole round, a round and one, two rounds (less one: 2^7 subsets)."""
    w = world
    carriers = [(1 + j, j) for j in range(k + 1)]
    sites = _subset_sites(w, carriers)
    sites[w.P[0]] = [h for h, _ in carriers]
    reg = _region(w, 5000, sites)
    lists, entries, _, b = _check(monkeypatch, w, 70, [("synthetic.bed", [reg["merged"]])], [reg])
    assert b.num_haplotypes == k + 2
    assert lists == _expect_lists(w, N_REF, len(sites))
    far = sum(len(v) - 1 for p, v in sites.items() if p != w.P[0])
    for c in range(2):
        assert max(entries[c]) == k and sum(entries[c]) == k + far, (c, sorted(entries[c], reverse=True)[:8])


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_totals_straddle_a_round(world, monkeypatch, d):
    """Two donors in one group: {P_0} with 40 entries and {P_1} with 24 + d: their hits'
    entries lie end to end in a pass, 63, 64 and 65 in sum."""
    w = world
    ca = [(1 + j, j) for j in range(41)]
    cb = [(60 + j, j) for j in range(25 + d)]
    sites = _subset_sites(w, ca + cb)
    sites[w.P[0]] = [h for h, _ in ca]
    sites[w.P[1]] = [h for h, _ in cb]
    reg = _region(w, 9000, sites)
    lists, entries, _, b = _check(monkeypatch, w, 70, [("synthetic.bed", [reg["merged"]])], [reg])
    assert b.num_haplotypes == 41 + 25 + d + 1
    assert lists == _expect_lists(w, N_REF, len(sites))
    far = sum(len(v) - 1 for p, v in sites.items() if p not in (w.P[0], w.P[1]))
    for c in range(2):
        assert 40 in entries[c] and 24 + d in entries[c] and sum(entries[c]) == 64 + d + far, sorted(entries[c])[-8:]


def _hundred(w, start, mul, n_haps=100):
    """n_haps haplotypes over seven sites (ids 1 .. n_haps, subset (id * mul) % 128)."""
    return _region(w, start, _subset_sites(w, [(h, (h * mul) % 128) for h in range(1, n_haps + 1)], first_far=0))


def test_popcounts_and_ranges_past_32(world, monkeypatch):
    """Three nested inner ranges: hits overlap one, two or three of them, so the donors'
    masks differ inside a round; a second region with 34 nested ranges: the ranges past 32
    take the spill path (for_sharers) beside them."""
    w = world
    # (the second region short, with three haplotypes: the oracle's time grows with hits x ranges)
    regs = [_hundred(w, 5000, 1, 12), _region(w, 9000, {w.P[0]: [1, 2], w.P[1]: [2, 3]}, n=120)]
    m0, m1 = regs[0]["merged"], regs[1]["merged"]
    ranges = [m0, (m0[0], m0[0] + 150), (m0[0], m0[0] + 320), m1] + [(m1[0], m1[0] + 1 + k) for k in range(33)]
    lists, entries, out, b = _check(monkeypatch, w, 15, [("synthetic.bed", ranges)], regs)
    assert b.layout(0)[3] == 3 and b.layout(1)[3] == 34
    assert out[("1", None)]["spill_records"] > 0  # (the ranges past 32)
    n_sites = [len({p for r in reg["records"] for p in [r[1]]}) for reg in regs]
    assert lists == [a + b_ for a, b_ in zip(_expect_lists(w, N_REF, n_sites[0]), _expect_lists(w, 120, n_sites[1]))]
    assert all(max(e) > 0 for e in entries)


def test_groups_of_a_unit(world, monkeypatch):
    """Groups of 5 haplotypes: 101 haplotypes make 21 groups, donors and sharers in
    different groups of a unit of 2 or 4 and in different units; the last group holds one
    haplotype and the last unit one group."""
    w = world
    reg = _hundred(w, 5000, 37)
    lists, entries, out, b = _check(monkeypatch, w, 60, [("synthetic.bed", [reg["merged"]])], [reg], hpb=5)
    assert b.num_haplotypes == 101
    assert all(max(e) > 5 for e in entries)  # a donor's sharers span groups


@pytest.fixture(scope="module")
def run_regions(world):
    """Four regions, one haplotype each beside the reference, with 1, 4, 5 and 16 diff runs
    (sites P_0 .. P_(r - 1)): the planted hit at the LAST site's alternative allele is dirty
    only through the haplotype's last run -- the only run, the last of the four loaded up
    front, the first of the loop behind them, the loop's last."""
    w = world
    return [_region(w, 5000 + 3000 * j, {w.P[t]: [1] for t in range(r)}) for j, r in enumerate((1, 4, 5, 16))]


def test_diff_runs_at_the_batch_boundary(world, run_regions, monkeypatch):
    w = world
    beds = [("synthetic.bed", [r["merged"] for r in run_regions])]
    lists, entries, _, b = _check(monkeypatch, w, 4, beds, run_regions)
    for j, r in enumerate((1, 4, 5, 16)):
        U = b.layout(j)[1]
        assert sorted(len(b.hap_own_runs(j, l)[2]) for l in range(U)) == [0, r]
    assert all(max(e) == 0 for e in entries)  # nothing to share: every site has one carrier
    assert lists == [4 * (N_REF - w.classes[c][0] + 1) + 26 * w.classes[c][1] for c in range(2)]


def test_n_and_indel_beside_sharers(world, monkeypatch):
    """A haplotype with an N and one with an insertion (position table) in the group of
    donors and sharers of P_0 and P_3: they neither donate nor share."""
    w = world
    m, es = _place(w, 5000)
    q, r = w.P[1] + 11, w.P[2] + 9
    extra = [("car", es + q, w.ref[q], w.ref[q] + "AC", [10, 11]), ("car", es + r, w.ref[r], "N", [12, 13])]
    reg = _region(w, 5000, {w.P[0]: [0, 1, 10, 12, 14, 15], w.P[3]: [1, 2, 11, 13, 15]}, extra=extra)
    lists, entries, _, b = _check(monkeypatch, w, 20, [("synthetic.bed", [m])], [reg])
    # {P_0}, {P_0, P_3}, {P_3} share; the four others list their own windows
    assert [max(e) for e in entries] == [1, 1] and [sum(e) for e in entries] == [2, 2], entries


def test_step_graph_replay(world, monkeypatch):
    """Three tfbs_step calls (the captured step graph from the third on) on the batch of a
    donor with 65 entries, units of 4: the oracle's keys, as the plain scan's."""
    w = world
    carriers = [(1 + j, j) for j in range(66)]
    sites = _subset_sites(w, carriers)
    sites[w.P[0]] = [h for h, _ in carriers]
    reg = _region(w, 5000, sites)
    beds = [("synthetic.bed", [reg["merged"]])]
    okeys, _, _ = run_oracle(w.ps, 70, beds, [reg])
    monkeypatch.setenv("TFBS_SHARE", "1")
    monkeypatch.setenv("TFBS_SCAN_UNIT", "4")
    monkeypatch.setenv("TFBS_MFMA_HAPS_PER_BLOCK", "16")
    sc = T.Scanner(w.ps)
    try:
        b = build_batch(w.ps, 70, beds, [reg])
        b.scan(sc, reduce=True)
        assert [b.keys(0)] == okeys
        assert max(_share_entries(sc)[0]) == 65
        for _ in range(3):
            T.check(T.lib().tfbs_step(sc.h, b.h))
        T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
        assert [b.keys(0)] == okeys
    finally:
        sc.close()
