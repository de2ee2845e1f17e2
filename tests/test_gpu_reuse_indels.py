"""Reference-window reuse across indels on the device: reuse_cases.py's families through the
count path against the oracle (keys and rows; TFBS_DEDUP unset and 0, TFBS_SHARE 1 and 0; whole
batches and regions alone), the census strands' counts against arithmetic on the haplotypes
(reuse_ref.census: every window was counted once), the window lists' sizes and
num_scan_windows against the own-column run lists (tfbs_batch_region_hap_own_runs, which
test_reuse_cases_cpu.py pins against the model; the lists of the regions a device groups are
checked here again), and the hit list folded through the overlap rule against the count path.
Integer work: every comparison is exact."""
import functools

import numpy as np
import pytest

import reuse_cases as K
import reuse_ref as R
from helpers import T, build_batch, depth_classes, run_oracle, window_list_entries

pytestmark = pytest.mark.gpu

MODES = ((False, False), (True, False), (True, True))  # dense download | device reduction | and encoding
# (family, build device): the families whose regions have at most 64 records also grouped on the device
BATCHES = [("single", None), ("pairs", None), ("caps", None), ("odd", None), ("caps", 0), ("odd", 0)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


def test_patterns_take_the_matrix_core_path_in_both_classes():
    ps = K.pattern_set()
    assert ps.plan_stats(mfma=True)["n_mfma_strands"] == len(K.patterns()) == 70
    classes, longer = depth_classes(ps)
    assert not longer and classes[0][:2] == (1, 16) and classes[1][:2] == (17, 32)
    assert sum(classes[0][2].values()) == 64 and sum(classes[1][2].values()) == 6
    assert sorted(K.census_ids().values()) == [1, 2, 8, 16, 17, 32]
    counts = []
    for name in K.FAMILIES:
        for reg in K.family(name)["regions"]:
            counts.append(len(reg["ranges"]))
            assert len(T.select_inner_peaks(reg["merged"], K.beds([reg]))) == len(reg["ranges"])
            if counts[-1] == 16:  # the shared window: every position of the merged range is told apart
                cuts = sorted({hi + 1 for lo, hi in reg["ranges"] if lo == reg["merged"][0]} |
                              {lo for lo, hi in reg["ranges"] if lo != reg["merged"][0]})
                assert all(y - x <= 5 for x, y in zip([reg["merged"][0]] + cuts, cuts))
    assert sorted(set(counts)) == [8, 16, 40] and counts.count(40) == 1


@functools.lru_cache(None)
def _oracle(name, subset):
    """(keys per region, rows) of the oracle for the regions `subset` (None: all) of a family."""
    fam = K.family(name)
    regs = fam["regions"] if subset is None else [fam["regions"][r] for r in subset]
    keys, rows, _ = run_oracle(K.pattern_set(), fam["n"], K.beds(regs), regs)
    as_arrays = lambda lr: tuple(np.asarray(v, dtype=np.uint32) for v in lr)
    return [{k: as_arrays(lr) for k, lr in region.items()} for region in keys], rows


def _check_census(b, regs, keys):
    """The census strands' count of every haplotype id and inner range is the number of windows
    whose first or last position lies in the range (reuse_ref.census), from the batch's own
    haplotypes: the oracle and the product against arithmetic."""
    checked = 0
    for r, reg in enumerate(regs):
        memb = b.membership(r)
        for h, ids in K.ids_of(b, r).items():
            nuc, pos, _ = b.haplotype(r, h)
            for pid, L in K.census_ids().items():
                want = R.census_ranges(nuc, pos, L, reg["ranges"])
                if h == memb[0] or h % 37 == 0:  # (the literal definition on some of them)
                    assert want == [R.census(nuc, pos, L, rng) for rng in reg["ranges"]]
                for rng, w in zip(reg["ranges"], want):
                    lr = keys[r].get(("reuse.bed", rng, pid))
                    for hid in ids:
                        got = lr[hid & 1][hid >> 1] if lr else 0
                        assert got == w, (reg["name"], h, hid, L, rng, got, w)
                    checked += 1
    return checked


@pytest.mark.parametrize("which", ["whole", "alone0", "alone1"])
@pytest.mark.parametrize("name,build_device", BATCHES)
def test_counts(monkeypatch, name, build_device, which):
    """Keys and rows equal the oracle's, with reuse on and off, with shared windows on and off, for
    the whole family in one batch (whole) and for two of its regions alone in a batch (so a
    missing run list cannot borrow a neighbour's); the census strands' counts equal arithmetic
    on the haplotypes."""
    ps = K.pattern_set()
    fam = K.family(name)
    subset = None if which == "whole" else (K.alone(name)[int(which[-1])],)
    regs = fam["regions"] if subset is None else [fam["regions"][r] for r in subset]
    beds = K.beds(regs)
    okeys, orows = _oracle(name, subset)
    census_done = False
    for dedup, share in ((None, "1"), (None, "0"), ("0", "1"), ("0", "0")):
        if dedup is None:
            monkeypatch.delenv("TFBS_DEDUP", raising=False)
        else:
            monkeypatch.setenv("TFBS_DEDUP", dedup)
        monkeypatch.setenv("TFBS_SHARE", share)
        sc = T.Scanner(ps)
        try:
            for reduce, encode in MODES:
                b = build_batch(ps, fam["n"], beds, regs, build_device=build_device)
                if build_device is not None:
                    assert b.build_stats()[0] == len(regs)
                b.scan(sc, reduce=reduce, encode=encode)
                for r, want in enumerate(okeys):
                    got = b.keys_np(r)
                    assert want.keys() == got.keys(), (dedup, share, reduce, r)
                    for k in want:
                        assert np.array_equal(want[k][0], got[k][0]) and np.array_equal(want[k][1], got[k][1]), \
                            (dedup, share, reduce, r, k)
                rows, _ = b.rows("chr1", 0)
                assert rows == orows, (dedup, share, reduce, encode)
                if not census_done:  # (the keys are equal in every mode: once per batch)
                    assert _check_census(b, regs, okeys) > 0
                    census_done = True
                if dedup is None:
                    assert b.num_scan_windows < b.num_windows
        finally:
            sc.close()


def _list_model(b, regs, classes):
    """The window lists' entries per depth class without shared windows, and the (window,
    strand) pairs the scan reads, from the haplotypes and their own-column runs: a haplotype
    scanned whole (the reference, the helper copy, one over 16 runs or over 1 024 columns) lists
    its max(0, n - lmin + 1) windows, one that reuses those of [0, n - lmin] meeting an own run
    with the class's span."""
    entries, scan_windows = [0, 0], 0
    reusing = whole = 0
    for r, reg in enumerate(regs):
        m = len(reg["codes"])
        haps = []
        lens = []
        has_ref = False
        for h in range(b.region_stats(r)[0]):
            nuc, pos, _ = b.haplotype(r, h)
            reuses, _, own = b.hap_own_runs(r, h)
            haps.append((len(nuc), own if reuses else None))
            lens.append(len(nuc))
            has_ref = has_ref or (nuc == reg["codes"] and pos == tuple(range(reg["es"], reg["es"] + m)))
        if not has_ref and m <= 1024 and min(lens) <= 1024:  # the helper copy of the reference
            haps.append((m, None))
            hb, count, ref_hap, _ = b.layout(r)
            assert ref_hap in (None, hb + count)
        for n, own in haps:
            reusing += own is not None
            whole += own is None
            for c, cl in enumerate(classes):
                lmin, S, strands = cl
                listed = [w for w in range(max(0, n - lmin + 1)) if own is None or R.meets(own, w, S)]
                entries[c] += len(listed)
                for L, k in strands.items():
                    scan_windows += k * sum(1 for w in listed if w <= n - L)
    return entries, scan_windows, reusing, whole


@pytest.mark.parametrize("name,build_device", BATCHES)
def test_window_lists(monkeypatch, name, build_device):
    """Without shared windows the lists hold, per depth class, exactly the windows the own-column
    runs make dirty for the class's span, and every window of the haplotypes scanned whole;
    num_scan_windows follows from the same sets, before and after the upload.  For the regions a
    device groups, I1-I4 hold for the lists of the batch built here too."""
    monkeypatch.setenv("TFBS_SHARE", "0")
    monkeypatch.delenv("TFBS_DEDUP", raising=False)
    ps = K.pattern_set()
    fam = K.family(name)
    regs = fam["regions"]
    classes, _ = depth_classes(ps)
    b = build_batch(ps, fam["n"], K.beds(regs), regs, build_device=build_device)
    if build_device is not None:
        assert b.build_stats()[0] == len(regs)
        for r, reg in enumerate(regs):
            res = K.check_region(b, r, reg)
            if name == "caps" and r < 5:
                assert res[1][0] and not res[2][0]  # 16 | 17 runs
    entries, scan_windows, reusing, whole = _list_model(b, regs, classes)
    assert reusing >= 5 and whole >= len(regs)
    before = b.num_scan_windows
    assert before == scan_windows
    sc = T.Scanner(ps)
    try:
        b.scan(sc)
        got = window_list_entries(sc)
        print(name, build_device, "entries", got, "model", entries, "scan windows", before, "of", b.num_windows)
        assert got == entries
        assert b.num_scan_windows == scan_windows
    finally:
        sc.close()


def _fold(hits, pats, reg, beds, memb, n_samples):
    """count_matches_by_sample from a region's hit list: {(bed, range, pattern_id): (L, R)} through
    select_inner_peaks, the overlap rule (a hit's first or last position inside the range) and the
    membership."""
    inner = T.select_inner_peaks(reg["merged"], beds)
    U, P = max(memb) + 1, len(pats)
    hap, pat = hits["haplotype"].astype(np.int64), hits["pattern"].astype(np.int64)
    start, end = hits["start"].astype(np.int64), hits["end"].astype(np.int64)
    memb = np.asarray(memb)
    out = {}
    for bi, a, z in inner:
        inside = ((start >= a) & (start <= z)) | ((end >= a) & (end <= z))
        per_id = np.bincount(hap[inside] * P + pat[inside], minlength=U * P).reshape(U, P)[memb]
        for p in np.nonzero(per_id.any(axis=0))[0]:
            v = per_id[:, p]
            key = (beds[bi][0], (a, z), pats[p].pattern_id)
            assert key not in out
            out[key] = (v[0::2].tolist(), v[1::2].tolist())
    return out


def test_second_opinion_on_the_pairs():
    """The hit list kernel (which shares nothing with the count path: no reuse, no window lists)
    folded through the overlap rule equals the count path's keys on the pairs family."""
    ps = K.pattern_set()
    pats = K.patterns()
    fam = K.family("pairs")
    regs = fam["regions"]
    beds = K.beds(regs)
    sc = T.Scanner(ps)
    try:
        b = build_batch(ps, fam["n"], beds, regs)
        b.upload(sc)
        mine = []
        for r, reg in enumerate(regs):
            hits = b.hits(sc, r, r + 1)
            assert len(hits) > 100 * reg["distinct"] and (hits["region"] == r).all()
            mine.append(_fold(hits, pats, reg, beds, b.membership(r), fam["n"]))
        b.scan(sc, upload=False)
        for r in range(len(regs)):
            got = b.keys(r)
            assert got.keys() == mine[r].keys(), r
            for k in got:
                assert got[k] == mine[r][k], (r, k)
        assert b.num_scan_windows < b.num_windows
    finally:
        sc.close()
