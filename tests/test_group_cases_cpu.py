"""The haplotype grouper at its limits, without a device (tests/group_cases.py).

Every case's claimed figures are proven from the reference (tests/group_ref.py) alone.
The host grouper (group_host.cpp, TFBS_GROUPER_HOST) equals the reference in all four
outputs -- the distinct masks, their order, their carrier counts, the membership row --
for every call of every case.  Batches built through the host grouper run batch.cpp's
device path (snv_prepare / mask_prepare, the chunk loop, snv_finish / mask_finish and
its remap after a lost group, the membership fetches) and must be the plain host
batch.  tests/test_gpu_group.py runs the same calls and batches on the HIP grouper."""
import pytest

import group_cases as Cs
import group_ref as R
from helpers import T, synth_patterns
from test_gpu_build import _edge_regions

CASE_NAMES = sorted(Cs.CASES)


@pytest.fixture(scope="module")
def reference():
    """Per case, per call, per region: group_ref's (G, masks, counts, row), computed once."""
    return {name: [[R.group(H, reg) for reg in regs] for H, regs in c["calls"]] for name, c in Cs.CASES.items()}


def check_calls(grouper, name, reference):
    """The calls of a case on one handle == the reference, exactly."""
    for ci, (H, regs) in enumerate(Cs.CASES[name]["calls"]):
        got = grouper.group(H, regs)
        assert len(got) == len(regs)
        for j, o in enumerate(got):
            G, masks, counts, row = reference[name][ci][j]
            where = (name, ci, j)
            assert o.n_groups == G, where
            assert o.masks == masks, where
            assert o.counts == counts, where
            if G is None:
                assert o.row == [0xFFFF] * H, where
            else:
                assert o.row == row, where


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_limit(name, reference):
    case, ref = Cs.CASES[name], reference[name]
    claims = case["claims"]
    for H, regs in case["calls"]:
        assert all(len(reg) <= 64 for reg in regs)
        for reg in regs:
            for rec in reg:
                assert rec and all(a < b for a, b in zip(rec, rec[1:])) and rec[-1] < H
    if claims["G"] is not None:
        assert [[r[0] for r in call] for call in ref] == claims["G"]
    for (ci, j), ids in claims.get("free", {}).items():
        G, _, _, row = ref[ci][j]
        assert [h for h, v in enumerate(row) if v == G] == ids
    for (ci, j), masks in claims.get("masks", {}).items():
        assert ref[ci][j][1] == masks
    for (ci, j, m), n in claims.get("count", {}).items():
        G, masks, counts, _ = ref[ci][j]
        assert counts[masks.index(m)] == n
    if "regions" in claims:
        assert [len(regs) for _, regs in case["calls"]] == claims["regions"]
    if "slots" in claims:
        masks = ref[0][0][1]
        hist = {}
        for m in masks:
            hist[R.slot(m)] = hist.get(R.slot(m), 0) + 1
        assert hist == claims["slots"]
        occupied, longest = R.probe_slots(masks)
        assert occupied == claims["occupied"]
        assert 0 in occupied and R.SLOTS - 1 in occupied and longest >= 2  # the chain wraps past slot 0


def test_cases_cover_the_limits(reference):
    """What the cases are there for, read off the reference."""
    Hs = {H for c in Cs.CASES.values() for H, _ in c["calls"]}
    assert {2, 6, 10, 2046, 3002} <= Hs and {8, 16} <= Hs
    assert all(H % 8 for H in (2, 6, 10, 2046, 3002))
    # 2047 masks with and without a reference id, 2048, and the overflow between two neighbours
    G, _, counts, row = reference["limit_a_2047_masks"][0][0]
    assert G == R.G_MAX and row.count(G) == 1 and sum(counts) == Cs.LIMIT_H - 1
    G, _, counts, row = reference["limit_b_2047_masks_no_reference"][0][0]
    assert G == R.G_MAX and row.count(G) == 0 and sum(counts) == Cs.LIMIT_H and max(counts) == 2
    assert len(set(R.id_masks(Cs.LIMIT_H, Cs.LIMIT_C))) == R.G_MAX + 1  # 2048 non-zero masks: no id without one
    assert [len(r) for r in Cs.LIMIT_A] == [1024] * 11  # both kernels' strides loop
    # the order case: a prefix of another mask, bit 63 with lower bits, all ones
    masks = reference["order"][0][0][1]
    full = (1 << 64) - 1
    for m in (1, 3, 1 | 1 << 63, 2, 3 << 62, 1 << 63, full, full >> 1, full - 1):
        assert m in masks
    assert len(Cs.CASES["order"]["calls"][0][1][0]) == 64


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_grouper_is_the_reference(name, reference):
    g = T.Grouper(T.GROUPER_HOST)
    try:
        check_calls(g, name, reference)
    finally:
        g.close()


def test_every_case_on_one_handle(reference):
    """Scratch and membership rows reused across all the cases' calls."""
    g = T.Grouper(T.GROUPER_HOST)
    try:
        for name in CASE_NAMES:
            check_calls(g, name, reference)
    finally:
        g.close()


REFUSED = [
    ("65 records", 200, [[[k] for k in range(65)]]),
    ("id == H", 10, [[[1, 10]]]),
    ("id beyond H in a later region", 10, [[[1, 2]], [[3], [4, 11]]]),
    ("ids descending", 10, [[[3, 2]]]),
    ("an id twice", 10, [[[2, 2]]]),
    ("a record without a carrier", 10, [[[1], []]]),
    ("H == 0", 0, [[]]),
    ("more regions than a chunk", 10, [[] for _ in range(1025)]),
]


def refusals(grouper):
    for why, H, regs in REFUSED:
        with pytest.raises(T.TfbsError) as e:
            grouper.group(H, regs)
        assert e.value.code == -1, why  # TFBS_E_ARG
    # the handle still works
    o, = grouper.group(10, [[[1, 2], [2, 3]]])
    assert (o.n_groups, o.masks, o.counts, o.row) == (3, [1, 3, 2], [1, 1, 1], [3, 0, 1, 2, 3, 3, 3, 3, 3, 3])


def test_refusals():
    g = T.Grouper(T.GROUPER_HOST)
    try:
        refusals(g)
    finally:
        g.close()
    with pytest.raises(T.TfbsError):
        T.Grouper(-1)


# ---- batches through the host grouper ----------------------------------------------------
def edge_batches(tmp_path, n_samples, build_device):
    ps, _ = synth_patterns(tmp_path, 8, 2, 106, thr=1e-3)
    regions = _edge_regions(n_samples, ps.max_length)
    assert len(regions) == 13
    host, dev = Cs.batch_pair(T, ps, n_samples, regions, build_device)
    assert dev.build_stats() == (10, 3)  # on the host: unsorted carriers, 2048+ masks, 65 records
    assert host.build_stats() == (0, 13)
    assert (host.group_calls(), dev.group_calls()) == (0, 1)  # ten regions and the overflowing one, one launch
    assert dev.patch_stats() == 5  # regions 3, 5, 7, 11, 12: one position twice, N, indels, a lost group
    Cs.same_batches(host, dev)
    return ps, host, dev


def limit_batches(tmp_path, build_device):
    """(a) to (d) as SNV regions in one held release: (c) overflows inside the chunk and
    is built on the host afterwards, from inputs the chunk left intact."""
    ps, _ = synth_patterns(tmp_path, 4, 2, 108, thr=1e-3)
    n_samples = Cs.LIMIT_H // 2
    regions = [Cs.snv_region(T, ps.max_length, n_samples, j, recs)
               for j, recs in enumerate((Cs.LIMIT_A, Cs.LIMIT_B, Cs.LIMIT_A, Cs.LIMIT_C, Cs.FIVE))]
    host, dev = Cs.batch_pair(T, ps, n_samples, regions, build_device)
    assert dev.build_stats() == (4, 1) and dev.group_calls() == 1
    assert dev.patch_stats() == 0
    Cs.same_batches(host, dev)
    # 2047 groups and the reference at index 2047; without a reference id a helper copy at 2048
    assert host.region_stats(0)[0] == 2048 and host.layout(0)[2] == 2047
    assert host.region_stats(1)[0] == 2047
    assert dev.layout(1) == host.layout(1)
    return ps, host, dev


def synth_batches(tmp_path, n_samples, indel, count, build_device, calls):
    ps, _ = synth_patterns(tmp_path, 6, 5, 109, thr=1e-3)
    host = T.RegionBatch(ps, n_samples)
    host.synth_fill(5, 0, count, indel)
    dev = T.RegionBatch(ps, n_samples, build_device=build_device)
    dev.synth_fill(5, 0, count, indel)
    assert dev.build_stats() == (count, 0) and dev.group_calls() == calls
    Cs.same_batches(host, dev)
    return ps, host, dev


def test_edge_regions_held_in_one_release(tmp_path):
    edge_batches(tmp_path, 1500, T.GROUPER_HOST)


def test_edge_regions_padded_rows(tmp_path):
    edge_batches(tmp_path, 1501, T.GROUPER_HOST)  # H = 3002: the rows end in padding


def test_limit_regions_in_one_chunk(tmp_path):
    limit_batches(tmp_path, T.GROUPER_HOST)


@pytest.mark.parametrize("cap", ["1", "7"])
@pytest.mark.parametrize("indel", [0, 3])
def test_chunk_loop_takes_further_turns(tmp_path, monkeypatch, indel, cap):
    """130 regions in chunks of 1 and 7 (TFBS_GROUP_REGIONS): the chunk loop's later turns."""
    monkeypatch.setenv("TFBS_GROUP_REGIONS", cap)
    synth_batches(tmp_path, 101, indel, 130, T.GROUPER_HOST, calls=-(-130 // int(cap)))


def test_chunk_cap_is_clamped(tmp_path, monkeypatch):
    for cap, calls in (("0", 9), ("-3", 9), ("x", 9), ("100000", 1), ("", 1)):
        monkeypatch.setenv("TFBS_GROUP_REGIONS", cap)
        synth_batches(tmp_path, 20, 0, 9, T.GROUPER_HOST, calls)
    monkeypatch.delenv("TFBS_GROUP_REGIONS")
    synth_batches(tmp_path, 20, 0, 9, T.GROUPER_HOST, 1)


def test_hold_keeps_regions_out_until_release(tmp_path):
    ps, _ = synth_patterns(tmp_path, 4, 2, 110, thr=1e-3)
    n_samples = 5
    regions = [Cs.snv_region(T, ps.max_length, n_samples, j, [[1, 2], [2, 9]]) for j in range(3)]
    beds = [("synthetic.bed", [reg["merged"] for reg in regions])]
    for dev in (None, T.GROUPER_HOST):
        b = T.RegionBatch(ps, n_samples, build_device=dev)
        b.add_bed("synthetic.bed")
        Cs.fill(T, b, beds, regions[:1])
        with b.hold():
            Cs.fill(T, b, beds, regions[1:])
            assert b.num_regions == 1 and b.num_haplotypes == 4
            assert b.build_stats() == ((1, 0) if dev else (0, 1))
            with pytest.raises(T.TfbsError):
                b.input_digest(1)
        assert b.num_regions == 3 and b.num_haplotypes == 12
        plain = T.RegionBatch(ps, n_samples)
        plain.add_bed("synthetic.bed")
        Cs.fill(T, plain, beds, regions)
        Cs.same_batches(plain, b)
        with b.hold():  # nothing held: the release is a no-op
            pass
        assert b.num_regions == 3


def test_failing_held_region_commits_none(tmp_path):
    ps, _ = synth_patterns(tmp_path, 4, 2, 111, thr=1e-3)
    n_samples = 5
    good = [Cs.snv_region(T, ps.max_length, n_samples, j, [[1, 2], [2, 9]]) for j in range(3)]
    bad = dict(good[1])
    pos, rb = bad["records"][0][1], bad["records"][0][2]
    wrong = [c for c in "ACGT" if c != rb]
    bad["records"] = [("car", pos, wrong[0], wrong[1], [1, 2])]  # REF is not the window's base
    beds = [("synthetic.bed", [reg["merged"] for reg in good])]
    for dev in (None, T.GROUPER_HOST):
        b = T.RegionBatch(ps, n_samples, build_device=dev)
        b.add_bed("synthetic.bed")
        with pytest.raises(T.TfbsError) as e:
            with b.hold():
                Cs.fill(T, b, beds, [good[0], bad, good[2]])
        assert e.value.code == -3  # TFBS_E_REFMISMATCH, the failing region's error
        assert b.num_regions == 0 and b.build_stats() == (0, 0)
        Cs.fill(T, b, beds, good)  # the batch goes on, unheld
        assert b.num_regions == 3
