"""Reference-window reuse across indels pinned on the host batch alone (no device): the two run
lists of every haplotype of reuse_cases.py (tfbs_batch_region_hap_own_runs: its own columns, what
the scan reads; tfbs_batch_region_hap_runs: the reference's columns, the hits the key assembly
passes on) against reuse_ref.py's model, which knows nothing of segments.  For every haplotype
that reuses and every L in {1, 2, 8, 15, 16, 17, 31, 32}:

I1  clean means equal: a window meeting no own run is a reference window (bases and positions).
I2  bijection: window -> reference window over the clean windows is injective, and its image is
    exactly the reference windows meeting no reference-column run (passed-on reference hits +
    scanned windows count every window once).
I3  form: both lists ascending, merged, at most 16 runs, a run to the end only last, a boundary
    run exactly (a, a - 1).
I4  footprint: every run lies within what the haplotype's applied records touch
    (reuse_ref.footprints: stated from the patcher's rules, not measured), so "everything dirty"
    does not pass I1 and I2.

The model does not demand maximality: an insertion whose last base equals the anchor leaves a
window equal to a reference window under a second alignment, which the builder rejects; such a
window is dirty, and I1 and I2 hold all the same.  And the cases sit on the edges they are named
for."""
import functools

import pytest

import reuse_cases as K
import reuse_ref as R
from helpers import T, build_batch


@functools.lru_cache(None)
def host_batch(name, grouped=False):
    """The host batch of a family, built once and never modified.  grouped: through the host
    grouper (TFBS_GROUPER_HOST), as a device groups it: regions of at most 64 records take the
    builder's other branches (SNVs alone: runs added column by column from the groups' masks;
    with indels: the groups patched on the host)."""
    f = K.family(name)
    return build_batch(K.pattern_set(), f["n"], K.beds(f["regions"]), f["regions"],
                       build_device=T.GROUPER_HOST if grouped else None)


@functools.lru_cache(None)
def checked(name, r, grouped=False):
    """I1-I4 over region r of a family; {haplotype id: (reuses, own runs, reference-column runs)}."""
    return K.check_region(host_batch(name, grouped), r, K.family(name)["regions"][r])


def _regions():
    return [(name, r, grouped) for name in K.FAMILIES for r in range(len(K.family(name)["regions"]))
            for grouped in ((False, True) if name in ("caps", "odd") else (False,))]


@pytest.mark.parametrize("name,r,grouped", _regions(), ids=lambda x: str(x))
def test_run_lists_against_the_model(name, r, grouped):
    res = checked(name, r, grouped)
    reg = K.family(name)["regions"][r]
    assert any(v[0] for v in res.values()) == (reg["name"] != "len_1025")
    if grouped:  # the same lists whichever way the region was built
        assert res == checked(name, r)


def test_the_model_alone_keeps_the_bound():
    """The bound of I4 is buildable: run lists made here from the model alone (a column is clean
    iff some window of length 1 there equals a reference window and its neighbour continues it)
    lie within reuse_ref.footprints for every haplotype of the cases -- so the bound comes from the
    records, not from the library's lists."""
    total = 0
    for name in K.FAMILIES:
        for reg in K.family(name)["regions"]:
            ref, es = reg["codes"], reg["es"]
            m = len(ref)
            for hid, recs in reg["placed"].items():
                nuc, pos, applied, truncated = R.patch(ref, es, recs)
                n = len(nuc)
                fq, fq_end, fo, fo_end = R.footprints(applied, truncated, m, n)
                # greedy cover: extend a window from column w while it stays a reference window,
                # and only onto reference columns past those already taken (what any valid pair
                # of lists must leave dirty at the least is not known to the model; this cover is
                # one valid choice, and it must fit the bound)
                own_dirty, taken, w, qend = [], set(), 0, 0
                breaks_own, breaks_ref = [], []
                prev = None
                while w < n:
                    q = R.equal_window(ref, es, nuc, pos, w, 1)
                    if q is None or q < qend:
                        own_dirty.append(w)
                        w += 1
                        continue
                    L = 1
                    while w + L < n and R.equal_window(ref, es, nuc, pos, w, L + 1) == q:
                        L += 1
                    if prev is not None and prev[0] == w:
                        breaks_own.append(w)
                    if prev is not None and prev[1] == q:
                        breaks_ref.append(q)
                    taken.update(range(q, q + L))
                    qend = q + L
                    prev = (w + L, q + L)
                    w += L
                ref_dirty = [q for q in range(m) if q not in taken]
                tail = m  # the reference columns dirty to the end begin here
                while tail and tail - 1 not in taken:
                    tail -= 1
                for c in own_dirty:
                    assert R.inside((c, c), fo, False), (reg["name"], hid, c, fo)
                for c in breaks_own:
                    assert R.inside((c, c - 1), fo, False), (reg["name"], hid, c, fo)
                for q in ref_dirty:
                    assert R.inside((q, q), fq, False) or (q >= tail and R.inside((tail, R.END), fq, fq_end)), \
                        (reg["name"], hid, q, fq)
                for q in breaks_ref:
                    assert R.inside((q, q - 1), fq, False), (reg["name"], hid, q, fq)
                total += 1
    assert total > 1800


def test_single_regions_hold_one_haplotype_per_placed_record():
    b = host_batch("single")
    for r, reg in enumerate(K.family("single")["regions"]):
        assert reg["name"] == K.SINGLE_KINDS[r]
        placed = K.M - K.need(reg["name"]) + 1
        assert len(reg["placed"]) == placed == reg["distinct"] >= 99
        assert b.region_stats(r)[0] == placed + 1  # and the reference
        res = checked("single", r)
        assert all(res[hid][0] for hid in reg["placed"]) and not res[0][0]


def test_pairs_cover_the_distances_and_places():
    regs = K.family("pairs")["regions"]
    assert [reg["name"] for reg in regs] == ["pairs_first", "pairs_middle", "pairs_last"]
    b = host_batch("pairs")
    for r, reg in enumerate(regs):
        assert 200 <= len(reg["placed"]) == reg["distinct"] <= 2048
        assert b.region_stats(r)[0] == reg["distinct"] + 1
        dist, kinds = set(), set()
        for recs in reg["placed"].values():
            assert len(recs) == 2
            (p1, r1, a1), (p2, r2, a2) = recs
            assert p1 + len(r1) <= p2  # they do not overlap
            dist.add(p2 - p1)
            kinds.add((len(r1), len(a1), len(r2), len(a2)))
        assert dist == set(K.DISTANCES)
        # SNV, insertions of two and three bases, deletion: every combination; equal-length
        # insertion-then-deletion and deletion-then-insertion among them
        shapes = {(1, 1), (1, 4), (1, 3), (4, 1)}
        assert kinds == {x + y for x in shapes for y in shapes}
        first = min(p for recs in reg["placed"].values() for p, _, _ in recs) - reg["es"]
        last = max(p + len(rf) - 1 for recs in reg["placed"].values() for p, rf, _ in recs) - reg["es"]
        assert (first == 0) == (reg["name"] == "pairs_first") and (last == K.M - 1) == (reg["name"] == "pairs_last")
    # a later segment back on its own column: some haplotype of insertion and deletion has an own
    # run list that differs from its reference-column list only between the two records
    res = checked("pairs", 1)
    realigned = [v for hid, v in res.items() if hid and v[0] and len(v[1]) == 2 and len(v[2]) == 2 and
                 v[1][1][1] != R.END and v[1] != v[2]]
    assert realigned


@pytest.mark.parametrize("grouped", [False, True])
def test_caps_sit_on_their_edges(grouped):
    b = host_batch("caps", grouped)
    regs = K.family("caps")["regions"]
    assert [reg["name"] for reg in regs[4:]] == ["snv_adjacent", "len_1024", "len_1025"]
    if grouped:  # SNVs alone: grouped as on a device; with an indel: grouped there, patched on the host
        assert b.build_stats() == (len(regs), 0)
    lens = {}
    for r, reg in enumerate(regs[:5]):
        res = checked("caps", r, grouped)
        assert res[1][0] and not res[2][0] and not res[0][0], reg["name"]  # 16 reuses, 17 does not
        lens[reg["name"]] = (len(res[1][1]), len(res[1][2]))
        # the one that does not differs by one SNV, which is one run more in either list
        extra = [rec for rec in reg["placed"][2] if rec not in reg["placed"][1]]
        assert len(extra) == 1 and len(extra[0][1]) == 1 and len(extra[0][2]) == 1
        cols = sorted(p - reg["es"] for p, rf, al in reg["placed"][2] if len(rf) == 1 and len(al) == 1)
        adjacent = sum(1 for x, y in zip(cols, cols[1:]) if y - x == 1)
        assert adjacent == (2 if reg["name"] == "snv_adjacent" else 0)  # (only there do SNV runs merge)
    assert lens == {"snv_16_17": (16, 16), "snv_ins_16_17": (16, 16), "snv_del_to_end": (15, 16),
                    "snv_ins_at_end": (16, 15), "snv_adjacent": (16, 16)}
    assert len(regs[4]["placed"][1]) == 18
    assert all(len(reg["records"]) <= 64 for reg in regs)  # a device groups these regions
    long_, longer = checked("caps", 5, grouped), checked("caps", 6, grouped)
    assert len(regs[5]["codes"]) == 1024 and len(regs[6]["codes"]) == 1025
    assert [long_[hid][0] for hid in (1, 2, 3)] == [False, True, True]  # 1 025 columns | 1 023 | an SNV
    assert len(b.haplotype(5, b.membership(5)[1])[0]) == 1025
    assert not any(v[0] for v in longer.values())
    assert b.layout(5)[2] is not None and b.layout(6)[2] is None


def test_odd_cases_are_what_they_say():
    b = host_batch("odd")
    regs = {reg["name"]: (r, reg) for r, reg in enumerate(K.family("odd")["regions"])}
    r, reg = regs["left_of_window"]
    assert min(p for _, p, _, _, _ in reg["records"]) < reg["es"]
    assert b.haplotype(r, b.membership(r)[1])[:2] == b.haplotype(r, b.membership(r)[0])[:2]  # not applied
    r, reg = regs["two_at_one_position"]
    memb = b.membership(r)
    assert len({memb[0], memb[1], memb[2], memb[3]}) == 4
    assert len(b.haplotype(r, memb[3])[0]) == 46  # the second record truncates it after column 45
    r, reg = regs["overlap_truncates"]
    assert len(b.haplotype(r, b.membership(r)[1])[0]) == 51 and checked("odd", r)[1][2][-1][1] == R.END
    r, reg = regs["n_runs"]
    assert [q for q, c in enumerate(reg["codes"]) if c == 4] == [50, 51, 52, 53, 70]
    assert all(v[0] for hid, v in checked("odd", r).items() if hid in reg["placed"])
    r, reg = regs["everyone_inserts"]
    hb, count, ref_hap, _ = b.layout(r)
    assert ref_hap == hb + count  # no reference group: the helper copy
    assert sorted(reg["placed"]) == list(range(16)) and all(v[0] for v in checked("odd", r).values())
    for name in ("prefix_beside_snvs", "prefix_alone"):
        r, reg = regs[name]
        ok, own, rq = checked("odd", r)[0]
        assert ok and own == [] and rq == [(K.M - 3, R.END)]
    assert b.region_stats(regs["prefix_alone"][0])[0] == 2


@pytest.mark.parametrize("name", K.FAMILIES)
def test_every_family_has_both_kinds_of_list(name):
    """A haplotype whose reference-column list is a list of its own and differs from its own-column
    list (the two accessors differ), in every family; one with an empty own list and a non-empty
    reference-column list among the single records and the odd cases."""
    sep = empty = 0
    for r in range(len(K.family(name)["regions"])):
        for hid, (ok, own, rq) in checked(name, r).items():
            sep += ok and own != rq
            empty += ok and own == [] and rq != []
    assert sep >= 1
    if name in ("single", "odd"):
        assert empty >= 1


def test_own_runs_reject_bad_indices():
    b = host_batch("odd")
    with pytest.raises(Exception):
        b.hap_own_runs(len(K.family("odd")["regions"]), 0)
    with pytest.raises(Exception):
        b.hap_own_runs(0, b.region_stats(0)[0])
    assert b.hap_own_runs(0, 0)[0] == b.hap_runs(0, 0)[0]
