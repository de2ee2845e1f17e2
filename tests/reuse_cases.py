"""Cases for reference-window reuse across indels (batch.cpp commit_regions: segments, the two
run lists per haplotype, boundary runs), used by test_reuse_cases_cpu.py (no device: the run
lists against reuse_ref's model) and test_gpu_reuse_indels.py (counts, window lists, hits).

One shared window: lmax 32 and a merged range of 40 bases, so 102 columns, bases from a fixed
seed.  A case family is one batch: family(name) -> {"n": samples, "regions": [region dicts for
helpers.build_batch / run_oracle, with "es", "name", "ranges" and "placed" (haplotype id ->
its records) beside]}.  One carrier id per haplotype unless stated; id 0 carries nothing (the
reference group) unless stated.

single  one region per kind of record, the kind placed at every column where it fits.
pairs   two records on one haplotype, both kinds from {SNV, insertion, tandem duplication,
        anchor repeat, deletion}, at distances 1..33 between their first columns, anchored at
        the window's first columns, its middle, and so that the second falls in its last ones
        (one region per anchor place).  Insertion and deletion both have three bases, so after
        insertion-then-deletion and deletion-then-insertion the columns stand at their own
        reference columns again.
caps    16 | 17 runs (SNVs alone, at most 64 records: grouped on the device where there is
        one; SNVs and an insertion: grouped there and patched on the host) and haplotypes
        whose two lists differ in length around the limit: SNVs and a deletion to the last
        base (no own run, a reference-column run to the end: 15 | 16 reuses, 16 | 17 does not)
        and SNVs and an insertion at the last column (an own run to the end, no
        reference-column run: 16 | 15 reuses, 17 | 16 does not); a 1 024-column reference
        with an insertion (1 025 columns: scanned whole) and a deletion (reuses); a
        1 025-column reference (nobody reuses); SNVs alone with two pairs in adjacent columns
        (18 | 19 SNVs: 16 | 17 runs once adjacent columns are merged, which only the device-grouped
        build does column by column).
odd     a record starting left of the window, two records at one position (on two haplotypes,
        and both on a third: the second truncates it), overlapping records, N runs in the
        reference touching indels and inside a segment, an insertion every id carries (no
        reference group: the helper copy), the deletion to the last base beside SNV
        carriers and as the region's only record, and a region of 40 inner ranges (the only one;
        every other region has 16, the two long ones 8) with one haplotype of every kind.
"""
import functools
import random

import reuse_ref as R
from helpers import T

LMAX = 32
WIDTH = 40
M = WIDTH + 2 * (LMAX - 1)  # 102 columns
STEP = 4000
SEED = 20251
DISTANCES = (1, 2, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33)
PAIR_KINDS = ("snv", "ins3", "tandem", "repeat", "del3")
SINGLE_KINDS = ("snv", "ins1", "ins3", "ins3_anchor", "tandem", "repeat", "del1", "del3", "del_to_end",
                "del_past_end")
CENSUS_LENGTHS = (1, 2, 8, 16, 17, 32)
FAMILIES = ("single", "pairs", "caps", "odd")


def _text(codes):
    return "".join("ACGTN"[c] for c in codes)


@functools.lru_cache(None)
def base_ref(m=M, seed=SEED):
    rnd = random.Random(seed)
    return tuple(rnd.randrange(4) for _ in range(m))


# ------------------------------------------------------------------------------------ patterns
def window_scores(w4, codes):
    """Every window's score of a PWM (rows of four weights) on codes 0-4 (N adds 0)."""
    L = len(w4)
    return [sum(w4[j][codes[i + j]] for j in range(L) if codes[i + j] < 4) for i in range(len(codes) - L + 1)]


@functools.lru_cache(None)
def patterns():
    """70 forward strands, each a pattern id of its own: 64 of up to 16 columns and 6 of 17 to 32
    (one matrix-core tile of either depth class).  Census strands (every weight 1, min_score 0:
    every window with a base other than N hits) of 1, 2, 8, 16, 17 and 32 columns; the others
    random weights with the median of the shared reference window's scores as threshold."""
    rnd = random.Random(SEED + 1)
    ref = base_ref()
    lengths = [1, 2, 8, 16] + [rnd.choice((1, 2, 3, 5, 7, 8, 9, 12, 15, 16)) for _ in range(60)]
    lengths += [17, 32, 17, 24, 31, 32]
    assert sum(1 for L in lengths if L <= 16) == 64 and sum(1 for L in lengths if L > 16) == 6
    seen, pats = set(), []
    for i, L in enumerate(lengths):
        if L in CENSUS_LENGTHS and L not in seen:
            seen.add(L)
            w4, thr, name = [[1, 1, 1, 1]] * L, 0, "census%d" % L
        else:
            w4 = [[rnd.randint(-3000, 1000) for _ in range(4)] for _ in range(L)]
            sc = sorted(window_scores(w4, ref))
            thr, name = sc[len(sc) // 2], "r%d_%d" % (i, L)
        pats.append(T.Pattern.PWM([T.Weight(*r) for r in w4], name, i + 1, thr, 0))
    assert seen == set(CENSUS_LENGTHS)
    return tuple(pats)


def census_ids():
    """{pattern id: length} of the census strands."""
    return {p.pattern_id: len(p.weights) for p in patterns() if p.name.startswith("census")}


@functools.lru_cache(None)
def pattern_set():
    ps = T.PatternSet.from_patterns(list(patterns()))
    assert ps.max_length == LMAX
    return ps


# ------------------------------------------------------------------------------------- records
def need(kind):
    """Reference columns from the record's first that must exist for it to be built."""
    # (a deletion past the end placed at the last column deletes nothing inside the window)
    return {"tandem": 3, "del1": 2, "del3": 4, "del_to_end": 2, "del_past_end": 2}.get(kind, 1)


def record(ref, c, kind, rnd):
    """(column, REF codes, ALT codes) of a record of `kind` at column c of ref."""
    a = ref[c]
    other = lambda x, k=1: (x + k) % 4 if x < 4 else 0
    if kind == "snv":
        return c, (a,), (other(a),)
    if kind == "ins1":
        return c, (a,), (a, other(a, 2))
    if kind == "ins3":  # (its last base is not the anchor's: that is ins3_anchor)
        return c, (a,), (a, rnd.randrange(4), rnd.randrange(4), other(a, 1 + rnd.randrange(3)))
    if kind == "ins3_anchor":  # ends in the anchor's base: the second alignment, which is rejected
        return c, (a,), (a, other(a), other(a, 2), a)
    if kind == "tandem":  # the next two reference bases again
        return c, (a,), (a, ref[c + 1], ref[c + 2])
    if kind == "repeat":
        return c, (a,), (a, a, a)
    if kind == "del1":
        return c, tuple(ref[c:c + 2]), (a,)
    if kind == "del3":
        return c, tuple(ref[c:c + 4]), (a,)
    if kind == "del_to_end":
        return c, tuple(ref[c:]), (a,)
    if kind == "del_past_end":
        return c, tuple(ref[c:]) + (0, 1, 2), (a,)
    raise KeyError(kind)


def tiles(s, width, count=None):
    """The merged range [s, e = s + width - 1] cut into tiles of 1, 2, 3 and 5 bases in turn (at most
    32; the last one takes what is left), so that every position is told apart.  An inner range
    is selected only if it holds an end of the merged range (select_inner_peaks, main.rs:62-72:
    a tile inside it never is), so tile [lo, hi] stands as the prefix (s, hi) or, every other one,
    as the suffix (hi + 1, e): a cut at every tile's end.  Or `count` ranges (40): the prefixes (s, s + k).  A
    range longer than the shared window's (the length caps) gets 8 tiles, all as prefixes."""
    e = s + width - 1
    if count is not None:
        assert count <= width
        return [(s, s + k) for k in range(count)]
    most = 32 if width <= WIDTH else 8
    out, at = [], s
    while at <= e:
        w = (1, 2, 3, 5)[len(out) % 4]
        hi = e if len(out) == most - 1 else min(at + w - 1, e)
        out.append((hi + 1, e) if len(out) % 2 and most == 32 and hi < e else (s, hi))
        at = hi + 1
    assert len(out) <= most and len(set(out)) == len(out)
    return out


def region(name, index, ref, haps, n_ranges=None, carriers=None):
    """haps: [[(column, REF, ALT), ...]] -- haplotype id k + 1 carries haps[k] (carriers: id lists
    instead).  Haplotypes equal to an earlier one or to the reference are the generator's error."""
    m = len(ref)
    s = 50000 + STEP * index
    es = s - LMAX + 1
    width = m - 2 * (LMAX - 1)
    per = {}
    placed = {}
    seen = {(tuple(ref), tuple(range(es, es + m)))}
    for k, recs in enumerate(haps):
        ids = carriers[k] if carriers else [k + 1]
        absolute = [(es + c, r, a) for c, r, a in recs]
        for hid in ids:
            placed.setdefault(hid, []).extend(absolute)
        for c, r, a in recs:
            per.setdefault((es + c, r, a), set()).update(ids)
    for hid, recs in placed.items():
        nuc, pos, _, _ = R.patch(ref, es, recs)
        if not carriers:
            assert (nuc, pos) not in seen, (name, hid)
        seen.add((nuc, pos))
    records = [("car", p, _text(r), _text(a), sorted(ids)) for (p, r, a), ids in sorted(per.items())]
    return {"name": name, "merged": (s, s + width - 1), "ref": _text(ref), "codes": tuple(ref), "es": es,
            "records": records, "placed": placed, "ranges": tiles(s, width, n_ranges), "distinct": len(seen) - 1}


# -------------------------------------------------------------------------------------- families
def _single():
    ref = base_ref()
    out = []
    for j, kind in enumerate(SINGLE_KINDS):
        rnd = random.Random(SEED + 10 + j)
        haps = [[record(ref, c, kind, rnd)] for c in range(M - need(kind) + 1)]
        out.append(region(kind, j, ref, haps))
    return out


def _footprint(kind):
    return {"del3": 4}.get(kind, 1)


def _pairs():
    ref = base_ref()
    out = []
    for j, place in enumerate(("first", "middle", "last")):
        rnd = random.Random(SEED + 30 + j)
        haps, seen = [], set()
        for k1 in PAIR_KINDS:
            for k2 in PAIR_KINDS:
                for d in DISTANCES:
                    if d < _footprint(k1):
                        continue  # the second would start inside the first's REF
                    c2max = M - need(k2)
                    c1 = {"first": 0, "middle": 40, "last": c2max - d}[place]
                    if c1 < 0 or c1 + d > c2max or c1 + need(k1) > M:
                        continue
                    recs = [record(ref, c1, k1, rnd), record(ref, c1 + d, k2, rnd)]
                    key = R.patch(ref, 0, recs)[:2]
                    if key in seen:  # (a tandem duplication of a repeated base is the anchor repeat)
                        continue
                    seen.add(key)
                    haps.append(recs)
        assert 200 <= len(haps) <= 2048, len(haps)
        out.append(region("pairs_" + place, j, ref, haps))
    return out


def _snv_sites(ref, count, first=4, step=2):
    return [record(ref, first + step * t, "snv", None) for t in range(count)]


def _caps():
    ref = base_ref()
    rnd = random.Random(SEED + 50)
    out = []
    # ids 1 and 2 carry `common`, id 2 one more SNV
    def edge(name, j, common_sites, extra):
        sites = _snv_sites(ref, common_sites + 1)
        common = sites[:common_sites] + extra
        haps = [[rec] for rec in common] + [[sites[common_sites]]]
        carriers = [[1, 2]] * len(common) + [[2]]
        return region(name, j, ref, haps, carriers=carriers)

    out.append(edge("snv_16_17", 0, 16, []))
    out.append(edge("snv_ins_16_17", 1, 15, [record(ref, 60, "ins3", rnd)]))
    out.append(edge("snv_del_to_end", 2, 15, [record(ref, M - 5, "del_to_end", rnd)]))
    out.append(edge("snv_ins_at_end", 3, 15, [record(ref, M - 1, "ins3", rnd)]))
    # SNVs alone, two pairs of them in adjacent columns: 18 | 19 SNVs are 16 | 17 runs once merged
    sites = [record(ref, c, "snv", None) for c in (4, 5, 8, 9)] + _snv_sites(ref, 15, first=12)
    out.append(region("snv_adjacent", 4, ref, [[rec] for rec in sites], carriers=[[1, 2]] * 18 + [[2]]))
    long_ref = base_ref(1024, SEED + 2)
    out.append(region("len_1024", 5, long_ref, [[record(long_ref, 500, "ins1", rnd)], [record(long_ref, 700, "del1", rnd)],
                                                [record(long_ref, 300, "snv", rnd)]]))
    longer = base_ref(1025, SEED + 3)
    out.append(region("len_1025", 6, longer, [[record(longer, 500, "ins1", rnd)], [record(longer, 700, "del1", rnd)],
                                              [record(longer, 300, "snv", rnd)]]))
    return out


def _odd():
    ref = base_ref()
    rnd = random.Random(SEED + 70)
    H = 16
    out = []
    # a deletion starting two bases left of the window (not applied: its carrier keeps the reference)
    left = (-2, (0, 1) + tuple(ref[:3]), (0,))
    out.append(region("left_of_window", 0, ref, [[left], [record(ref, 40, "snv", rnd)], [record(ref, 0, "ins3", rnd)]],
                      carriers=[[1], [2], [3]]))
    a = ref[45]
    two = [(45, (a,), ((a + 1) % 4,)), (45, (a,), ((a + 2) % 4,))]
    out.append(region("two_at_one_position", 1, ref, [[two[0]], [two[1]]], carriers=[[1, 3], [2, 3]]))
    out.append(region("overlap_truncates", 2, ref, [[record(ref, 50, "del3", rnd), record(ref, 52, "snv", rnd)],
                                                    [record(ref, 50, "del3", rnd)],
                                                    [record(ref, 60, "ins3", rnd), record(ref, 60, "snv", rnd)]]))
    nref = list(ref)
    for q in (50, 51, 52, 53, 70):
        nref[q] = 4
    nref = tuple(nref)
    out.append(region("n_runs", 3, nref, [[record(nref, 49, "ins3", rnd)], [record(nref, 54, "del3", rnd)],
                                          [(47, tuple(nref[47:50]), (nref[47],))],  # (deletes 48 and 49: the N run follows)
                                          [record(nref, 20, "snv", rnd)], [record(nref, 30, "ins1", rnd)],
                                          [record(nref, 66, "del3", rnd)], [record(nref, 71, "repeat", rnd)]]))
    everyone = record(ref, 44, "ins3", rnd)
    out.append(region("everyone_inserts", 4, ref, [[everyone], [record(ref, 20, "snv", rnd)],
                                                   [record(ref, 80, "del1", rnd)]],
                      carriers=[list(range(H)), [1, 2], [2, 3]]))
    prefix = record(ref, M - 4, "del_to_end", rnd)
    out.append(region("prefix_beside_snvs", 5, ref, [[prefix], [record(ref, 5, "snv", rnd)], [record(ref, 40, "snv", rnd)],
                                                     [record(ref, 77, "snv", rnd)]],
                      carriers=[[0, 3, 6], [1, 2], [2, 4], [5]]))
    out.append(region("prefix_alone", 6, ref, [[prefix]], carriers=[[0, 3, 6]]))
    # 40 inner ranges (the assembly's path past 32), every kind of record among its haplotypes
    kinds = ("snv", "ins1", "ins3", "ins3_anchor", "tandem", "repeat", "del1", "del3", "del_to_end", "del_past_end")
    out.append(region("forty_ranges", 7, ref, [[record(ref, 28 + 7 * k, kind, rnd)] for k, kind in enumerate(kinds)],
                      n_ranges=40))
    return out


@functools.lru_cache(None)
def family(name):
    regions = {"single": _single, "pairs": _pairs, "caps": _caps, "odd": _odd}[name]()
    ids = max(max(reg["placed"]) for reg in regions) + 1
    n = {"odd": 8}.get(name, (ids + 1) // 2)
    assert 2 * n >= ids
    return {"name": name, "n": n, "regions": regions}


def beds(regions):
    return [("reuse.bed", [r for reg in regions for r in reg["ranges"]])]


def alone(name):
    """The two regions of a family that are also run alone in a batch."""
    return {"single": (3, 8), "pairs": (0, 2), "caps": (2, 5), "odd": (4, 6)}[name]


# ------------------------------------------------------------------- the invariants on a batch
LENGTHS = (1, 2, 8, 15, 16, 17, 31, 32)
MAX_RUNS = 16


def ids_of(b, r):
    """{distinct index: [haplotype ids]} of region r."""
    out = {}
    for hid, h in enumerate(b.membership(r)):
        out.setdefault(h, []).append(hid)
    return out


def check_form(runs):
    """I3: ascending, merged (a run starts past the previous b + 1), at most 16, a run to the end
    only last, a boundary run exactly (a, a - 1)."""
    assert len(runs) <= MAX_RUNS, runs
    for k, (a, b) in enumerate(runs):
        assert b == R.END or b + 1 >= a, runs  # a proper run, or the boundary (a, a - 1)
        assert b != R.END or k == len(runs) - 1, runs
        if k:
            pb = runs[k - 1][1]
            assert pb != R.END and a > pb + 1, runs


def check_haplotype(b, r, reg, h, ids, lengths=LENGTHS):
    """I1-I4 (reuse_ref.py, DESIGN.md "Across indels") for distinct haplotype h of region r, whose
    carrier ids are `ids`; returns (reuses, own runs, reference-column runs)."""
    ref, es = reg["codes"], reg["es"]
    m = len(ref)
    nuc, pos, _ = b.haplotype(r, h)
    n = len(nuc)
    want_nuc, want_pos, applied, truncated = R.patch(ref, es, reg["placed"].get(ids[0], []))
    assert (nuc, pos) == (want_nuc, want_pos), (reg["name"], h)
    reuses, off, own = b.hap_own_runs(r, h)
    reuses_q, off_q, rq = b.hap_runs(r, h)
    assert reuses == reuses_q
    if not reuses:
        assert own == [] and rq == []
        return False, own, rq
    check_form(own)
    check_form(rq)
    if off != off_q:  # a list of its own behind the haplotype's (equal offsets: one list, or no own run)
        assert off_q == off + len(own)
    # I4: either list within the records' footprints
    fq, fq_end, fo, fo_end = R.footprints(applied, truncated, m, n)
    for run in rq:
        assert R.inside(run, fq, fq_end), (reg["name"], h, "reference columns", run, fq)
    for run in own:
        assert R.inside(run, fo, fo_end), (reg["name"], h, "own columns", run, fo)
    for L in lengths:
        # I1: a window that meets no own run is a reference window
        image = {}
        for w in range(n - L + 1):
            if R.meets(own, w, L):
                continue
            q = R.equal_window(ref, es, nuc, pos, w, L)
            assert q is not None, (reg["name"], h, L, w, own)
            assert q not in image, (reg["name"], h, L, w, image[q])  # I2: injective
            image[q] = w
        # I2: onto the reference windows that meet no reference-column run
        passed_on = {q for q in range(m - L + 1) if not R.meets(rq, q, L)}
        assert set(image) == passed_on, (reg["name"], h, L, sorted(set(image) ^ passed_on), own, rq)
    return True, own, rq


def check_region(b, r, reg, lengths=LENGTHS):
    """check_haplotype over region r; {haplotype id: (reuses, own runs, reference-column runs)}."""
    out = {}
    for h, ids in sorted(ids_of(b, r).items()):
        res = check_haplotype(b, r, reg, h, ids, lengths)
        for hid in ids:
            out[hid] = res
    return out
