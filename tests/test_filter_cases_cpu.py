"""The matrix-core filter pinned on the host (no GPU): the plan a Scanner uploads
(PatternSet.mfma_plan: the FP6 image's bytes, the super tiles, the tiles' rescoring fields) is
decoded by tests/filter_ref.py and checked against the bound's contract column by column --
with the common T0 the plan chose, the scale that follows from it, the clipped digits,
the padding strands and acc0 --, and every case of tests/filter_cases.py is proven to sit
on the edge it claims, from the decoded plan and the oracle alone.  test_gpu_filter.py
then runs the same cases and compares the device's candidate count with the model's."""
import struct

import numpy as np
import pytest

import filter_cases as FC
import filter_ref as F
import oracle_py as O
from helpers import synth_patterns

BUDGETS = (8, 44, 144)


def ceil_div(a, b):
    return -((-a) // b)


def strand_terms(p):
    """(c_j per column, C) of a pattern: c_j = max(0, max_b w_jb)."""
    c = [max(0, max(w.acgtn[:4])) for w in p.weights]
    return c, sum(c)


def expected_slots(patterns):
    """pattern_id -> count slot: groups of one pattern_id in ascending (longest strand,
    pattern_id) order, groups with a strand past 32 columns last."""
    groups = {}
    for p in patterns:
        if p.kind == 0 and len(p.weights):
            groups[p.pattern_id] = max(groups.get(p.pattern_id, 0), len(p.weights))
    order = sorted(groups, key=lambda pid: (groups[pid] > 32, groups[pid], pid))
    return {pid: k for k, pid in enumerate(order)}


def check_plan(fp, patterns):
    """The contract of the uploaded arrays; returns the scales of the real strands."""
    slots = expected_slots(patterns)
    scales, seen = [], []
    spans = sorted((S["img_off"], S["img_off"] + S["img_bytes"]) for S in fp.supers)
    assert spans[0][0] == 0 and spans[-1][1] == len(fp.image), spans
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 == b0, spans  # the images tile the buffer: no gap, no overlap
    tile0 = 0
    for k, S in enumerate(fp.supers):
        tiles = [t for t in fp.tiles if t.sup == k]
        t0 = S["t0"]
        assert -1024 < t0 < 0 and S["nk"] in (2, 4) and S["tile0"] == tile0 and len(tiles) == S["tile_count"] <= 64
        tile0 += len(tiles)
        assert S["img_bytes"] == sum(F.CHUNK_BYTES * t.depth for t in tiles) and S["img_off"] % 4 == 0
        want_acc0 = float(2**23 + (F.FIELD_BIAS - t0) * (1 + 2**F.FIELD_BITS))
        assert S["acc0"] == struct.unpack("<I", struct.pack("<f", want_acc0))[0], (k, hex(S["acc0"]))
        assert F.acc0_value(S["acc0"]) == 2**23 + (1023 - t0) * 2049
        lens = []
        for t in tiles:
            real = [s for s in range(F.STRANDS) if t.orig[s] >= 0]
            assert real == list(range(len(real))) and real, "padding places follow the real ones"
            depth = max(ceil_div(t.length[s], 8) for s in real)
            assert depth == t.depth and S["nk"] - 1 <= depth <= S["nk"], (k, t.index, depth, hex(S["seg"]))
            assert t.depth_class == S["nk"]
            lens += [t.length[s] for s in real]
            for s in range(F.STRANDS):
                if t.orig[s] < 0:  # a padding place: never a hit
                    assert (t.min_score[s], t.length[s]) == (F.INT32_MAX, 0), (t.index, s)
                    check_never(t, s, t0)
                    continue
                p = patterns[t.orig[s]]
                L = len(p.weights)
                assert (t.length[s], t.min_score[s], t.slot[s]) == (L, p.min_score, slots[p.pattern_id]), (t.index, s)
                seen.append(t.orig[s])
                assert not t.codes[s, L:, :].any(), "columns past the strand's are zero"
                c, C = strand_terms(p)
                D = C - p.min_score
                if D <= 0:  # cannot hit: the padding digits
                    check_never(t, s, t0)
                    continue
                scale = max(1, ceil_div(8 * D, -t0))
                scales.append(scale)
                assert (8 * (p.min_score - C)) // scale >= t0, (t.index, s, scale)
                w = np.array([x.acgtn[:4] for x in p.weights], dtype=np.int64)
                mag = -t.d8[s, :L, :]
                assert (mag >= 0).all(), "every digit is <= 0"
                assert (scale * mag <= 8 * (np.array(c)[:, None] - w)).all(), (t.index, s, scale)
                assert mag.max(axis=1).sum() <= F.FIELD_BIAS - t0, (t.index, s)
        assert (S["lmin"], S["lmax"]) == (min(lens), max(lens)), (k, S)
        ends = F.seg_ends(S["seg"])
        assert ends == [sum(1 for t in tiles if t.depth <= d) for d in (1, 2, 3, 4)], (ends, [t.depth for t in tiles])
    want = [i for i, p in enumerate(patterns) if p.kind == 0 and 0 < len(p.weights) <= 32]
    assert sorted(seen) == want, "every strand of up to 32 columns, once"
    order = [(fp.tiles[i].slot[s]) for i in range(len(fp.tiles)) for s in range(F.STRANDS) if fp.tiles[i].orig[s] >= 0]
    assert order == sorted(order), "strands lie in slot order"
    return scales


def check_never(tile, s, t0):
    """Per column, whatever the base: the digits of a strand that cannot hit sum to U <= t0
    on every window without N."""
    mag = -tile.d8[s]
    assert (mag >= 0).all() and mag.min(axis=1).sum() >= -t0, (tile.index, s, t0)


def all_bounds(fp, hap):
    """[(tile, U[window, place])] of a haplotype, every tile over its class's windows."""
    codes = F.base_codes(hap)
    lmin = fp.class_lmin()
    out = []
    for t in fp.tiles:
        nw = F.n_windows(len(codes), lmin[1 if fp.supers[t.sup]["nk"] > 2 else 0])
        if nw:
            out.append((t, F.tile_bounds(t, codes, nw)))
    return out


def oracle_hits(case, hap):
    """{(pattern index, window)} of the oracle's matches."""
    h = [(ch, j) for j, ch in enumerate(hap)]
    return {(i, a) for i, p in enumerate(case.patterns)
            for a, _ in O.matches([w.acgtn for w in p.weights], p.min_score, h)}


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in FC.all_cases()}


@pytest.fixture(scope="module")
def synth_sets(tmp_path_factory):
    """The benchmark's synthetic pattern sets: C2 (10 PWMs of 8-15 columns), C3 (600 of 8-30)
    and C5 (600 of 25-30), exact 1e-4 thresholds, both strands."""
    return {name: synth_patterns(tmp_path_factory.mktemp(name), n, config, seed)[0]
            for name, (n, config, seed) in {"C2": (10, 2, 2), "C3": (600, 3, 3), "C5": (600, 5, 5)}.items()}


@pytest.mark.parametrize("name", ["C2", "C3", "C5"])
def test_synthetic_plans_are_sound(synth_sets, name):
    ps = synth_sets[name]
    patterns = ps.to_list()
    for kb in BUDGETS:
        fp = F.FilterPlan(ps.mfma_plan(kb))
        scales = check_plan(fp, patterns)
        print(name, kb, "KiB:", len(fp.supers), "super tiles, t0", sorted({S["t0"] for S in fp.supers}),
              "scales", min(scales), "..", max(scales))
    # the default budget is the one a Scanner uses
    assert ps.mfma_plan(0) == ps.mfma_plan(44)


def test_case_plans_are_sound(cases):
    for c in cases.values():
        for kb in (c.lds_kb,) + BUDGETS:
            check_plan(F.FilterPlan(c.pset.mfma_plan(kb)), c.patterns)


def test_model_keeps_every_oracle_hit_and_fields_never_borrow(cases):
    """Every oracle hit of a case haplotype is a model candidate; every output word of every
    strand pair keeps both fields in [0, 2048), and the top-bit test of the packed word is
    "U > t0" for both fields."""
    n_hits = 0
    for c in cases.values():
        fp = c.plan
        for name, hap in c.haps.items():
            total, real, _ = F.candidates(fp, hap)
            hits = oracle_hits(c, hap)
            assert hits <= real, (c.name, name, sorted(hits - real)[:5])
            n_hits += len(hits)
            for t, U in all_bounds(fp, hap):
                S = fp.supers[t.sup]
                t0 = S["t0"]
                assert (U <= 0).all() and (U >= t0 - F.FIELD_BIAS).all(), (c.name, name, t.index)
                word = F.acc0_value(S["acc0"]) + U[:, 0::2] + (U[:, 1::2] << F.FIELD_BITS)
                assert ((word >= 2**23) & (word < 2**24)).all()
                assert ((((word >> 10) & 1) == 1) == (U[:, 0::2] > t0)).all()
                assert ((((word >> 21) & 1) == 1) == (U[:, 1::2] > t0)).all()
                assert ((word & 2047) == U[:, 0::2] + F.FIELD_BIAS - t0).all()
                assert (((word >> 11) & 2047) == U[:, 1::2] + F.FIELD_BIAS - t0).all()
    assert n_hits > 20000


def test_field_neighbours(cases):
    """Pairs (2n, 2n + 1) of one output: a field at its minimum (V = 0) beside a true hit at
    V = 1024 and beside a tie at V = 1023, both ways round; a field at its maximum beside a
    tie; a strand the clip loop cut back."""
    c = cases["neighbours"]
    fp = c.plan
    assert len(fp.tiles) == 1 and len(fp.supers) == 1
    t, t0 = fp.tiles[0], fp.supers[0]["t0"]
    assert t0 == c.marks["t0"], "the family is built for the threshold the plan keeps"
    acc0 = fp.supers[0]["acc0"]
    roles = c.marks["roles"]
    assert t.orig[:12] == list(range(12)) and t.orig[12] == -1
    assert roles == ["min", "edge", "clip", "edge", "min", "edge", "min", "edge", "edge", "min", "zero", "edge"]
    vmax = F.FIELD_BIAS - t0
    clip = roles.index("clip")
    phases = set()
    for name, hap in c.haps.items():
        w1, w2 = c.marks["w"][name]
        phases |= {w1 % 32, w2 % 32}
        U = F.tile_bounds(t, F.base_codes(hap), F.n_windows(len(hap), FC.NB_LEN))
        hits = oracle_hits(c, hap)
        V1, V2 = U[w1] + vmax, U[w2] + vmax
        want = {"min": (0, 0), "edge": (1024, 1023), "zero": (vmax, vmax)}
        for s, role in enumerate(roles):
            if role != "clip":
                assert (V1[s], V2[s]) == want[role], (name, s, role, V1[s], V2[s])
            if role == "edge":  # a true hit one unit over the threshold, a tie that is none
                assert (s, w1) in hits and (s, w2) not in hits, (name, s)
        # (min, edge), (edge, min) and (zero, edge) share an output each
        pairs = [(roles[2 * q], roles[2 * q + 1]) for q in (0, 4, 5)]
        assert pairs == [("min", "edge"), ("edge", "min"), ("zero", "edge")]
        # lane half 0 (strand pairs 0-3): no even place fires at W1, the odd places do
        assert not (U[w1, 0:8:2] > t0).any() and (U[w1, 1:8:2] > t0).all()
        for w in (w1, w2):
            for pair in range(6):
                ue, uo = int(U[w, 2 * pair]), int(U[w, 2 * pair + 1])
                word = F.packed(acc0, ue, uo)
                assert F.fields(word) == (ue + vmax, uo + vmax)
                assert F.fires(word) == (ue > t0, uo > t0)
        # the clipped strand: plain rounding (scale 8: a weight of -60 is the digit 60) breaks the budget
        assert (c.patterns[clip].min_score, strand_terms(c.patterns[clip])[1]) == (t0, 0)  # D = |t0|: scale 8
        plain = 60 * FC.NB_LEN
        got = -t.d8[clip, :FC.NB_LEN, 3]
        assert plain > vmax >= got.sum() and (got < 60).all() and 0 <= V1[clip] < 1024
    assert {0, 15, 16, 31} <= phases, phases


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_every_strand_place(cases, n):
    """Each literal strand alone fires at its planted window, and hits; with 64 strands that
    is every place of a tile (16 outputs x 2 lane halves x 2 fields); with 1, 2, 63 and 65 the
    other places are padding strands, and a second tile starts."""
    c = cases["every_place_%d" % n]
    fp = c.plan
    assert len(fp.tiles) == (n + 63) // 64
    hap = c.haps["plain"]
    hits = oracle_hits(c, hap)
    bounds = all_bounds(fp, hap)
    fired_places = set()
    for k, w in enumerate(c.marks["at"]):
        fired = [(t.index, s) for t, U in bounds for s in np.nonzero(U[w] > fp.t0(t))[0]]
        assert fired == [(k // 64, k % 64)] and (k, w) in hits, (k, w, fired)
        fired_places.add(fired[0])
    assert len(fired_places) == n
    if n >= 32:
        assert {0, 15, 16, 31} <= {w % 32 for w in c.marks["at"]}
    n_pad = sum(1 for t in fp.tiles for s in range(64) if t.orig[s] < 0)
    assert n_pad == 64 * len(fp.tiles) - n
    # N: a window whose first column is N is a candidate of every padding strand (its one
    # padding column adds 0), counted by the kernel and never a hit
    hn = c.haps["n"]
    assert [hn[p] for p in c.marks["n_at"]] == ["N"] * len(c.marks["n_at"])
    if n >= 2:
        assert n < 32 or {31, 32} <= set(c.marks["n_at"])  # (two strands: 22 bases)
        total, real, _ = F.candidates(fp, hn)
        windows = [p for p in c.marks["n_at"] if p < F.n_windows(len(hn), FC.EP_LEN)]
        bn = all_bounds(fp, hn)
        for p in windows:
            for t, U in bn:
                for s in range(64):
                    if t.orig[s] < 0:
                        assert U[p, s] == 0 > fp.t0(t)
        assert total - len(real) == n_pad * len(windows) and (n_pad == 0 or total > len(real))
        # N at a planted window's first and at another's last column: candidates that do not hit
        at = c.marks["at"]
        hits_n = oracle_hits(c, hn)
        for k in (0, 1):
            assert (k, at[k]) in real and (k, at[k]) not in hits_n


def test_depths_supers_and_windows(cases):
    c, c8 = cases["depths"], cases["depths@8k"]
    fp = c.plan
    assert [t.depth for t in fp.tiles] == [1, 2, 3, 4] and [S["nk"] for S in fp.supers] == [2, 4]
    lens = {L for t in fp.tiles for L in t.length if L}
    assert {1, 8, 9, 16, 17, 24, 25, 32} <= lens
    assert tuple(fp.class_lmin()) == c.marks["lmin"] == (1, 17)
    per_class = [sum(1 for S in c8.plan.supers if S["nk"] == nk) for nk in (2, 4)]
    assert max(per_class) >= 2, per_class  # 8 KiB: one class spans several super tiles
    seen = [set(), set()]
    for name, hap in c.haps.items():
        n = len(hap)
        for cl in (0, 1):
            seen[cl].add(F.n_windows(n, fp.class_lmin()[cl]))
        hits = oracle_hits(c, hap)
        if n >= 17 and "N" not in hap:  # the last windows, where only the class's shortest strands fit, hit
            assert any(w == n - 17 and len(c.patterns[i].weights) == 17 for i, w in hits), name
        if n >= 1 and "N" not in hap:
            assert any(w == n - 1 and len(c.patterns[i].weights) == 1 for i, w in hits), name
    for cl in (0, 1):
        assert set(c.marks["counts"]) | {0, 1} <= seen[cl], (cl, sorted(seen[cl]))
    assert {len(h) for h in c.haps.values()} >= {0, 1, 16, 17} and len(c.haps["n1100"]) > 1024
    hn = c.haps["withn"]
    assert all(hn[p] == "N" for p in (0, 31, 32, 63, 64, len(hn) - 1))
    assert sum(1 for t in fp.tiles for s in range(64) if t.orig[s] < 0) > 0


def test_super_tiles_with_different_thresholds(cases):
    c = cases["t0mix"]
    t0s = [S["t0"] for S in c.plan.supers]
    print("t0 per super tile:", t0s)
    assert len(set(t0s)) >= 2
    hits = oracle_hits(c, c.haps["h"])
    for S_index in range(len(t0s)):  # planted hits in every super tile
        origs = {o for t in c.plan.tiles if t.sup == S_index for o in t.orig if o >= 0}
        assert any(i in origs for i, _ in hits)


def test_lists_case_overflows_every_list(cases):
    """In one pair of window tiles (64 windows) x the one strand tile, more than 64 lanes
    fire (lane half h holds the strand pairs p with (p >> 2) & 1 == h) and more than 48
    candidates are listed; the whole haplotype lists more than the 8 waves' small lists (8
    LDS + 8 global entries each with TFBS_CAND_CAP=64) plus 16 overflow entries hold."""
    c = cases["lists"]
    fp = c.plan
    assert len(fp.tiles) == 1
    (t, U), = all_bounds(fp, c.haps["n200"])
    fire = U[:64] > fp.t0(t)
    lanes = 0
    for h in (0, 1):
        places = [s for s in range(64) if ((s >> 1) >> 2) & 1 == h]
        lanes += int(fire[:, places].any(axis=1).sum())
    assert lanes > 64 and fire.sum() > 48
    assert (U > fp.t0(t)).sum() > 8 * 16 + 16


def test_scales_case(cases):
    c = cases["scales"]
    scales = check_plan(c.plan, c.patterns)
    never = sum(1 for p in c.patterns if strand_terms(p)[1] - p.min_score <= 0)
    print("scales", sorted(set(scales))[:5], "..", max(scales), "never", never)
    assert min(scales) == 1 and max(scales) >= 10**5 and never >= 5
    spans = {max(abs(x) for w in p.weights for x in w.acgtn) for p in c.patterns}
    assert {1, 7, 8} <= spans and any(900 < s <= 1000 for s in spans) and any(s > 2**19 for s in spans)
    kinds = {(all(x < 0 for w in p.weights for x in w.acgtn[:4]), all(x > 0 for w in p.weights for x in w.acgtn[:4]))
             for p in c.patterns}
    assert {(True, False), (False, True), (False, False)} <= kinds
