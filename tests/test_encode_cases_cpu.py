"""encode_cases.py's cases sit on the edges they are named for -- shown with the oracle
alone (its rows and keys) and the generator's own (left level, right level) lists, so
that a case that drifts off its edge fails here and cannot pass vacuously on the GPU
(test_gpu_encode_edges.py)."""
import pytest

import encode_cases as E


def _rows(name, min_maf=0):
    return [r for r in E.oracle(name, min_maf)[1].split("\n") if r]


def _counts(row):
    return [int(x) for x in row.split("\t")[7].split(";")[0].split("=")[1].split(",")]


def _texts(row):
    return row.split("\t")[9:]


def _runs(texts):
    """Maximal runs of equal sample texts: (text, first sample, samples)."""
    out, i = [], 0
    while i < len(texts):
        j = i
        while j < len(texts) and texts[j] == texts[i]:
            j += 1
        out.append((texts[i], i, j - i))
        i = j
    return out


def test_encode_stats_are_zero_before_an_encode():
    b = E.T.RegionBatch(E.pattern_set(1), 4)
    assert b.encode_stats() == {k: 0 for k in ("keys", "w2", "w4", "w8", "no_pairs", "range", "values")}


def test_the_case_list_covers_the_issue():
    names = E.names()
    for nv in (2, 4, 5, 16, 17, 255, 256, 257):
        mods = {E.case(n)["n_samples"] % 4 for n in names if n.startswith("vals_%d_" % nv)}
        assert mods - {0}, nv  # each value count at an n with a packed tail
    sizes = {E.case(n)["n_samples"] for n in names if n.startswith("vals_")}
    assert {2, 3, 5, 63, 65, 513} <= sizes
    assert {s % 4 for s in sizes} == {0, 1, 2, 3}
    for want in ("range_65535", "range_65536", "pairs_8192_sorted", "pairs_8192_shuffled", "pairs_8193_sorted",
                 "pairs_8193_shuffled", "mult_2", "mult_3", "maf", "runs_w4", "runs_w8", "round_robin_w4",
                 "round_robin_w8", "block_value_texts", "block_encoded_rows", "block_tiny_rows"):
        assert want in names
    for c in E.cases():  # no case without a path assertion
        assert len(E.region_paths(c)) == len(c["regions"])
        assert all(p in ("w2", "w4", "w8", "values", "range", "no_pairs") for p in E.region_paths(c))


@pytest.mark.parametrize("name", E.names())
def test_case_has_its_property(name):
    c = E.case(name)
    keys, _ = E.oracle(name)
    rows = _rows(name)
    P = c["prop"]
    n = c["n_samples"]
    assert len(keys) == len(c["regions"])
    assert len(rows) == len(c["regions"]) * c["n_ids"]  # every key varies: one row each
    for r in rows:
        assert len(_texts(r)) == n
    # the generator's totals are the oracle's: per region and pattern_id, COUNTS= holds exactly the
    # distinct totals, shifted by a constant (the reference haplotype's count, times the multiplicity)
    per_region = [rows[j * c["n_ids"]:(j + 1) * c["n_ids"]] for j in range(len(c["regions"]))]
    for spec, rws, rk, path in zip(c["regions"], per_region, keys, E.region_paths(c)):
        red = sorted({E.reduction(a) + E.reduction(b) for a, b in spec["pairs"]})
        n_pairs = E.pair_count(spec)
        for row in rws:
            cnt = _counts(row)
            if spec["kind"] == "mix" or c["n_ids"] == 1:
                assert [cnt[-1] - x for x in reversed(cnt)] == [c["mult"] * d for d in red]
        assert len(rk) == c["n_ids"]
        for (left, right) in rk.values():
            assert E.key_path(left, right, n_pairs) == path
            tot = [a + b for a, b in zip(left, right)]
            assert [max(tot) - t for t in tot] == [c["mult"] * (E.reduction(a) + E.reduction(b)) for a, b in spec["pairs"]]
    spec, row = c["regions"][0], rows[0]
    cnt = _counts(row)
    if "n_vals" in P:
        assert len(cnt) == P["n_vals"]
    if "range" in P:
        assert cnt[-1] - cnt[0] == P["range"]
    if "n_mod4" in P:
        assert n % 4 == P["n_mod4"]
    if P.get("words"):  # totals at lo + 31, + 32, + 33: both sides of the bitmap's first word boundary
        assert {cnt[0] + 31, cnt[0] + 32, cnt[0] + 33} <= set(cnt)
    if P.get("same_total"):  # one total from (a, b), (b, a) and from another split
        by_total = {}
        for a, b in spec["pairs"]:
            by_total.setdefault(E.reduction(a) + E.reduction(b), set()).add((a, b))
        assert any(len(v) >= 2 for v in by_total.values())
        assert any((b, a) in v for v in by_total.values() for (a, b) in v if a != b)
    if "spread_words" in P:  # more words than one thread of key_encode_kernel ranks (8 of 2 048), all over the bitmap
        words = {(x - cnt[0]) // 32 for x in cnt}
        assert max(words) - min(words) > P["spread_words"]
        assert len({w // 8 for w in words}) >= 10  # ten threads' shares hold a value: the cross-thread prefix
        assert (cnt[-1] - cnt[0]) // 32 == (2047 if P["range"] == 65535 else 2048)
    if "n_pairs" in P:
        assert E.pair_count(spec) == P["n_pairs"]
        assert len(spec["pairs"]) == P["n_pairs"] + 100  # repeated pairs: sample counts > 1
        assert spec["pairs"].count((E.snv(0), E.snv(0))) == 41
        adjacent = sum(1 for a, b in zip(spec["pairs"], spec["pairs"][1:]) if a == b)
        if P["order"] == "sorted":  # equal pairs side by side, from a wave's first lane on
            assert adjacent >= 99 and len(set(spec["pairs"][:41])) == 1
        else:
            assert adjacent < 5
    if "mult" in P:
        assert P["mult"] == c["mult"] and E.materialize(c)[2][0][1].count(E.materialize(c)[3][0]["merged"]) == c["mult"]
        assert [len(_counts(r)) for r in rows] == [10, 30]
    if "row_bytes" in P:
        assert len(rows) == P["rows"]
        for r in rows:
            assert P["row_bytes"][0] <= len(r) + 1 <= P["row_bytes"][1]


def test_min_maf_keeps_and_drops_the_row():
    rows = _rows("maf")
    mafs = sorted(E.maf_of(r) for r in rows)
    assert mafs[0] < mafs[1] == E.maf_threshold()
    assert len(_rows("maf", mafs[1])) == 1      # min_maf = maf: the row stays, the other is dropped
    assert len(_rows("maf", mafs[1] + 1)) == 0  # maf + 1: dropped
    assert len(_rows("maf", mafs[0])) == 2


@pytest.mark.parametrize("width", [4, 8])
def test_sorted_runs(width):
    row = _rows("runs_w%d" % width)[0]
    texts = _texts(row)
    runs = _runs(texts)
    by_len = {}
    for t, start, length in runs:
        by_len.setdefault((len(t) + 1, length), []).append((t, start))
    for n8 in (32, 33):  # 256 and 264 bytes around the 258-byte match, of both 8-byte texts
        assert {t for t, _ in by_len[(8, n8)]} == {E.LO_TEXT, E.HI_TEXT}
    assert (11, 23) in by_len and (11, 24) in by_len  # 253 and 264 bytes
    for length in (960, 961):  # the 15-group run item and its successor, off a group boundary
        assert any(l == length and s % 64 for _, s, l in runs)
    assert any(l > 1024 and s % 64 for _, s, l in runs)
    # a run across the first block boundary of the case's own stream (the row starts it)
    head = len(row) - sum(len(t) + 1 for t in texts)
    off = [head]
    for t in texts:
        off.append(off[-1] + len(t) + 1)
    assert any(off[s] < E.BLOCK_TEXT < off[s + l] and l > 100 for _, s, l in runs)
    assert len(row) + 1 > E.BLOCK_TEXT
    assert len(_counts(row)) == (12 if width == 4 else 40)


@pytest.mark.parametrize("width", [4, 8])
def test_round_robin_periods(width):
    row = _rows("round_robin_w%d" % width)[0]
    texts = _texts(row)
    nv = len(_counts(row))
    assert nv == (12 if width == 4 else 40) and len(row) + 1 > E.BLOCK_TEXT
    at = nv
    for period, count in ((2, 2000), (8, 2400), (9, 2700)):
        seg = texts[at:at + count]
        assert len(set(seg[:period])) == period  # distinct texts: a look-back hit at distance period only
        assert all(seg[i] == seg[i - period] for i in range(period, count))
        assert {E.LO_TEXT, seg[0]} <= set(seg) and len({len(t) for t in seg}) == 2  # 8- and 11-byte texts
        at += count
    assert at == len(texts)


def test_shuffled_row_has_no_structure():
    """About 180 distinct texts over 8 292 samples in seeded random order: hardly a repeat
    within the 8 previous texts' reach beyond chance, no runs."""
    row = _rows("pairs_8192_shuffled")[0]
    texts = _texts(row)
    assert len(texts) >= 8000 and len(set(texts)) >= 170 and len(_counts(row)) > 16
    assert max(l for _, _, l in _runs(texts)) <= 4
    assert len(row) + 1 > E.BLOCK_TEXT


def test_block_compositions():
    rows = _rows("block_value_texts")  # > 512 value texts among the rows of the first block
    assert sum(len(_counts(r)) for r in rows[:3]) > 512 and sum(len(r) + 1 for r in rows[:2]) < E.BLOCK_TEXT
    rows = _rows("block_encoded_rows")  # > 8 rows with genotype text in the first block
    assert sum(len(r) + 1 for r in rows[:9]) < E.BLOCK_TEXT
    runs = {(len(t) + 1, l) for t, _, l in _runs(_texts(rows[0]))}  # runs around the 258-byte match there too
    assert {(8, 40), (8, 33), (8, 32), (11, 24), (11, 23), (11, 30)} <= runs
    rows = _rows("block_tiny_rows")  # > 96 rows in one block, one of them with 8-bit codes
    assert len(rows) > 96 and sum(len(r) + 1 for r in rows) < E.BLOCK_TEXT
    widths = [E.width_of(len(_counts(r))) for r in rows]
    assert widths.count("w8") == 12 and set(widths) == {"w2", "w8"}


def test_mixed_batch_puts_fallbacks_between_encoded_regions():
    ps, n, beds, regions, where = E.mixed()
    assert n == E.N_MIX and len(regions) == sum(len(c["regions"]) for c in E.cases())
    assert sorted({w[0] for w in where}) == sorted(E.names())
    paths = [E.region_paths(E.case(name))[j] for name, j, _ in where]
    fb = [i for i, p in enumerate(paths) if p in E.FALLBACK_PATHS]
    assert {paths[i] for i in fb} == set(E.FALLBACK_PATHS)
    for i in fb:
        assert 0 < i < len(paths) - 1
        assert paths[i - 1] not in E.FALLBACK_PATHS and paths[i + 1] not in E.FALLBACK_PATHS
    # the padded sample lists keep every region on its path
    keys, rows = E.oracle("mixed")
    for (name, j, r), path in zip(where, paths):
        (left, right), = keys[r].values()
        assert E.key_path(left, right, E.pair_count(E.case(name)["regions"][j])) == path
    assert len([x for x in rows.split("\n") if x]) == len(regions)
