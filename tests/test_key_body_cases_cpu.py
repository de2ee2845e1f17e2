"""key_body_cases.py's regions sit on the edges they are named for: shown from the oracle's keys
and the host batch alone (no device) -- distinct haplotypes U, reference hits nref, diff runs per
haplotype, touched keys T, and the per-haplotype counts of the rows built to be equal, to cancel
or to differ on one haplotype only."""
import pytest

import assembly_cases as A
import key_body_cases as C


def _fig(batch):
    key = C.BATCHES[batch]
    return key, [A.figures(key, r) for r in range(len(key))]


def _runs(key, r):
    b = A.host_batch(key)
    return [b.hap_runs(r, l) for l in range(b.layout(r)[1])]


def test_hit_counts():
    key, figs = _fig("hits")
    st = A.strands("full")
    wide = {"hits70_u140": 140, "hits70_u520": 520}
    assert key[len(C.HIT_COUNTS):] == tuple(wide)
    for r, n in enumerate(C.HIT_COUNTS + (70, 70)):
        f = figs[r]
        per = -(-n // min(n, 16)) if n else 1  # hits per haplotype's run
        assert f["nref"] == n and f["refs_on"] and f["U"] == wide.get(key[r], 1 + max(1, -(-n // per))), (n, f)
        assert f["U"] * max(n, 1) <= A.PAIR_LIMIT  # the pairwise test, not the walk
        hits, runs = A.reference_hits(A.case(key[r])), _runs(key, r)
        # (the reference's own haplotype stands last and is scanned itself; the others reuse, one run each)
        assert all(reuses and 1 <= len(rr) <= 6 for reuses, _, rr in runs[:-1]) and runs[-1][2] == []
        for i, w in hits:  # every hit dirty for exactly one haplotype: a hit left out shows
            assert sum(1 for _, _, rr in runs if any(A.run_meets(a, e, w, st[i][2]) for a, e in rr)) == 1, (n, w)
        bits = {A.range_bits(A.case(key[r]), w, st[i][2]) for i, w in hits}
        assert bits <= {1, 2} and (n < 2 or bits == {1, 2})
    assert C.GROUP == 8 and {7, 8, 9, 63, 64, 65, 128, 256} <= set(C.HIT_COUNTS)
    # no hit shares, so one wave meets all 70 hits: 140 | 520 haplotypes are 3 | 9 blocks of 64, more than half of 4 | 16 waves
    assert 2 * ((140 + 63) // 64) > 4 and 2 * ((520 + 63) // 64) > 16 and 520 > A.BIG_U


def test_haplotype_counts():
    key, figs = _fig("haps")
    assert [f["U"] for f in figs] == list(C.U_COUNTS)
    for r, f in enumerate(figs):
        # (a region of one haplotype scans it and inherits nothing: no reference hit)
        assert (f["nref"] == 0 if f["U"] == 1 else 1 <= f["nref"] <= 64) and f["U"] * f["nref"] <= A.PAIR_LIMIT
        assert any(len(rr) == 0 for _, _, rr in _runs(key, r))  # the reference's haplotype: no run
    # the hit shares' edge: haplotype blocks of 64 fill at most half of 4 | 16 waves
    assert [(u + 63) // 64 * 2 <= 4 for u in (128, 129)] == [True, False]
    assert [(u + 63) // 64 * 2 <= 16 for u in (512, 513)] == [True, False]


def test_runs_ranges_and_the_second_pass():
    key, figs = _fig("misc")
    st = A.strands("full")
    for r, name in enumerate(key):
        runs = _runs(key, r)
        if name.startswith("runs"):
            assert [len(rr) for reuses, _, rr in runs if reuses] == [int(name[4:])] * figs[r]["U"], name
            assert figs[r]["nD"] > 0
        if name == "between":
            flags = [reuses for reuses, _, _ in runs]
            assert flags.count(False) == 1 and flags[0] and flags[-1], flags
        if name.startswith("inner"):
            spec, k = A.case(name), int(name[5:])
            assert figs[r]["n_inner"] == k
            assert max(A.range_bits(spec, w, st[i][2]) for i, w in A.reference_hits(spec)) == k
    # core: a run that meets a hit's window on its first column only, and one on its last only
    r = key.index("core")
    first_only = last_only = False
    for reuses, _, rr in _runs(key, r):
        for i, w in A.reference_hits(A.case("core")):
            L = st[i][2]
            for a, e in rr:
                if L > 1 and a <= e:
                    first_only |= e == w
                    last_only |= a == w + L - 1
    assert first_only and last_only
    f = figs[key.index("listed_3585")]
    assert f["nD"] == A.SHAPES["small"]["cor"] + 1 and f["U"] == 128


def test_row_counts():
    key, figs = _fig("rows")
    want = {"rows127": (48, 127), "rows128": (48, 128), "rows129": (48, 129), "rows256": (24, 256), "rows257": (24, 257)}
    for r, name in enumerate(key):
        f = figs[r]
        if name in want:
            assert (f["U"], f["T"]) == want[name], (name, f)
            assert 4 * (f["lmax"] + 64) < 65536  # packed counters
        else:
            assert f["U"] == int(name[3:]) and f["T"] >= 1, (name, f)
    assert C.rows_per(48) == 128 and C.rows_per(24) == C.ROWS == 256
    # the varying rows of the chunk regions: the first id's 32 keys
    counts = C.hap_counts(key, key.index("rows129"))
    assert sum(1 for c in counts.values() if len(set(c)) > 1) == 32


def _by_id(key, name):
    """{id: its two rows' per-haplotype counts (the same under both ranges)}, the region's figures."""
    r = key.index(name)
    by = {}
    for k, c in C.hap_counts(key, r).items():
        assert by.setdefault(k[2], c) == c
    return by, A.figures(key, r)


def _only(c, at):
    """The counts differ on haplotype `at` alone."""
    rest = c[:at] + c[at + 1:]
    return len(set(rest)) == 1 and c[at] != rest[0]


def test_special_rows():
    key = C.BATCHES["special"]
    N = C.N_IDS
    # (ids 1 and 2: rows 0-3, the chunk's first; ids N - 1 and N: its last)
    for name, ref_only, first_only in (("edge_a", (1, N - 1), (2, N)), ("edge_b", (2, N), (1, N - 1))):
        by, f = _by_id(key, name)
        U = f["U"]
        assert f["T"] == 2 * N <= C.rows_per(U) and len(by) == N and f["nref"] == N and f["refs_on"]
        for pid in ref_only:  # only haplotype U - 1 (the reference's) differs
            assert _only(by[pid], U - 1), (name, pid, by[pid])
        for pid in first_only:  # only haplotype 0 differs
            assert _only(by[pid], 0), (name, pid, by[pid])
        for pid in range(3, N - 1):  # equal and not 0: ANY, not VARIES
            assert by[pid] == [1] * U, (name, pid)
    assert A.figures(key, 0)["U"] % 2 == 1 and A.figures(key, 1)["U"] % 2 == 0
    by, f = _by_id(key, "cancel")
    assert f["T"] == 2 * N and f["nref"] == N and f["refs_on"]
    assert 1 not in by and N not in by and len(by) == N - 2  # the reference's hits, on no haplotype: rows of zeros
    assert len(set(by[20])) == 2 and all(by[p] == [1] * f["U"] for p in by if p != 20)
    # rows 63 | 64 | 65 are ids 32 | 33 | 33: all vary; 64 and 65 do and 63 does not; the other way round
    for name, varying in (("vary_all", range(1, N + 1)), ("vary_ids_odd", range(1, N + 1, 2)), ("vary_ids_even", range(2, N + 1, 2))):
        by, f = _by_id(key, name)
        assert f["T"] == 2 * N <= C.rows_per(f["U"])  # one chunk
        assert [p for p in sorted(by) if len(set(by[p])) > 1] == list(varying), name
    assert 63 // 2 + 1 == 32 and 64 // 2 + 1 == 33 == 65 // 2 + 1
