"""Shared windows (window_lists.hip "Shared windows", TFBS_SHARE): a dirty window of an
SNV-only HAP_DEDUP haplotype is listed only for the lowest-indexed haplotype of the
region that has the same window (its donor), and the rescoring lists a donor's hits
for its sharers.  Hand-built small regions against the oracle (keys and rows), the
same with TFBS_SHARE=0, and the window lists' sizes against a brute-force count made
here from the regions' haplotypes: distinct (region, class, window, bases) among the
haplotypes that may share, plus every window of the others."""
import pytest

from helpers import T, build_batch, make_regions_synth, run_oracle, synth_patterns
from helpers import depth_classes as _classes, window_list_entries as _lists

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


def _haplotypes(reg, H):
    """The region's distinct haplotype sequences (SNV records applied per carrier) and
    the set of those that carry an indel record (not modelled further)."""
    ref = reg["ref"]
    per = [[] for _ in range(H)]
    for rec in reg["records"]:
        assert rec[0] == "car"
        for h in rec[4]:
            per[h].append(rec)
    seqs, indel = set(), set()
    for h in range(H):
        q = list(ref)
        bad = False
        for (_, pos, rf, alt, _) in per[h]:
            if len(rf) != 1 or len(alt) != 1:
                bad = True
            else:
                q[pos - reg["es"]] = alt
        if bad:
            indel.add(h)
        else:
            seqs.add("".join(q))
    return seqs, indel


def _model(ps, regions, H):
    """Brute force: per class the entries the lists hold with sharing (None when a region
    has indel haplotypes, whose own lists are not modelled), the entries sharing removes,
    and the (window, pattern) pairs the scan reads (None likewise)."""
    classes, longer = _classes(ps)
    listed, removed, scan_windows = [0, 0], [0, 0], 0
    exact = True
    for reg in regions:
        ref = reg["ref"]
        n = len(ref)
        seqs, indel = _haplotypes(reg, H)
        exact = exact and not indel and ref in seqs
        for L, k in longer.items():
            scan_windows += k * len(seqs) * max(0, n - L + 1)
        for c, cl in enumerate(classes):
            if cl is None:
                continue
            lmin, S, lens = cl
            nw = n - lmin + 1
            distinct, unshared = set(), []  # (window, bases) of the sharing haplotypes | others' windows
            n_elig = 0
            for q in seqs:
                cols = [p for p in range(n) if q[p] != ref[p]]
                runs = sum(1 for t, p in enumerate(cols) if t == 0 or cols[t - 1] + 1 != p)
                if q == ref or runs > 16 or n > 1024:  # the reference, or scanned whole
                    unshared.extend(range(nw))
                    continue
                dirty = sorted({i for p in cols for i in range(max(0, p - S + 1), min(p, nw - 1) + 1)})
                if "N" in q:
                    unshared.extend(dirty)
                    continue
                n_elig += len(dirty)
                distinct.update((i, q[i:i + S]) for i in dirty)
            listed[c] += len(unshared) + len(distinct)
            removed[c] += n_elig - len(distinct)
            for L, k in lens.items():
                scan_windows += k * (sum(1 for i in unshared if i <= n - L) + sum(1 for i, _ in distinct if i <= n - L))
    return (listed if exact else None), removed, (scan_windows if exact else None)


def _check(monkeypatch, ps, n_samples, beds, regions, modes=((False, False), (True, True))):
    """Oracle == product with shared windows (dense download, and the device reduction +
    encoding) == product with TFBS_SHARE=0; the lists' sizes == the brute-force model's.
    Returns (entries shared, entries unshared, model)."""
    okeys, orows, _ = run_oracle(ps, n_samples, beds, regions)
    model = _model(ps, regions, 2 * n_samples)
    sc = T.Scanner(ps)
    ent = {}
    try:
        for share in ("1", "0"):
            monkeypatch.setenv("TFBS_SHARE", share)
            for reduce, encode in (modes if share == "1" else modes[-1:]):
                b = build_batch(ps, n_samples, beds, regions)
                before = b.num_scan_windows
                b.scan(sc, reduce=reduce, encode=encode)
                ent[share] = _lists(sc)
                for i, want in enumerate(okeys):
                    got = b.keys(i)
                    assert want.keys() == got.keys(), (share, reduce, i)
                    for k in want:
                        assert want[k] == got[k], (share, reduce, i, k)
                rows, _ = b.rows("chr1", 0)
                assert rows == orows, (share, reduce, encode)
                print("TFBS_SHARE", share, "entries", ent[share], "scan windows", before, "->", b.num_scan_windows,
                      "model", model)
                if share == "0":
                    assert b.num_scan_windows == before
                elif model[2] is not None:
                    assert b.num_scan_windows == model[2]
    finally:
        sc.close()
        monkeypatch.delenv("TFBS_SHARE", raising=False)
    listed, removed, _ = model
    assert [ent["0"][c] - ent["1"][c] for c in range(2)] == removed
    if listed is not None:
        assert ent["1"] == listed
    return ent["1"], ent["0"], model


def _base(ps, j, n_samples, seed=77):
    r = T.SynthRegion(seed, j, n_samples, ps.max_length, 0)
    s, e = r.merged
    return r.ref, (s, e), s - ps.max_length + 1


def _snv(ref, es, p, car, k=1):
    return ("car", es + p, ref[p], "ACGT"[("ACGT".index(ref[p]) + k) % 4], sorted(car))


def _region(ref, merged, es, recs):
    return {"merged": merged, "ref": ref, "es": es, "records": sorted(recs, key=lambda x: x[1])}


def _patterns(tmp_path, thr=0.05, n_pwms=40):
    """40 PWMs: one depth class (their 80 strands share tiles with the long ones); 300:
    both classes."""
    ps, _ = synth_patterns(tmp_path, n_pwms, 3, 131, thr=thr)
    classes, _ = _classes(ps)
    assert classes[1] and (n_pwms < 300 or classes[0]), classes
    return ps, classes


N_SAMPLES = 20  # 40 haplotype ids


def test_far_pair(tmp_path, monkeypatch):
    """Two sites at least S apart: {a}, {b}, {a, b}: the {a, b} haplotype lists nothing."""
    ps, classes = _patterns(tmp_path, n_pwms=300)
    ref, m, es = _base(ps, 0, N_SAMPLES)
    S = classes[1][1]
    a, b = 70, 70 + S + 3
    reg = _region(ref, m, es, [_snv(ref, es, a, [0, 1, 4, 5]), _snv(ref, es, b, [2, 3, 4, 5])])
    shared, unshared, _ = _check(monkeypatch, ps, N_SAMPLES, [("synthetic.bed", [m])], [reg])
    for c in range(2):
        lmin, Sc, _ = classes[c]
        nw = len(ref) - lmin + 1
        assert shared[c] == nw + 2 * Sc     # the reference's windows, {a}'s and {b}'s
        assert unshared[c] == nw + 4 * Sc   # {a, b} lists both sites' windows again


def test_near_pair(tmp_path, monkeypatch):
    """Two sites closer than the class span but farther apart than the shortest strand:
    windows covering both sites are {a, b}'s own, windows covering one are shared."""
    ps, classes = _patterns(tmp_path, n_pwms=300)
    regs, ranges = [], []
    for c in range(2):
        lmin, S, _ = classes[c]
        d = S - 1
        assert d > classes[0][0]  # farther apart than some strand's L
        ref, m, es = _base(ps, 1 + c, N_SAMPLES)
        regs.append(_region(ref, m, es, [_snv(ref, es, 80, [0, 1, 4, 5]), _snv(ref, es, 80 + d, [2, 3, 4, 5])]))
        ranges.append(m)
    shared, unshared, _ = _check(monkeypatch, ps, N_SAMPLES, [("synthetic.bed", ranges)], regs)
    assert shared[0] < unshared[0] and shared[1] < unshared[1]


def test_same_column_different_alt(tmp_path, monkeypatch):
    """Two records at one position with different alt bases do not share that site's
    windows; a second site far away is shared by both."""
    ps, classes = _patterns(tmp_path)
    ref, m, es = _base(ps, 3, N_SAMPLES)
    S = classes[1][1]
    recs = [_snv(ref, es, 60, [0, 1, 2], 1), _snv(ref, es, 60, [3, 4, 5], 2), _snv(ref, es, 60 + 2 * S, [1, 4, 7])]
    _check(monkeypatch, ps, N_SAMPLES, [("synthetic.bed", [m])], [_region(ref, m, es, recs)])


def test_edge_sites(tmp_path, monkeypatch):
    """Sites within S - 1 of column 0 and of the last window (and past the last window of
    the longer strands): clipping at both ends."""
    ps, classes = _patterns(tmp_path)
    ref, m, es = _base(ps, 4, N_SAMPLES)
    n = len(ref)
    recs = [_snv(ref, es, 2, [0, 1, 2, 3]), _snv(ref, es, n - 3, [2, 3, 4, 5]), _snv(ref, es, n // 2, [1, 3, 5, 7]),
            _snv(ref, es, 0, [8, 9]), _snv(ref, es, n - 1, [9, 10]), _snv(ref, es, n - classes[1][0], [11, 1])]
    _check(monkeypatch, ps, N_SAMPLES, [("synthetic.bed", [m])], [_region(ref, m, es, recs)])


def _many_haplotype_regions(ps, n_samples, extra_ranges=False):
    """Two regions with the same bases and sites, 100 distinct haplotypes each (donors and
    sharers in different 64-haplotype groups), the carriers differing between them."""
    H = 2 * n_samples
    ref, m0, es0 = _base(ps, 6, n_samples)
    sites = [20, 58, 61, 100, 140, 150, 200]
    regs, ranges = [], []
    for j, mul in enumerate((1, 37)):
        m = (m0[0] + 1000 * j, m0[1] + 1000 * j)
        es = es0 + 1000 * j
        recs = [_snv(ref, es, p, [h for h in range(1, 101) if ((h * mul) % 128) >> t & 1]) for t, p in enumerate(sites)]
        regs.append(_region(ref, m, es, recs))
        ranges.append(m)
        if extra_ranges and j == 1:  # 40 nested inner ranges: hits past range 32 go to the spill list
            ranges.extend((m[0], m[0] + 1 + k) for k in range(39))
    assert H > 100
    return regs, ranges


def test_across_groups_and_regions(tmp_path, monkeypatch):
    """More than 64 distinct haplotypes per region (donor and sharer in different groups);
    a second region with the same bases and sites shares nothing with the first."""
    ps, classes = _patterns(tmp_path, n_pwms=300)
    regs, ranges = _many_haplotype_regions(ps, 60)
    shared, unshared, model = _check(monkeypatch, ps, 60, [("synthetic.bed", ranges)], regs)
    first = _model(ps, regs[:1], 120)[0]  # (the second region's windows are mostly the first's)
    assert all(shared[c] > first[c] + (len(regs[0]["ref"]) - classes[c][0] + 1) for c in range(2))


def test_mixed_haplotype_kinds(tmp_path, monkeypatch):
    """Beside SNV sharers: an indel haplotype, a haplotype with an N and one with more
    than 16 diff runs, all carrying a shared site too; they are scanned as before."""
    ps, classes = _patterns(tmp_path)
    ref, m, es = _base(ps, 8, N_SAMPLES)
    n = len(ref)
    many = [30 + 3 * t for t in range(18)]  # 18 runs on haplotype 14 alone
    recs = [_snv(ref, es, 120, [0, 1, 10, 12, 14, 15]), _snv(ref, es, 200, [1, 2, 11, 13, 15]),
            ("car", es + 160, ref[160], ref[160] + "AC", [10, 11]),
            ("car", es + 180, ref[180], "N", [12, 13])]
    recs += [_snv(ref, es, p, [14]) for p in many]
    _check(monkeypatch, ps, N_SAMPLES, [("synthetic.bed", [m])], [_region(ref, m, es, recs)])


def test_small_lists_and_many_inner_ranges(tmp_path, monkeypatch):
    """8 hit-list entries per wave: the sharers' expanded pairs overflow the wave lists into
    the spill path; 40 inner ranges: the expansion of the ranges past 32 (spill records)."""
    monkeypatch.setenv("TFBS_CAND_CAP", "64")
    ps, classes = _patterns(tmp_path)
    regs, ranges = _many_haplotype_regions(ps, 60, extra_ranges=True)
    _check(monkeypatch, ps, 60, [("synthetic.bed", ranges)], regs, modes=((True, False),))


def test_list_sizes_c3_generator(tmp_path, monkeypatch):
    """20 regions of the C3 generator at 2 000 samples: the window lists' entries and
    num_scan_windows after the upload equal the brute-force count (exactly)."""
    ps, classes = _patterns(tmp_path, thr=1e-3)
    regs = make_regions_synth(3, 0, 20, 2000, ps.max_length, 0)
    for reg in regs:
        reg["es"] = reg["merged"][0] - ps.max_length + 1
    beds = [("synthetic.bed", [reg["merged"] for reg in regs])]
    shared, unshared, model = _check(monkeypatch, ps, 2000, beds, regs, modes=((True, False),))
    assert model[0] is not None and model[2] is not None
    assert sum(shared) < sum(unshared)
