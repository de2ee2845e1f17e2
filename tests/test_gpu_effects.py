"""The variant-effect kernel (scan_effects.hip) through RegionBatch.effects: per (record, pattern
strand) the best site touching the record on the REF and on the ALT allele, against the plain
Python restatement (effects_ref.py); the scratch budget; a second opinion from the hit kernel; the
calls' contract; the run flow's and the command line's --effects_output.  The cases are
dinuc_cases.py's, unchanged, and one built here; what is expected comes from the oracle's
patch_haplotype.  Integer work: every comparison is exact."""
import contextlib
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import dinuc_cases as K
import effects_ref as E
import hits_ref as H
import oracle_py as O
from helpers import GOLD, TD, T

pytestmark = pytest.mark.gpu

NUC = "ACGTN"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@contextlib.contextmanager
def scanner(ps):
    sc = T.Scanner(ps)
    try:
        yield sc
    finally:
        sc.close()


def case_patterns(case):
    if "mono" in case:
        return sorted(case["mono"] + case["pats"], key=lambda p: p.pattern_id)
    return case["pats"]


# ------------------------------------------------------------------ the case built here
SPECIAL_LMAX = 33
IDX = {"ins70": 30, "ins_anchor": 50, "two": 70, "n": 80, "snv_n": 81, "del_in": 95, "bad": 97}


@functools.lru_cache(None)
def case_special():
    """One region of 124 reference bases (lmax 33) and 6 samples whose records are: an SNV at the
    window's first base and one at its last (windows clipped at both ends); an insertion of 70
    bases (alt windows in more than one 64-lane chunk); an insertion of three bases equal to the
    anchor (the suffix runs into the prefix: the cap); a deletion running to the window's last
    base (A a prefix of R); a record outside the window; two records at one position; an SNV
    beside an N; a multi-allelic record, a record without carriers and a bad-REF SNV inside a
    deletion that its carriers also carry (the region builds, the record alone does not patch).
    Strands: mono of 1, 8 and 33 columns, dinucleotide of 2 and 32 bases."""
    rnd = random.Random(2310)
    n = 6
    s, e = 70000, 70059
    es, ee = s + 1 - SPECIAL_LMAX, e + SPECIAL_LMAX - 1
    nb = ee - es + 1
    assert nb == 124
    ref = [rnd.randrange(4) for _ in range(nb)]
    ref[IDX["n"]] = 4
    a = IDX["ins_anchor"]
    ref[a + 1] = (ref[a] + 1) % 4  # (the base after the anchor differs from it)
    txt = lambda codes: "".join(NUC[c] for c in codes)
    other = lambda c, k=1: NUC[(c + k) % 4]
    last = nb - 1
    ins70 = txt(rnd.randrange(4) for _ in range(70))
    recs = [
        ("car", es, NUC[ref[0]], other(ref[0]), [0, 3]),
        ("car", es + IDX["ins70"], NUC[ref[30]], NUC[ref[30]] + ins70, [1, 2]),
        ("car", es + a, NUC[ref[a]], NUC[ref[a]] * 4, [4, 5]),
        ("car", es + IDX["two"], NUC[ref[70]], other(ref[70], 1), [6]),
        ("car", es + IDX["two"], NUC[ref[70]], other(ref[70], 2), [7]),
        ("gt", es + 75, 3, NUC[ref[75]], other(ref[75]), [(4, 5)] * n),
        ("car", es + 77, NUC[ref[77]], other(ref[77]), []),
        ("car", es + IDX["snv_n"], NUC[ref[81]], other(ref[81]), [8, 9]),
        ("car", es + IDX["del_in"], txt(ref[95:101]), NUC[ref[95]], [10]),
        ("car", es + IDX["bad"], other(ref[97]), other(ref[97], 2), [10]),
        ("car", es + last - 5, txt(ref[last - 5:]), NUC[ref[last - 5]], [11]),
        ("car", es + last, NUC[ref[last]], other(ref[last]), [2, 9]),
        ("car", ee + 5, "A", "C", [0, 3]),
    ]
    reg = {"merged": (s, e), "ref": txt(ref), "records": recs, "es": es, "ee": ee}
    calib = [c for c in ref if c != 4]
    pats = []
    for pid, L in enumerate((1, 8, 33)):
        w = [[rnd.randint(-2000, 2000) for _ in range(4)] for _ in range(L)]
        thr = K.attained_threshold(K.mono_scores(w, calib), 0.7)
        pats.append(T.Pattern.PWM([T.Weight(*x) for x in w], "m%d" % L, pid, thr, T.DIR_N if pid & 1 else T.DIR_P))
    pats += K.both_strands(rnd, 3, 2, calib, frac=0.7)
    pats += K.both_strands(rnd, 4, 32, calib, frac=0.7)
    beds = [("a.bed", [(s, e)])]
    return {"pats": pats, "n": n, "regions": [reg], "beds": beds}


def get_case(name):
    if name == "special":
        return case_special()
    return getattr(K, name)()


def check_effects(sc, ps, pats, case, **kw):
    """effects() equals the reference list, dense and sorted; returns (batch, tuples, geometry)."""
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"], **kw)
    got = E.as_tuples(b.effects(sc))
    want, geo = E.expected_effects(pats, case["regions"])
    assert len(got) == len(want) == sum(b.region_stats(r)[1] * len(pats) for r in range(b.num_regions))
    for g, w in zip(got, want):
        assert g == w
    assert [x[:3] for x in got] == sorted(set(x[:3] for x in got))  # one record each, sorted
    for r, reg in enumerate(case["regions"]):
        assert b.variants(r) == E.variants(reg)
    return b, got, geo


CASES = ["case_all_kernels", "case_geometry", "case_n_and_indels", "case_wrap", "special"]


@pytest.mark.parametrize("name", CASES)
def test_reference_equality(name):
    """Field by field on every case.  case_geometry's set gets a TFBS_KIND_OTHER pattern on top.
    Each case asserts what it is there for."""
    case = get_case(name)
    pats = case_patterns(case)
    if name == "case_geometry":
        pats = pats + [T.Pattern.OtherPattern("other", 50)]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, got, geo = check_effects(sc, ps, pats, case)
    scored = [x for x in got if x[3] == E.SCORED]
    assert scored
    lens = lambda g: (len(g[0][0]), len(g[1][0]))
    if name == "case_all_kernels":  # a 36-column strand: more than 32 windows per side; indels
        assert any(len(pats[x[2]]) == 36 and x[4] > 32 and x[7] > 32 for x in scored)
        assert any(lens(g)[0] != lens(g)[1] for gr in geo for g in gr.values())
    if name == "case_geometry":  # sides shorter than the strands; the TFBS_KIND_OTHER strand
        other = [i for i, p in enumerate(pats) if p.kind == T.KIND_OTHER]
        assert len(other) == 1
        assert all(x[4:] == E.EMPTY_SIDE + E.EMPTY_SIDE + (0, 0, 0, 0) for x in got if x[2] in other)
        short = [x for x in scored if x[2] not in other and len(pats[x[2]]) > lens(geo[x[0]][x[1]])[0]]
        assert short and all(x[4] == 0 and x[7] == 0 for x in short)
    if name == "case_n_and_indels":  # N inside affected windows; insertions and deletions
        assert any(4 in g[1][0][max(0, g[2] - 19):g[2] + 20] for gr in geo for g in gr.values())
        d = {lens(g)[1] - lens(g)[0] for gr in geo for g in gr.values()}
        assert min(d) < 0 < max(d)
    if name == "case_wrap":  # wrapped sums: weights at INT32_MIN
        assert any(w == K.INT32_MIN for p in pats for row in p.weights for w in row)
    if name == "special":
        reg = case["regions"][0]
        nb = len(reg["ref"])
        var = E.variants(reg)
        assert [v[5] for v in var] == [0, 0, 0, 0, 0, E.MULTIALLELIC, E.NO_CARRIER, 0, 0, E.UNPATCHED, 0, 0, 0]
        g = geo[0]
        by = {(x[1], x[2]): x for x in got}
        L33 = next(i for i, p in enumerate(pats) if len(p) == 33)
        L8 = next(i for i, p in enumerate(pats) if len(p) == 8)
        # SNVs at the first and the last base: one window of any strand, clipped at the ends
        assert (g[0][2], g[0][3]) == (0, nb - 1) and (g[11][2], g[11][3]) == (nb - 1, 0)
        for v, w33, w8 in ((0, 0, 0), (11, nb - 33, nb - 8)):
            for pi, w in ((L33, w33), (L8, w8)):
                assert by[(v, pi)][4] == by[(v, pi)][7] == 1 and by[(v, pi)][6] == by[(v, pi)][9] == w
        # the insertion of 70 bases: the alt windows of a strand take more than one 64-lane chunk
        assert lens(g[1]) == (nb, nb + 70) and by[(1, L33)][7] > 64 and by[(1, L8)][7] == 70 + 7 > 64
        assert by[(1, L33)][4] > 0 and by[(1, L8)][4] == 7  # the reference windows spanning the junction
        # the insertion equal to its anchor: the suffix would run into the prefix
        R, A, a, z = g[2]
        assert a == IDX["ins_anchor"] + 1 and z == len(R[0]) - a
        free = 0
        while free < len(R[0]) and (R[0][-1 - free], R[1][-1 - free]) == (A[0][-1 - free], A[1][-1 - free]):
            free += 1
        assert free > z  # (uncapped, the suffix is longer)
        # the deletion to the window's last base: A is a prefix of R, no alt window
        R, A, a, z = g[10]
        assert A[0] == R[0][:len(A[0])] and a == len(A[0]) and z == 0
        assert all(by[(10, pi)][7] == 0 and by[(10, pi)][4] > 0 for pi in range(len(pats)))
        # the record outside the window: A == R
        assert g[12][0] == g[12][1] and all(by[(12, pi)][4] == by[(12, pi)][7] == 0 for pi in range(len(pats)))
        # two records at one position, each its own alt side
        assert var[3][0] == var[4][0] and g[3][1] != g[4][1]
        # the SNV beside the N: its windows hold the N
        assert g[7][0][0][IDX["n"]] == 4 and g[7][2] == IDX["snv_n"]
        # unscored records hold the sentinel
        assert all(by[(v, pi)][4:] == E.EMPTY_SIDE + E.EMPTY_SIDE + (0, 0, 0, 0) for v in (5, 6, 9)
                   for pi in range(len(pats)))
        assert sorted(len(p) for p in pats) == [1, 2, 2, 8, 32, 32, 33]
        # the region built and its count path is the batch's without variants kept
        plain = T.RegionBatch(ps, case["n"])
        plain.add_bed("a.bed")
        plain.begin(reg["merged"][0], reg["merged"][1], reg["ref"])
        plain.add_inner(0, *reg["merged"])
        for rec in reg["records"]:
            if rec[0] == "car":
                plain.add_record_carriers(*rec[1:])
            else:
                plain.add_record_gt(*rec[1:])
        plain.end()
        assert plain.input_digest(0) == b.input_digest(0)


def test_device_built_batches_keep_their_records():
    """variants() and effects() of batches grouped on the device: SNV-only regions, regions with
    indels patched on the host, and tfbs_synth_fill_batch."""
    case = K.case_all_kernels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, _, _ = check_effects(sc, ps, pats, case, build_device=0)
        assert b.build_stats()[0] > 0 and b.patch_stats() > 0
        case = K.case_geometry()  # SNVs only
        ps2 = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps2) as sc:
        b, _, _ = check_effects(sc, ps2, case["pats"], case, build_device=0)
        assert b.build_stats()[0] > b.patch_stats()
        n = 20
        sb = T.RegionBatch(ps2, n, keep_variants=True, build_device=0)
        sb.synth_fill(5, 0, 3, 30)
        regions = []
        for j in range(3):
            r = T.SynthRegion(5, j, n, ps2.max_length, 30)
            es, ee = sb.ext(*r.merged)
            regions.append({"merged": r.merged, "ref": r.ref, "es": es, "ee": ee,
                            "records": [("car", pos, ref, alt, car) for pos, ref, alt, car in r.records]})
            assert sb.variants(j) == E.variants(regions[-1])
        want, _ = E.expected_effects(case["pats"], regions)
        assert E.as_tuples(sb.effects(sc)) == want


def test_scratch_budget_and_subranges(monkeypatch):
    case = K.case_n_and_indels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        full = b.effects(sc)
        assert len(full) > 100
        for mb in ("0", "0.01", "256"):
            monkeypatch.setenv("TFBS_EFFECTS_SCRATCH_MB", mb)
            assert np.array_equal(b.effects(sc), full), mb
        monkeypatch.delenv("TFBS_EFFECTS_SCRATCH_MB")
        for r0 in range(4):
            for r1 in range(r0, 4):
                part = b.effects(sc, r0, r1)
                assert np.array_equal(part, full[(full["region"] >= r0) & (full["region"] < r1)]), (r0, r1)
        assert np.array_equal(np.concatenate([b.effects(sc, r, r + 1) for r in range(3)]), full)


def single_variant_pairs(case, pats, b, got, geo):
    """(region, variant, strand, haplotype, affected alt windows) of every scored record whose
    single-record sequence A is one of the region's distinct haplotypes."""
    out = []
    for r in range(b.num_regions):
        order = H.library_order(b, r)
        for v, (R, A, a, z) in geo[r].items():
            if A == R or A not in order:
                continue
            h = order.index(A)
            for pi, p in enumerate(pats):
                out.append((r, v, pi, h, E.affected(len(A[0]), len(p), a, z) if len(p) else []))
    return out


def test_second_opinion_from_the_hit_kernel():
    """alt_score > min_score iff the hit list has a hit of that haplotype and strand in an affected
    window; then alt_score is the maximum of those hits' scores, at the lowest such window."""
    with_hit = without = 0
    for name in ("case_all_kernels", "case_n_and_indels", "special"):
        case = get_case(name)
        pats = case_patterns(case)
        ps = T.PatternSet.from_patterns(pats)
        with scanner(ps) as sc:
            b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
            got = E.as_tuples(b.effects(sc))
            b.upload(sc)
            hits = H.as_tuples(b.hits(sc))
        _, geo = E.expected_effects(pats, case["regions"])
        by = {x[:3]: x for x in got}
        per = {}
        for x in hits:  # (region, haplotype, pattern, window, start, end, score)
            per.setdefault(x[:3], []).append(x)
        for r, v, pi, h, win in single_variant_pairs(case, pats, b, got, geo):
            x = by[(r, v, pi)]
            mine = [y for y in per.get((r, h, pi), []) if y[3] in set(win)]
            assert x[7] == len(win)
            assert (x[7] > 0 and x[8] > pats[pi].min_score) == bool(mine), (name, r, v, pi)
            if mine:
                top = max(y[6] for y in mine)
                first = min(y for y in mine if y[6] == top)
                assert (x[8], x[9], x[12], x[13]) == (top, first[3], first[4], first[5])
                with_hit += 1
            else:
                without += 1
    assert with_hit >= 20 and without >= 20


def test_calls(monkeypatch):
    case = K.case_n_and_indels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    L = T.lib()
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        assert b.num_regions == 3
        full = b.effects(sc)  # no upload needed
        assert len(full) == sum(b.region_stats(r)[1] for r in range(3)) * len(pats) > 100
        ms = sc.last_effects_ms()
        assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0
        b.scan(sc, reduce=True)
        want = [b.digest(r) for r in range(3)]
        T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(3)] == want
        assert np.array_equal(b.effects(sc), full)
        for _ in range(3):  # (from the third step alike a graph replay)
            T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(3)] == want
        rows = b.rows("chr1")[0]
        assert np.array_equal(b.effects(sc), full)
        assert b.rows("chr1")[0] == rows
        # a batch that keeps no variants; a bad range; another pattern set's scanner
        from helpers import build_batch
        plain = build_batch(ps, case["n"], case["beds"], case["regions"])
        assert [plain.input_digest(r) for r in range(3)] == [b.input_digest(r) for r in range(3)]
        with pytest.raises(T.TfbsError) as ei:
            plain.effects(sc)
        assert ei.value.code == -14  # TFBS_E_STATE
        for r0, r1 in ((2, 1), (0, 4)):
            with pytest.raises(T.TfbsError) as ei:
                b.effects(sc, r0, r1)
            assert ei.value.code == -1  # TFBS_E_ARG
        assert len(b.effects(sc, 1, 1)) == 0
    empty = T.PatternSet.from_patterns([T.Pattern.OtherPattern("o", 0)])
    with scanner(empty) as sc:  # a set that scores nothing: every record is the empty one
        probe = T.RegionBatch(empty, 2, keep_variants=True)
        probe.add_bed("a.bed")
        es, ee = probe.ext(500, 520)
        probe.begin(500, 520, ("ACGT" * 20)[:ee - es + 1])
        probe.add_inner(0, 500, 520)
        probe.add_record_carriers(505, "ACGT"[(505 - es) % 4], "ACGT"[(506 - es) % 4], [1])
        probe.end()
        got = E.as_tuples(probe.effects(sc))
        assert got == [(0, 0, 0, 0) + E.EMPTY_SIDE + E.EMPTY_SIDE + (0, 0, 0, 0)]
        with pytest.raises(T.TfbsError) as ei:
            b.effects(sc)
        assert ei.value.code == -1  # TFBS_E_ARG: another pattern set


# ------------------------------------------------------------ run flow and command line
BEDS = [os.path.join(TD, "regions1.bed"), os.path.join(TD, "regions2.bed")]


def fixture_regions(ps):
    """The merged regions of the reference's test data (genotypes2.bcf, the samples file) as a
    case's region dicts, from BcfReader and fasta_fetch."""
    merged, beds = O.load_peak_files(BEDS, "chr1", 0)
    rd = T.BcfReader(os.path.join(TD, "genotypes2.bcf"))
    want = {l.strip() for l in open(os.path.join(TD, "samples")) if len(l.rstrip("\n")) > 1}
    rd.select([i for i, s in enumerate(rd.samples) if s in want])
    probe = T.RegionBatch(ps, len(rd.selected))
    regions = []
    for s, e in merged:
        es, ee = probe.ext(s, e)
        ref = T.fasta_fetch(os.path.join(TD, "reference_genome.fa"), "chr1", es, ee + 1)
        recs = [("gt", rec["pos0"], rec["n_alleles"], rec["ref"], rec["alt"], rec["gt"])
                for rec in rd.fetch("chr1", es, ee + 1)]
        regions.append({"merged": (s, e), "ref": ref, "es": es, "ee": ee, "records": recs})
    return regions, beds, len(rd.selected)


def run_fixture(out, **kw):
    T.run("chr1", os.path.join(TD, "genotypes2.bcf"), BEDS, os.path.join(TD, "reference_genome.fa"),
          os.path.join(TD, "samples"), os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"], str(out), **kw)
    return T.bgzf_read(str(out))


def test_run_flow_and_cli_effects_output(tmp_path):
    main = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    assert run_fixture(tmp_path / "plain.vcf.gz") == main
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    pats = ps.to_list()
    regions, beds, n = fixture_regions(ps)
    assert len(regions) >= 2
    rows, _ = E.expected_effects(pats, regions)
    assert rows
    want = {mode: E.HEADER + E.format_tsv("1", pats, regions, rows, mode) for mode in ("sites", "all")}
    # the fixture's one polymorphism takes a site from 4000 to 3000: a line with its delta
    assert any(l.split("\t")[7] in ("loss", "change", "gain") for l in want["sites"].splitlines())
    assert "\tvar\tscored\t" in want["sites"] and len(want["all"]) >= len(want["sites"])
    with scanner(ps) as sc:  # the library's own formatter on its own records says the same
        b = E.build_batch(ps, n, beds, regions)
        eff = b.effects(sc)
        assert E.as_tuples(eff) == rows
        for mode in ("sites", "all"):
            assert b.effects_tsv(eff, "1", mode, header=True) == want[mode]
    k = 0
    for mode in ("sites", "all"):
        for kw in ({"regions_per_batch": 1}, {"regions_per_batch": 512}, {"devices": [0, 0], "regions_per_batch": 1}):
            k += 1
            out, eout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("e%d.tsv.gz" % k)
            assert run_fixture(out, effects_output=str(eout), effects_mode=mode, **kw) == main, (mode, kw)
            assert T.bgzf_read(str(eout)) == want[mode], (mode, kw)
            assert not os.path.exists(str(eout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    for mode in ("sites", "all"):
        out, eout = tmp_path / ("cli_%s.vcf.gz" % mode), tmp_path / ("cli_%s.tsv.gz" % mode)
        r = subprocess.run([exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed",
                            ",".join(BEDS), "--reference", os.path.join(TD, "reference_genome.fa"), "--samples",
                            os.path.join(TD, "samples"), "--pwm_file", os.path.join(TD, "pwm_definitions.txt"),
                            "--pwm_threshold_directory", TD, "--pwm_threshold", "0.0001", "--pwm_names", "ACGT",
                            "--output", str(out), "--effects_output", str(eout), "--effects_mode", mode],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert T.bgzf_read(str(out)) == main
        assert T.bgzf_read(str(eout)) == want[mode]
