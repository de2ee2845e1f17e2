"""The binding-affinity kernel (scan_affinity.hip) through RegionBatch.affinity: per (distinct
haplotype, pattern strand, inner range) the exact integer sum of a(top - score) over the windows
overlapping the range and the two counts, against the plain Python restatement (affinity_ref.py,
a from 80-digit decimals); the cutoff of a at hand-counted windows; the census of an all-zero
PWM; agreement with the best sites; scratch budgets and sub-ranges; the calls' contract; the run
flow's and the command line's --affinity_output.  The cases are dinuc_cases.py's, unchanged, and
the periodic construction of test_gpu_best.py rebuilt here; what is expected comes from their
per-haplotype-id sequences.  Integer work: every comparison is exact."""
import collections
import contextlib
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import affinity_ref as A
import best_ref as R
import dinuc_cases as K
import hits_ref as H
import oracle_py as O
from helpers import GOLD, TD, T, build_batch

pytestmark = pytest.mark.gpu
Q40 = 1 << 40


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


def uploaded(sc, ps, case):
    b = build_batch(ps, case["n"], case["beds"], case["regions"])
    b.upload(sc)
    return b


def orders(b, case):
    """Per region the sequences in the library's index order; they are the case's."""
    out = [H.library_order(b, r) for r in range(b.num_regions)]
    for order, seqs in zip(out, case["seqs"]):
        assert sorted(order) == sorted(set(seqs))
    return out


@functools.lru_cache(None)
def case_periodic():
    """test_gpu_best.py's periodic case: a reference window of 734 bases of period 2, one SNV
    carried by three of eight haplotype ids, a mono strand of 8 columns and a dinucleotide strand
    of 5 bases; three inner ranges, the last one beyond window 256."""
    n = 4
    probe = K.probe_batch(8, n)
    s, e = 40000, 40719
    es, ee = probe.ext(s, e)
    ref = ("AC" * ((ee - es + 2) // 2))[:ee - es + 1]
    assert len(ref) >= 700
    k = 333
    reg = {"merged": (s, e), "ref": ref, "es": es, "ee": ee, "records": [("car", es + k, ref[k], "G", [1, 4, 6])]}
    mono = T.Pattern.PWM([T.Weight(*w) for w in ([5, -3, 2, 0], [-1, 4, 0, 2], [3, 0, -2, 1], [0, 6, 1, -4],
                                                 [2, -5, 0, 3], [-2, 7, 1, 0], [4, 1, -1, 0], [0, 3, 2, -6])],
                         "per8", 0, 0)
    di = T.Pattern.DiPWM(K.rand_rows(random.Random(1809), 5, -50, 50), "per5", 1, 0, T.DIR_N)
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 40), (e - 60, e)])]
    case = {"pats": [mono, di], "n": n, "regions": [reg], "beds": beds}
    case["seqs"] = [K.hap_sequences(reg, n)]
    return case


def check_against_best(aff, best, tops):
    """Equal n_windows; a(top - best score) <= sum <= n_windows * a(top - best score)."""
    assert len(aff) == len(best)
    for name in ("region", "haplotype", "pattern", "range", "n_windows"):
        assert np.array_equal(aff[name], best[name]), name
    for x, y in zip(aff, best):
        if y["n_windows"]:
            a = A.weight(tops[int(x["pattern"])] - int(y["score"]))
            assert a <= int(x["sum"]) <= int(y["n_windows"]) * a
            assert (int(x["n_nonzero"]) > 0) == (a > 0)
        else:
            assert (int(x["n_nonzero"]), int(x["sum"])) == (0, 0)


def check_affinity(sc, ps, pats, case):
    """affinity() equals the model's list, dense and sorted, and agrees with best() on the same
    batch; returns (batch, orders, tuples)."""
    b = uploaded(sc, ps, case)
    order = orders(b, case)
    aff = b.affinity(sc)
    got = A.as_tuples(aff)
    want = A.expected(pats, case["regions"], case["beds"], order)
    assert len(got) == len(want) == sum(len(order[r]) * len(pats) * len(b.ranges(r)) for r in range(b.num_regions))
    for g, w in zip(got, want):
        assert g == w
    assert [x[:4] for x in got] == sorted(set(x[:4] for x in got))  # one record each, sorted
    assert all(x[5] <= x[4] and x[6] <= x[5] * Q40 for x in got)
    check_against_best(aff, b.best(sc), A.tops(pats))
    return b, order, got


CASES = ["case_all_kernels", "case_geometry", "case_many_haplotypes", "case_n_and_indels", "case_reduction", "periodic"]


@pytest.mark.parametrize("name", CASES)
def test_reference_equality(name):
    """Field by field on every case.  case_geometry's set gets a TFBS_KIND_OTHER pattern on top.
    case_all_kernels' set holds the `quad` PWM, whose weights of 2^30 and -2^30 can wrap int32 by
    the rule of tfbs_patterns_affinity_tops: the unchanged set is refused naming it, and the
    records are compared on the set without that one strand."""
    case = case_periodic() if name == "periodic" else getattr(K, name)()
    pats = case_patterns(case)
    if name == "case_geometry":
        pats = pats + [T.Pattern.OtherPattern("other", 50)]
    if name == "case_all_kernels":
        ps = T.PatternSet.from_patterns(pats)
        with scanner(ps) as sc:
            b = uploaded(sc, ps, case)
            with pytest.raises(T.TfbsError) as ei:
                b.affinity(sc)
            assert ei.value.code == -1 and "'quad' (+) can wrap int32" in str(ei.value)
        assert [p.name for p in pats].count("quad") == 1
        pats = [p for p in pats if p.name != "quad"]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, order, got = check_affinity(sc, ps, pats, case)
    other = [i for i, p in enumerate(pats) if p.kind == T.KIND_OTHER]
    assert all(x[4:] == (0, 0, 0) for x in got if x[2] in other)
    most = max(x[4] for x in got)
    if name in ("case_all_kernels", "case_n_and_indels", "case_reduction"):  # (strands long enough for d > 27725)
        assert any(0 < x[5] < x[4] for x in got)  # windows on both sides of the cutoff in one record
    if name == "case_all_kernels":  # windows in all four chunks of a pass, a strand over 32 columns, dinucleotide L of 2 and 32, indels
        assert max(len(codes) for o in order for codes, _ in o) - 1 > 192 and {2, 32, 36} <= {len(p) for p in pats}
        assert any(len(pats[x[2]]) == 36 and x[4] for x in got)
        assert any(len(set(pos)) < len(pos) or list(pos) != list(range(pos[0], pos[0] + len(pos)))
                   for o in order for _, pos in o)
    if name == "case_geometry":  # 1 .. 257 windows, haplotypes shorter than L, a TFBS_KIND_OTHER pattern
        assert len(other) == 1
        assert sorted(len(o[0][0]) - 1 for o in order) == sorted(K.GEOMETRY_WINDOWS)
        assert sum(1 for x in got if x[4] == 0 and x[2] not in other) >= 36
        assert {63, 64, 65, 191, 192, 193} <= {len(o[0][0]) - 1 for o in order}
    if name == "periodic":  # more than 256 windows in one range, and a range of its own beyond window 256
        assert most > 640
    if name == "case_n_and_indels":  # several windows of one position (an insertion), N runs
        assert any(len(set(pos)) < len(pos) for o in order for _, pos in o)
        assert any(4 in codes for o in order for codes, _ in o)
    if name == "case_reduction":  # more ranges than one sweep takes, and a last sweep of every width
        assert len(b.ranges(0)) > 32 and len(b.ranges(1)) in (1, 2, 3)


def test_cutoff_at_hand_counted_windows():
    """One-column strands: a window's score is its base's weight, so the windows of a range sit at
    d = 0, 1, 999, 1000 (strand 0), 27725, 27726 and a million (strand 1, which shares strand 0's
    pattern_id and so its top of 30000), and the record follows from the range's base counts."""
    top = 30000
    s0 = T.Pattern.PWM([T.Weight(top, top - 1, top - 999, top - 1000)], "cut", 0, 0, T.DIR_P)
    s1 = T.Pattern.PWM([T.Weight(top - 27725, top - 27726, top - 1000000, top - 27726)], "cut", 0, 0, T.DIR_N)
    pats = [s0, s1]
    n = 3
    rnd = random.Random(77)
    ps = T.PatternSet.from_patterns(pats)
    reg = K.make_region(rnd, T.RegionBatch(ps, n), n, 5000, 300, 5, n_at=(7, 8, 120))  # (L = 1: no flank)
    s, e = reg["merged"]
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 63), (s, s + 64), (s + 100, e), (s, s + 8)])]  # (each holds an end of the merged range)
    case = {"pats": pats, "n": n, "regions": [reg], "beds": beds, "seqs": [K.hap_sequences(reg, n)]}
    assert ps.affinity_tops() == [top, top]
    a = {d: A.weight_exact(d) for d in (0, 1, 999, 1000, 27725, 27726)}
    assert a[0] == Q40 and a[27725] == 1 and a[27726] == 0 and a[0] > a[1] > a[999] > a[1000] > 1
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        order = orders(b, case)
        got = b.affinity(sc)
    ranges = b.ranges(0)
    assert len(ranges) == 5 and len(order[0]) >= 3 and len(got) == len(order[0]) * 2 * 5
    seen = collections.Counter()
    for x in got:
        codes, pos = order[0][int(x["haplotype"])]
        lo, hi = ranges[int(x["range"])]
        cnt = collections.Counter(c for c, p in zip(codes, pos) if lo <= p <= hi)  # (L = 1: the match is the base)
        nA, nC, nG, nT, nN = (cnt[c] for c in range(5))
        seen.update(cnt)
        assert int(x["n_windows"]) == nA + nC + nG + nT + nN
        if int(x["pattern"]) == 0:  # an N scores 0: d = 30000, beyond the cutoff
            assert int(x["n_nonzero"]) == nA + nC + nG + nT
            assert int(x["sum"]) == nA * a[0] + nC * a[1] + nG * a[999] + nT * a[1000]
        else:  # d = 27725 weighs 1, 27726 and everything beyond weigh 0
            assert (int(x["n_nonzero"]), int(x["sum"])) == (nA, nA)
    assert all(seen[c] > 0 for c in range(5))


def test_census_of_an_all_zero_pwm():
    """Every window of an all-zero strand sits at d = 0: sum = n_windows * 2^40 exactly, on every
    haplotype (N runs, indels) and range."""
    case = K.case_n_and_indels()
    pats = [T.Pattern.PWM([T.Weight(0, 0, 0, 0)] * 6, "zero", 0, 0),
            T.Pattern.DiPWM([[0] * 16] * 19, "dizero", 1, 0),
            T.Pattern.PWM([T.Weight(0, 0, 0, 0)] * 20, "zero20", 2, 0, T.DIR_N)]  # (the case's regions extend by 20)
    ps = T.PatternSet.from_patterns(pats)
    assert ps.affinity_tops() == [0, 0, 0]
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        got = b.affinity(sc)
        best = b.best(sc)
    assert len(got) > 100 and np.array_equal(got["n_windows"], best["n_windows"])
    assert np.array_equal(got["n_nonzero"], got["n_windows"]) and got["n_windows"].max() > 64
    assert np.array_equal(got["sum"], got["n_windows"].astype(np.uint64) * np.uint64(Q40))


def test_calls(monkeypatch):
    case = K.case_n_and_indels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    L = T.lib()
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        assert b.num_regions == 3
        b.scan(sc, upload=False, reduce=True)
        want = [b.digest(r) for r in range(3)]
        T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        before = [b.digest(r) for r in range(3)]
        assert before == want
        best_before = b.best(sc)
        assert sc.last_affinity_ms() == (0.0, 0.0)  # (nothing made before the first call)
        full = b.affinity(sc)
        assert len(full) > 1000
        ms = sc.last_affinity_ms()
        assert ms[0] > 0 and ms[1] > 0
        for _ in range(3):  # (from the third step alike a graph replay)
            T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(3)] == before
        assert np.array_equal(b.best(sc), best_before)
        for r0 in range(4):
            for r1 in range(r0, 4):
                part = b.affinity(sc, r0, r1)
                assert np.array_equal(part, full[(full["region"] >= r0) & (full["region"] < r1)]), (r0, r1)
        assert np.array_equal(np.concatenate([b.affinity(sc, r, r + 1) for r in range(3)]), full)
        for mb in ("0", "0.001", "0.01"):  # one haplotype per chunk; a few
            monkeypatch.setenv("TFBS_AFFINITY_SCRATCH_MB", mb)
            assert np.array_equal(b.affinity(sc), full), mb
        monkeypatch.delenv("TFBS_AFFINITY_SCRATCH_MB")
        assert np.array_equal(b.affinity(sc), full)
        # affinity_by_sample: the per-haplotype-id sequences' own records
        tp = A.tops(pats)
        for r, reg in enumerate(case["regions"]):
            sums, counts = b.affinity_by_sample(full, r)
            ranges = R.region_ranges(reg, case["beds"])
            assert sums.shape == counts.shape == (2 * case["n"], len(pats), len(ranges))
            for x, (codes, pos) in enumerate(case["seqs"][r]):
                for pi in (0, len(pats) - 1):
                    for k, rng in enumerate(ranges):
                        nw, _, s = A.record_of(pats[pi], tp[pi], codes, pos, rng)
                        assert (int(sums[x, pi, k]), int(counts[x, pi, k])) == (s, nw), (r, x, pi, k)
        other = build_batch(ps, case["n"], case["beds"], case["regions"])
        with pytest.raises(T.TfbsError) as ei:
            other.affinity(sc)
        assert ei.value.code == -14  # TFBS_E_STATE: not resident
        for r0, r1 in ((2, 1), (0, 4)):
            with pytest.raises(T.TfbsError) as ei:
                b.affinity(sc, r0, r1)
            assert ei.value.code == -1  # TFBS_E_ARG
        foreign = T.PatternSet.from_patterns(pats[:2])
        with scanner(foreign) as sc2:  # a ctx of another pattern set
            with pytest.raises(T.TfbsError) as ei:
                b.affinity(sc2)
            assert ei.value.code == -1
        assert np.array_equal(b.affinity(sc), full)
    empty = T.PatternSet.from_patterns([T.Pattern.OtherPattern("o", 0)])
    with scanner(empty) as sc:  # a set that scores nothing: every record is the empty one
        probe = T.RegionBatch(empty, 2)
        probe.add_bed("a.bed")
        es, ee = probe.ext(500, 520)
        probe.begin(500, 520, ("ACGT" * 20)[:ee - es + 1])
        probe.add_inner(0, 500, 520)
        probe.end()
        probe.upload(sc)
        assert A.as_tuples(probe.affinity(sc)) == [(0, 0, 0, 0, 0, 0, 0)]
        assert len(probe.affinity(sc, 0, 0)) == 0


def test_refusals_leave_the_ctx_usable():
    """case_wrap's set is refused naming the strand, each time, and best() goes on working; a
    region whose longest haplotype times the most strands of a pattern_id reaches 2^23 is refused."""
    case = K.case_wrap()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        best = b.best(sc)
        for _ in range(2):
            with pytest.raises(T.TfbsError) as ei:
                b.affinity(sc)
            assert ei.value.code == -1 and "can wrap int32" in str(ei.value)
        assert sc.last_affinity_ms() == (0.0, 0.0)
        assert np.array_equal(b.best(sc), best)
    # 64 one-column strands of one pattern_id: 2^23 / 64 = 131072 bases
    pats = [T.Pattern.PWM([T.Weight(1, 0, 0, 0)], "many", 0, 0, T.DIR_N if k & 1 else T.DIR_P) for k in range(64)]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        for length in (131071, 131072):
            b = T.RegionBatch(ps, 1)
            b.add_bed("a.bed")
            es, ee = b.ext(1000, 1000 + length - 1)
            assert (es, ee) == (1000, 1000 + length - 1)  # (L = 1: no flank)
            b.begin(1000, ee, "A" * length)
            b.add_inner(0, 1000, 1003)
            b.end()
            b.upload(sc)
            if length == 131071:  # the longest region that passes
                got = b.affinity(sc)
                assert len(got) == 64 and set(got["n_windows"]) == {4} and set(got["sum"]) == {4 * Q40}
            else:
                with pytest.raises(T.TfbsError) as ei:
                    b.affinity(sc)
                assert ei.value.code == -1 and "2^23" in str(ei.value)


# ------------------------------------------------------------ run flow and command line
BEDS = [os.path.join(TD, "regions1.bed"), os.path.join(TD, "regions2.bed")]


def fixture_batch(ps):
    """The merged regions of the reference's test data (genotypes2.bcf, the samples file) as one
    batch, from BcfReader and fasta_fetch."""
    merged, beds = O.load_peak_files(BEDS, "chr1", 0)
    rd = T.BcfReader(os.path.join(TD, "genotypes2.bcf"))
    want = {l.strip() for l in open(os.path.join(TD, "samples")) if len(l.rstrip("\n")) > 1}
    rd.select([i for i, s in enumerate(rd.samples) if s in want])
    b = T.RegionBatch(ps, len(rd.selected))
    for name, _ in beds:
        b.add_bed(name)
    for s, e in merged:
        es, ee = b.ext(s, e)
        b.begin(s, e, T.fasta_fetch(os.path.join(TD, "reference_genome.fa"), "chr1", es, ee + 1))
        for bi, a, z in T.select_inner_peaks((s, e), beds):
            b.add_inner(bi, a, z)
        for rec in rd.fetch("chr1", es, ee + 1):
            b.add_record_gt(rec["pos0"], rec["n_alleles"], rec["ref"], rec["alt"], rec["gt"])
        b.end()
    return b


def run_fixture(out, **kw):
    T.run("chr1", os.path.join(TD, "genotypes2.bcf"), BEDS, os.path.join(TD, "reference_genome.fa"),
          os.path.join(TD, "samples"), os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"], str(out), **kw)
    return open(str(out), "rb").read()


def test_run_flow_and_cli_affinity_output(tmp_path):
    main_text = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    plain = run_fixture(tmp_path / "plain.vcf.gz")
    assert T.bgzf_read(str(tmp_path / "plain.vcf.gz")) == main_text
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    with scanner(ps) as sc:
        b = fixture_batch(ps)
        b.upload(sc)
        assert b.num_regions >= 2
        aff = b.affinity(sc)
        assert len(aff) > 0 and aff["sum"].max() >= Q40  # (the fixture holds a perfect ACGT site: d = 0)
        want = {mode: T.AFFINITY_HEADER + b.affinity_tsv(aff, "1", mode) for mode in ("all", "diff")}
    # the fixture's one polymorphism takes a site from 4000 to 3000: an `alt` line with a negative delta
    alts = [l.split("\t") for l in want["diff"].splitlines() if l.split("\t")[9] == "alt"]
    assert alts and all(l[10] == "4000" for l in alts) and any(l[13].startswith("-") for l in alts)
    assert "\taff\t" in want["all"] and "\tbase\t" in want["diff"] and "\thap\t" in want["diff"]
    k = 0
    for mode in ("all", "diff"):
        for kw in ({"regions_per_batch": 1}, {"regions_per_batch": 512}, {"devices": [0, 0], "regions_per_batch": 1}):
            k += 1
            out, aout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("a%d.tsv.gz" % k)
            got = run_fixture(out, affinity_output=str(aout), affinity_mode=mode, **kw)
            assert T.bgzf_read(str(out)) == main_text, (mode, kw)
            if kw == {"regions_per_batch": 512}:  # the run of `plain`, plus the flag: the same bytes
                assert got == plain
            assert T.bgzf_read(str(aout)) == want[mode], (mode, kw)
            assert not os.path.exists(str(aout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    argv = [exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed", ",".join(BEDS),
            "--reference", os.path.join(TD, "reference_genome.fa"), "--samples", os.path.join(TD, "samples"),
            "--pwm_file", os.path.join(TD, "pwm_definitions.txt"), "--pwm_threshold_directory", TD,
            "--pwm_threshold", "0.0001", "--pwm_names", "ACGT"]
    out, aout = tmp_path / "cli.vcf.gz", tmp_path / "cli.tsv.gz"
    r = subprocess.run(argv + ["--output", str(out), "--affinity_output", str(aout)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(str(out), "rb").read() == plain
    assert T.bgzf_read(str(aout)) == want["diff"]  # (the default mode)
    r = subprocess.run(argv + ["--output", str(tmp_path / "bad.vcf.gz"), "--affinity_output", str(tmp_path / "bad.tsv.gz"),
                               "--affinity_mode", "both"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and not os.path.exists(str(tmp_path / "bad.tsv.gz"))
    with pytest.raises(T.TfbsError) as ei:  # the run flow refuses an unknown mode too
        x = T._capi.tfbs_run_ext_affinity()
        x.size = C.sizeof(x)
        x.affinity_output, x.affinity_mode = str(tmp_path / "bad2.tsv.gz").encode(), 7
        a = T._capi.tfbs_run_args()
        a.chromosome, a.bcf, a.bed_files = b"chr1", os.path.join(TD, "genotypes2.bcf").encode(), ",".join(BEDS).encode()
        a.reference, a.samples_file = os.path.join(TD, "reference_genome.fa").encode(), os.path.join(TD, "samples").encode()
        a.pwm_file, a.pwm_threshold_dir, a.pwm_names = os.path.join(TD, "pwm_definitions.txt").encode(), TD.encode(), b"ACGT"
        a.output, a.pwm_threshold, a.threads = str(tmp_path / "bad2.vcf.gz").encode(), 0.0001, 1
        T.check(T.lib().tfbs_run_ex(C.byref(a), C.byref(x)))
    assert ei.value.code == -1
