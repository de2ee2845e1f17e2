"""The best-site kernel (scan_best.hip) through RegionBatch.best: per (distinct haplotype, pattern
strand, inner range) the highest score among the windows overlapping the range, the lowest window
attaining it and the number of such windows, against the plain Python restatement (best_ref.py);
ties; agreement with the hit list and with the count path's keys; the calls' contract; the run
flow's and the command line's --best_output.  The cases are dinuc_cases.py's, unchanged, and one
periodic case built here; what is expected comes from their per-haplotype-id sequences.  Integer
work: every comparison is exact."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

import best_ref as R
import dinuc_cases as K
import hits_ref as H
import oracle_py as O
from helpers import GOLD, TD, T, build_batch, run_product

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------ the periodic case (ties)
PERIOD_MONO_L, PERIOD_DI_L = 8, 5


@functools.lru_cache(None)
def case_periodic():
    """A reference window of 734 bases of period 2 (ACAC...), one SNV carried by three of eight
    haplotype ids (two distinct haplotypes), a mono strand of 8 columns and a dinucleotide strand
    of 5 bases: the windows of one parity share a score, so a maximum is attained in every
    64-window chunk and every 256-window sweep that the range reaches.  Three inner ranges: the
    merged range, its first 41 bases and its last 61 (best windows beyond window 256)."""
    n = 4
    probe = K.probe_batch(PERIOD_MONO_L, n)
    s, e = 40000, 40719
    es, ee = probe.ext(s, e)
    ref = ("AC" * ((ee - es + 2) // 2))[:ee - es + 1]
    assert len(ref) >= 700
    k = 333
    reg = {"merged": (s, e), "ref": ref, "es": es, "ee": ee,
           "records": [("car", es + k, ref[k], "G", [1, 4, 6])]}
    mono = T.Pattern.PWM([T.Weight(*w) for w in ([5, -3, 2, 0], [-1, 4, 0, 2], [3, 0, -2, 1], [0, 6, 1, -4],
                                                 [2, -5, 0, 3], [-2, 7, 1, 0], [4, 1, -1, 0], [0, 3, 2, -6])],
                         "per8", 0, 0)
    assert len(mono) == PERIOD_MONO_L
    import random
    di = T.Pattern.DiPWM(K.rand_rows(random.Random(1809), PERIOD_DI_L, -50, 50), "per5", 1, 0, T.DIR_N)
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 40), (e - 60, e)])]
    case = {"pats": [mono, di], "n": n, "regions": [reg], "beds": beds}
    case["seqs"] = [K.hap_sequences(reg, n)]
    return case


def check_best(sc, ps, pats, case):
    """best() equals the reference list, dense and sorted; returns (batch, orders, tuples)."""
    b = uploaded(sc, ps, case)
    order = orders(b, case)
    got = R.as_tuples(b.best(sc))
    want = R.expected_best(pats, case["regions"], case["beds"], order)
    assert len(got) == len(want) == sum(len(order[r]) * len(pats) * len(b.ranges(r)) for r in range(b.num_regions))
    for g, w in zip(got, want):
        assert g == w
    assert [x[:4] for x in got] == sorted(set(x[:4] for x in got))  # one record each, sorted
    return b, order, got


CASES = ["case_all_kernels", "case_geometry", "case_many_haplotypes", "case_n_and_indels", "case_reduction",
         "case_wrap", "periodic"]


@pytest.mark.parametrize("name", CASES)
def test_reference_equality(name):
    """Field by field on every case.  case_geometry's set gets a TFBS_KIND_OTHER pattern on top (no
    case has one); the periodic case is here beside the six of dinuc_cases.py because none of
    those has a best window beyond window 256.  Each case asserts what it is there for."""
    case = case_periodic() if name == "periodic" else getattr(K, name)()
    pats = case_patterns(case)
    if name == "case_geometry":
        pats = pats + [T.Pattern.OtherPattern("other", 50)]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, order, got = check_best(sc, ps, pats, case)
    other = [i for i, p in enumerate(pats) if p.kind == T.KIND_OTHER]
    assert all(x[4:] == (R.UINT32_MAX, 0, R.INT32_MIN, 0, 0) for x in got if x[2] in other)
    chunks = {x[4] // 64 for x in got if x[5]}
    if name == "case_all_kernels":  # best windows in each of chunks 0 .. 3; a strand over 32 columns
        assert {0, 1, 2, 3} <= chunks
        assert any(len(pats[x[2]]) == 36 and x[5] for x in got)
        assert any(len(set(pos)) < len(pos) or list(pos) != list(range(pos[0], pos[0] + len(pos)))
                   for o in order for _, pos in o)  # indels
    if name == "case_geometry":  # records with n_windows == 0, a TFBS_KIND_OTHER pattern, a one-window haplotype
        assert len(other) == 1
        # region 0's haplotypes of 2 bases are shorter than the four strands of 5 and 9 bases
        short = len(order[0]) * 4 * len(b.ranges(0))
        assert short >= 36 and sum(1 for x in got if x[5] == 0 and x[2] not in other) >= short
        assert sorted(len(o[0][0]) - 1 for o in order) == sorted(K.GEOMETRY_WINDOWS)
    if name == "periodic":  # best windows beyond window 256
        assert any(c >= 4 for c in chunks) and any(x[4] >= 640 for x in got if x[5])
    if name == "case_n_and_indels":  # several windows of one position (an insertion): overlap goes by position
        assert any(len(set(pos)) < len(pos) for o in order for _, pos in o)
    if name == "case_reduction":  # nested and duplicate inner ranges, more ranges than one sweep takes
        assert len(b.ranges(0)) > 32
    if name == "case_wrap":  # wrapped sums: weights at INT32_MIN
        assert any(w == K.INT32_MIN for p in pats for row in p.weights for w in row)


def test_ties_go_to_the_lowest_window():
    case = case_periodic()
    pats = case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        order = orders(b, case)
        assert len(order[0]) >= 2
        got = R.as_tuples(b.best(sc))
    ranges = b.ranges(0)
    assert len(got) == len(order[0]) * 2 * len(ranges)
    spread = set()
    for x in got:
        _, h, pi, k, window, n, score, start, end = x
        codes, pos = order[0][h]
        p = pats[pi]
        sc_all = H.pattern_scores(p, codes)
        mine = [i for i in range(len(sc_all)) if T.range_overlaps(ranges[k], (pos[i], pos[i] + len(p) - 1))]
        assert n == len(mine) > 0
        top = max(sc_all[i] for i in mine)
        at = [i for i in mine if sc_all[i] == top]
        assert (score, window) == (top, at[0]) and (start, end) == (pos[at[0]], pos[at[0]] + len(p) - 1)
        if len({i // 64 for i in at}) >= 3 and len({i // 256 for i in at}) >= 2:
            spread.add((h, pi))
    # the maximum sits in at least three 64-window chunks and two 256-window sweeps for both strands
    # (under the merged range; the SNV gives its haplotype's dinucleotide strand one window above the rest)
    assert len(spread) >= 3 and {pi for _, pi in spread} == {0, 1}


def test_agreement_with_the_hit_list():
    case = K.case_all_kernels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        hits = H.as_tuples(b.hits(sc))
        best = R.as_tuples(b.best(sc))
    per = {}
    for x in hits:  # (region, haplotype, pattern, window, start, end, score)
        per.setdefault(x[:3], []).append(x)
    with_hits = without = 0
    ranges = [b.ranges(r) for r in range(b.num_regions)]
    for r, h, pi, k, window, n, score, _, _ in best:
        rng = ranges[r][k]
        over = [x for x in per.get((r, h, pi), []) if T.range_overlaps(rng, (x[4], x[5]))]
        if over:
            top = max(x[6] for x in over)
            assert score == top and window == min(x[3] for x in over if x[6] == top) and n >= len(over)
            with_hits += 1
        else:
            assert n == 0 or score <= pats[pi].min_score
            without += 1
    assert with_hits > 100 and without > 100


def test_agreement_with_the_count_path():
    case = K.case_reduction()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    n, beds = case["n"], case["beds"]
    want = [dict(w) for w in case["want"]]
    for w, m in zip(want, case["mono_keys"]):
        w.update(m)
    pids = sorted({p.pattern_id for p in pats})
    possible = [[(beds[bi][0], (a, z), pid) for bi, a, z in T.select_inner_peaks(reg["merged"], beds) for pid in pids]
                for reg in case["regions"]]
    assert any(k in w for ks, w in zip(possible, want) for k in ks)        # (known on the CPU beforehand)
    assert any(k not in w for ks, w in zip(possible, want) for k in ks)
    with scanner(ps) as sc:
        keys, _, b = run_product(sc, ps, n, beds, case["regions"], reduce=True)
        assert keys == want
        best = b.best(sc)
        hit = miss = 0
        for r in range(b.num_regions):
            scores, counts = b.best_by_sample(best, r)
            ranges = b.ranges(r)
            thr = np.array([p.min_score for p in pats], dtype=np.int64)
            above = (counts > 0) & (scores.astype(np.int64) > thr[None, :, None])  # [id][strand][range]
            for key in set(possible[r]):
                bed, rng, pid = key
                strands = [i for i, p in enumerate(pats) if p.pattern_id == pid]
                k = ranges.index(rng)
                lr = keys[r].get(key, ([0] * n, [0] * n))
                for x in range(2 * n):
                    assert (lr[x & 1][x >> 1] > 0) == bool(above[x, strands, k].any()), (key, x)
                hit += key in keys[r]
                miss += key not in keys[r]
        assert hit > 0 and miss > 0


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
        full = b.best(sc)
        assert len(full) > 1000
        ms = sc.last_best_ms()
        assert ms[0] > 0 and ms[1] > 0
        for _ in range(3):  # (from the third step alike a graph replay)
            T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(3)] == before
        for r0 in range(4):
            for r1 in range(r0, 4):
                part = b.best(sc, r0, r1)
                assert np.array_equal(part, full[(full["region"] >= r0) & (full["region"] < r1)]), (r0, r1)
        assert np.array_equal(b.best(sc, 1), full[full["region"] >= 1])
        monkeypatch.setenv("TFBS_BEST_SCRATCH_MB", "0.001")  # one haplotype per chunk
        assert np.array_equal(b.best(sc), full)
        monkeypatch.delenv("TFBS_BEST_SCRATCH_MB")
        assert np.array_equal(b.best(sc), full)
        # best_by_sample: the per-haplotype-id sequences' own best records
        for r, reg in enumerate(case["regions"]):
            scores, counts = b.best_by_sample(full, r)
            ranges = R.region_ranges(reg, case["beds"])
            assert scores.shape == counts.shape == (2 * case["n"], len(pats), len(ranges))
            assert scores.dtype == np.int32
            for x, (codes, pos) in enumerate(case["seqs"][r]):
                for pi, p in enumerate(pats):
                    for k, rng in enumerate(ranges):
                        _, nw, s, _, _ = R.best_of(p, codes, pos, rng)
                        assert (int(scores[x, pi, k]), int(counts[x, pi, k])) == (s, nw), (r, x, pi, k)
        with pytest.raises(ValueError):
            b.best_by_sample(full[1:], 0)
        other = build_batch(ps, case["n"], case["beds"], case["regions"])
        with pytest.raises(T.TfbsError) as ei:
            other.best(sc)
        assert ei.value.code == -14  # TFBS_E_STATE
        for r0, r1 in ((2, 1), (0, 4)):
            with pytest.raises(T.TfbsError) as ei:
                b.best(sc, r0, r1)
            assert ei.value.code == -1  # TFBS_E_ARG
    empty = T.PatternSet.from_patterns([T.Pattern.OtherPattern("o", 0)])
    with scanner(empty) as sc:  # a set that scores nothing: every record is the empty one
        probe = T.RegionBatch(empty, 2)
        probe.add_bed("a.bed")
        es, ee = probe.ext(500, 520)
        probe.begin(500, 520, ("ACGT" * 20)[:ee - es + 1])
        probe.add_inner(0, 500, 520)
        probe.end()
        probe.upload(sc)
        got = R.as_tuples(probe.best(sc))
        assert got == [(0, 0, 0, 0, R.UINT32_MAX, 0, R.INT32_MIN, 0, 0)]
        assert len(probe.best(sc, 0, 0)) == 0


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
    return T.bgzf_read(str(out))


def test_run_flow_and_cli_best_output(tmp_path):
    main = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    assert run_fixture(tmp_path / "plain.vcf.gz") == main
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    with scanner(ps) as sc:
        b = fixture_batch(ps)
        b.upload(sc)
        assert b.num_regions >= 2
        best = b.best(sc)
        assert len(best) > 0
        want = {mode: T.BEST_HEADER + b.best_tsv(best, "1", mode) for mode in ("all", "diff")}
    # the fixture's one polymorphism takes a site from 4000 to 3000: an `alt` line with its delta
    alts = [l.split("\t") for l in want["diff"].splitlines() if l.split("\t")[9] == "alt"]
    assert alts and all(l[14] not in (".", "0") for l in alts) and any(l[14] == "-1000" for l in alts)
    assert "\tbest\t" in want["all"] and "\tbase\t" in want["diff"] and "\thap\t" in want["diff"]
    k = 0
    for mode in ("all", "diff"):
        for kw in ({}, {"regions_per_batch": 1}, {"regions_per_batch": 512}, {"devices": [0, 0], "regions_per_batch": 1}):
            k += 1
            out, bout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("b%d.tsv.gz" % k)
            assert run_fixture(out, best_output=str(bout), best_mode=mode, **kw) == main, (mode, kw)
            assert T.bgzf_read(str(bout)) == want[mode], (mode, kw)
            assert not os.path.exists(str(bout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    for mode in ("all", "diff"):
        out, bout = tmp_path / ("cli_%s.vcf.gz" % mode), tmp_path / ("cli_%s.tsv.gz" % mode)
        r = subprocess.run([exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed",
                            ",".join(BEDS), "--reference", os.path.join(TD, "reference_genome.fa"), "--samples",
                            os.path.join(TD, "samples"), "--pwm_file", os.path.join(TD, "pwm_definitions.txt"),
                            "--pwm_threshold_directory", TD, "--pwm_threshold", "0.0001", "--pwm_names", "ACGT",
                            "--output", str(out), "--best_output", str(bout), "--best_mode", mode],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert T.bgzf_read(str(out)) == main
        assert T.bgzf_read(str(bout)) == want[mode]
