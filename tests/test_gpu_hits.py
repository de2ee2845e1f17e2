"""The hit list kernel (scan_hits.hip) through RegionBatch.hits: every (distinct haplotype,
pattern strand, window) with score > min_score, its range and its score, against the oracle's
`matches` (mono), dinuc_ref (dinucleotide) and the wrapped reference scores (hits_ref.py); the
hits folded through the overlap rule against the count path's keys (a second opinion on the
scan kernels, which share nothing with this one); the calls' contract; the run flow's and the
command line's --hits_output.  The cases are dinuc_cases.py's, unchanged; what is expected comes
from their per-haplotype-id sequences.  Integer work: every comparison is exact."""
import contextlib
import os
import random
import subprocess

import numpy as np
import pytest

import dinuc_cases as K
import dinuc_ref as D
import hits_ref as H
import oracle_py as O
from helpers import GOLD, TD, T, build_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@contextlib.contextmanager
def scanner(ps, **env):
    """A Scanner created with the environment variables `env` set (a context reads its settings
    when it is made); they are restored before it is used."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        sc = T.Scanner(ps)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    try:
        yield sc
    finally:
        sc.close()


def case_patterns(case, with_mono=True):
    if with_mono and "mono" in case:
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


def check_hits(sc, ps, pats, case):
    """hits() equals the reference list; returns (batch, orders, hits as tuples)."""
    b = uploaded(sc, ps, case)
    order = orders(b, case)
    got = H.as_tuples(b.hits(sc))
    want = H.expected_hits(pats, order)
    assert len(got) == len(want)
    assert got == want
    assert got == sorted(got, key=lambda x: x[:4])  # (region, haplotype, pattern, window)
    counts = b.hits_count(sc)
    assert [int(c) for c in counts] == [sum(1 for x in want if x[0] == r) for r in range(b.num_regions)]
    assert int(counts.sum()) == len(got)
    return b, order, got


def test_every_scan_path_against_the_oracle():
    """case_all_kernels: matrix-core, quad, 36-column and dinucleotide strands in one set, regions
    with indels.  Per region, distinct haplotype and pattern the ranges are the oracle's `matches`
    (mono) or dinuc_ref.matches (dinucleotide) in window order, the scores the wrapped reference's."""
    case = K.case_all_kernels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, order, got = check_hits(sc, ps, pats, case)
        per = {}
        for x in got:
            per.setdefault(x[:3], []).append(x)
        n_mono = n_di = 0
        for r, ord_r in enumerate(order):
            assert 5740 <= sum(1 for x in got if x[0] == r) <= 6462
            for h, (codes, pos) in enumerate(ord_r):
                hap = [(K.NUC[c], p) for c, p in zip(codes, pos)]
                for pi, p in enumerate(pats):
                    mine = per.get((r, h, pi), [])
                    if p.kind == T.KIND_DIPWM:
                        ranges = D.matches(p.weights, p.min_score, codes, pos)
                        n_di += len(ranges)
                    else:
                        ranges = O.matches([w.acgtn for w in p.weights], p.min_score, hap, kind=p.kind)
                        n_mono += len(ranges)
                    assert [(x[4], x[5]) for x in mine] == ranges, (r, h, pi)
                    sc_ref = H.pattern_scores(p, codes)
                    assert [x[6] for x in mine] == [sc_ref[x[3]] for x in mine], (r, h, pi)
                    assert all(pos[x[3]] == x[4] for x in mine)
        assert n_mono > 1000 and n_di > 1000
        long_ = [i for i, p in enumerate(pats) if len(p) == 36]
        assert long_ and any(x[2] in long_ for x in got)  # a strand over 32 columns hits


@pytest.mark.parametrize("name", ["case_geometry", "case_many_haplotypes"])
def test_window_geometry(name):
    """1 to 257 windows per haplotype (the 64-window chunk edges, a haplotype with one window, a
    region with no hit) and a region of 132 distinct haplotypes."""
    case = getattr(K, name)()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, order, got = check_hits(sc, ps, pats, case)
        if name == "case_geometry":
            assert sorted(len(o[0][0]) - 1 for o in order) == sorted(K.GEOMETRY_WINDOWS)
            assert not any(x[0] == 0 for x in got) and all(any(x[0] == r for x in got) for r in range(1, len(order)))
        else:
            assert len(order[0]) == 132 and len(got) == 13582


def test_arithmetic_edges():
    """case_wrap: thresholds INT32_MIN (every score but INT32_MIN hits) and INT32_MAX (none),
    sums that wrap in int32, a window with an N."""
    case = K.case_wrap()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b, order, got = check_hits(sc, ps, pats, case)
        assert len(got) == 8857
        by_thr = {}
        for x in got:
            by_thr.setdefault(pats[x[2]].min_score, []).append(x[6])
        assert K.INT32_MAX not in by_thr and len(by_thr[K.INT32_MIN]) > 1000
        wrapped = 0
        for codes, _ in order[0]:
            for p in pats:
                wrapped += sum(1 for i in range(len(codes) - len(p) + 1)
                               if not K.INT32_MIN <= K.exact_sum(p.weights, codes, i) <= K.INT32_MAX)
        assert wrapped > 100


def count_path_keys(sc, b):
    b.scan(sc, upload=False)
    return [b.keys(r) for r in range(b.num_regions)]


def folded(b, pats, case, hits):
    return [H.fold_keys(pats, case["n"], case["beds"], reg["merged"], [x for x in hits if x[0] == r],
                        b.membership(r)) for r, reg in enumerate(case["regions"])]


def wanted_keys(case, with_mono):
    want = [dict(w) for w in case["want"]]
    if with_mono and "mono_keys" in case:
        for w, m in zip(want, case["mono_keys"]):
            w.update(m)
    return want


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("name,with_mono", [("case_reduction", False), ("case_reduction", True),
                                            ("case_n_and_indels", True), ("case_all_kernels", True)])
def test_second_opinion_on_the_counts(name, with_mono, mfma):
    """The hits folded through select_inner_peaks, range_overlaps(inner, match), the bed
    multiplicity and the membership are the count path's keys (40 nested ranges, a range listed
    twice, N and indels, all four scan kernels) and the reference's."""
    case = getattr(K, name)()
    pats = case_patterns(case, with_mono)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps, TFBS_MFMA=mfma) as sc:
        b = uploaded(sc, ps, case)
        hits = H.as_tuples(b.hits(sc))
        mine = folded(b, pats, case, hits)
        assert mine == wanted_keys(case, with_mono)
        assert mine == count_path_keys(sc, b)


def test_calls(monkeypatch):
    """Any scratch budget gives the default's array (0: a chunk holds one haplotype and a region
    is split; 0.02 and 0.05 MiB: chunks of a few haplotypes, their records in several fills);
    hits(r0, r1) over a partition concatenates to hits(); the keys of a scan made before, between
    and after hits calls are equal; a batch not resident gives TFBS_E_STATE."""
    case = K.case_all_kernels()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        keys0 = count_path_keys(sc, b)
        full = b.hits(sc)
        assert len(full) > 15000
        keys1 = count_path_keys(sc, b)
        for mb in ("0", "0.02", "0.05", "1"):
            monkeypatch.setenv("TFBS_HITS_SCRATCH_MB", mb)
            assert np.array_equal(b.hits(sc), full), mb
            assert int(b.hits_count(sc).sum()) == len(full)
        monkeypatch.delenv("TFBS_HITS_SCRATCH_MB")
        parts = [b.hits(sc, 0, 1), b.hits(sc, 1, 1), b.hits(sc, 1, 3)]
        assert len(parts[1]) == 0 and np.array_equal(np.concatenate(parts), full)
        assert [int(x) for x in b.hits_count(sc, 1, 3)] == [int((full["region"] == r).sum()) for r in (1, 2)]
        keys2 = count_path_keys(sc, b)
        assert keys0 == keys1 == keys2 == wanted_keys(case, True)
        b.scan(sc, upload=False, reduce=True)  # the reduced path after hits calls, then hits again
        assert [b.keys(r) for r in range(b.num_regions)] == keys0
        assert np.array_equal(b.hits(sc), full)
        other = build_batch(ps, case["n"], case["beds"], case["regions"])
        with pytest.raises(T.TfbsError) as ei:
            other.hits(sc)
        assert ei.value.code == -14  # TFBS_E_STATE
        with pytest.raises(T.TfbsError) as ei:
            other.hits_count(sc)
        assert ei.value.code == -14
        with pytest.raises(T.TfbsError):
            b.hits(sc, 2, 1)


def test_many_haplotypes_in_small_chunks(monkeypatch):
    """132 distinct haplotypes of one region under budgets that split it into chunks of one, a
    few and tens of haplotypes."""
    case = K.case_many_haplotypes()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        full = b.hits(sc)
        assert len(full) == 13582
        for mb in ("0", "0.001", "0.004", "0.03"):
            monkeypatch.setenv("TFBS_HITS_SCRATCH_MB", mb)
            assert np.array_equal(b.hits(sc), full), mb


def test_only_other_patterns_give_an_empty_list():
    rnd = random.Random(1708)
    ps = T.PatternSet.from_patterns([T.Pattern.OtherPattern("o", 0), T.Pattern.OtherPattern("p", 1)])
    n = 4
    probe = T.RegionBatch(ps, n)  # (a set without a PWM extends a region by its own length 0)
    regions = [K.make_region(rnd, probe, n, 50000 + 1000 * k, 90, 6) for k in range(2)]
    case = {"n": n, "beds": [("a.bed", [r["merged"] for r in regions])], "regions": regions}
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        assert b.num_haplotypes > 2
        assert len(b.hits(sc)) == 0
        assert [int(x) for x in b.hits_count(sc)] == [0, 0]


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


def test_run_flow_and_cli_hits_output(tmp_path):
    main = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    assert run_fixture(tmp_path / "plain.vcf.gz") == main
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    with scanner(ps) as sc:
        b = fixture_batch(ps)
        b.upload(sc)
        assert b.num_regions >= 2
        hits = b.hits(sc)
        assert len(hits) > 0
        want = {mode: T.HITS_HEADER + b.hits_tsv(hits, "1", mode) for mode in ("all", "diff")}
    assert "\tgain\t" in want["diff"] or "\tloss\t" in want["diff"]  # (the fixture's one polymorphism)
    k = 0
    for mode in ("all", "diff"):
        for kw in ({}, {"regions_per_batch": 1}, {"regions_per_batch": 512}, {"devices": [0, 0], "regions_per_batch": 1}):
            k += 1
            out, hout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("h%d.tsv.gz" % k)
            assert run_fixture(out, hits_output=str(hout), hits_mode=mode, **kw) == main, (mode, kw)
            assert T.bgzf_read(str(hout)) == want[mode], (mode, kw)
            assert not os.path.exists(str(hout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    for mode in ("all", "diff"):
        out, hout = tmp_path / ("cli_%s.vcf.gz" % mode), tmp_path / ("cli_%s.tsv.gz" % mode)
        r = subprocess.run([exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed",
                            ",".join(BEDS), "--reference", os.path.join(TD, "reference_genome.fa"), "--samples",
                            os.path.join(TD, "samples"), "--pwm_file", os.path.join(TD, "pwm_definitions.txt"),
                            "--pwm_threshold_directory", TD, "--pwm_threshold", "0.0001", "--pwm_names", "ACGT",
                            "--output", str(out), "--hits_output", str(hout), "--hits_mode", mode],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert T.bgzf_read(str(out)) == main
        assert T.bgzf_read(str(hout)) == want[mode]
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--hits_output" in r.stderr and "--hits_mode" in r.stderr
