"""The score rows (score_rows.hip) through RegionBatch.score_rows: the device's text against the
plain Python restatement (score_ref.py, from brute-force best records of the cases' per-haplotype-id
sequences) and against the host function (tfbs_scores_as_genotypes on the values that b.best() and
the membership give), byte for byte.  The cases are score_cases.py's (test_scores_cpu.py shows on
the reference alone that each bites) and four of dinuc_cases.py's, unchanged.  Integer work: every
comparison is exact."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import best_ref as R
import dinuc_cases as K
import hits_ref as H
import oracle_py as O
import score_cases as SC
import score_ref as S
from helpers import GOLD, TD, T, build_batch

pytestmark = pytest.mark.gpu
CHROM = "chr7"


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


def host_text(sc, b, pats, case, min_maf=0, min_spread=1, pos=1, r0=0, r1=None):
    """The rows from the library's own best records and membership through the host function."""
    best = b.best(sc)
    pids = sorted({p.pattern_id for p in pats})
    lines = []
    for r in range(r0, b.num_regions if r1 is None else r1):
        reg = case["regions"][r]
        if not b.ranges(r):
            continue
        scores, counts = b.best_by_sample(best, r)  # [haplotype id][strand][range]
        ranges = b.ranges(r)
        for a, z, bi in sorted({(a, z, bi) for bi, a, z in R.inner_of(reg, case["beds"]) if z >= a}):
            k = ranges.index((a, z))
            for pid in pids:
                strands = [i for i, p in enumerate(pats) if p.pattern_id == pid]
                vals = []
                for x in range(2 * case["n"]):
                    have = [int(scores[x, i, k]) for i in strands if counts[x, i, k] > 0]
                    vals.append(max(have) if have else None)
                if None in vals or not vals:
                    continue
                g = T.scores_as_genotypes(vals[0::2], vals[1::2], min_spread)
                if g is None or g[0] < min_maf:
                    continue
                name = next(p.name for p in pats if p.pattern_id == pid)
                lines.append("%s\t%d\t%s,%s,%d-%d\t.\t.\t.\tPASS\t%s\tGT:DS%s\n" %
                             (CHROM.replace("chr", ""), pos, case["beds"][bi][0], name, a, z, g[1], g[2]))
                pos += 1
    return "".join(lines), len(lines), pos


def check(sc, b, pats, case, host=True, **kw):
    """score_rows == the reference == the host function; the count-only call agrees.  Returns the text."""
    got = b.score_rows(sc, CHROM, **kw)
    want = S.expected_text(CHROM, pats, case["regions"], case["beds"], case["seqs"], kw.get("min_maf", 0),
                           kw.get("min_spread", 1), kw.get("fake_position", 1))
    assert got == want
    if host:
        assert host_text(sc, b, pats, case, kw.get("min_maf", 0), kw.get("min_spread", 1), kw.get("fake_position", 1)) == got
    counted = b.score_rows(sc, CHROM, **dict(kw, fake_position=None))
    assert counted == ("", got[1], None)
    return got[0]


def uploaded(sc, ps, case, **kw):
    b = SC.build(ps, case, **kw)
    b.upload(sc)
    return b


def fields_of(line):
    return line.rstrip("\n").split("\t")


@pytest.mark.parametrize("n", SC.SAMPLE_COUNTS)
def test_sample_counts(n):
    """One lane, a wave's edge, a tile's edge (512 samples), several tiles; 8- and 11-byte fields mixed."""
    case = SC.sample_case(n)
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        text = check(sc, uploaded(sc, ps, case), case["pats"], case)
    assert (text == "") == (n == 1)
    for line in text.splitlines():
        assert len(fields_of(line)) == 9 + n


@pytest.mark.parametrize("kind", ["one", "two", "pairs"])
def test_haplotype_counts(kind):
    case = SC.haps_case(kind)
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, case["pats"], case)
        assert b.region_stats(0)[0] == {"one": 1, "two": 2, "pairs": 4}[kind]
    assert (text == "") == (kind == "one")


@pytest.mark.parametrize("name", ["patterns", "extreme", "none", "keys"])
def test_patterns_and_keys(name):
    """patterns: a reverse strand that wins, a tie between strands, a dinucleotide id, a strand of 36
    columns, a TFBS_KIND_OTHER id; extreme: the spread 2^33 - 2; none: a carried haplotype without a
    window under the narrow range; keys: two beds, nested, duplicated and empty ranges, forty ranges."""
    case = getattr(SC, name + "_case")()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, case["pats"], case)
        if name == "keys":
            assert len(b.ranges(0)) == 42
    assert text
    if name == "patterns":
        assert ",other," not in text and ",long," in text and ",tie," in text
    if name == "extreme":
        assert text == "7\t1\ta.bed,one,%d-%d\t.\t.\t.\tPASS\tSCORES=-4294967296,4294967294;freqs=1/1/1\tGT:DS" \
            "\t1|1:2.0\t0|0:0.0\t0|1:1.0000\n" % case["regions"][0]["inner"][0][1:]
    if name == "none":
        assert "w.bed," in text and "n.bed," not in text


@pytest.mark.parametrize("name", ["case_all_kernels", "case_geometry", "case_n_and_indels", "case_reduction"])
def test_dinuc_cases(name):
    """The count path's cases: every kernel's strands, one-window haplotypes, N and indels, more
    ranges than one sweep of the best kernel takes."""
    case = getattr(K, name)()
    pats = sorted(case["mono"] + case["pats"], key=lambda p: p.pattern_id) if "mono" in case else case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = build_batch(ps, case["n"], case["beds"], case["regions"])
        b.upload(sc)
        check(sc, b, pats, case, host=name != "case_reduction")


def test_arguments():
    """min_maf and min_spread at the values that just keep and just drop a row; POS over sub-ranges."""
    case = SC.multi_case()
    pats = case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, pats, case, fake_position=17)
        rows = [fields_of(l) for l in text.splitlines()]
        assert [int(r[1]) for r in rows] == list(range(17, 17 + len(rows)))
        spreads, mafs = [], []
        for r in rows:
            info = dict(kv.split("=") for kv in r[7].split(";"))
            lo, hi = (int(x) for x in info["SCORES"].split(","))
            spreads.append(hi - lo)
            mafs.append(S.maf_of(*(int(x) for x in info["freqs"].split("/"))))
        assert len(set(spreads)) > 3 and len(set(mafs)) > 2
        for v in sorted(set(spreads))[1:3]:  # v keeps the rows of spread v, v + 1 drops them
            kept = check(sc, b, pats, case, host=False, min_spread=v)
            assert kept.count("\n") == sum(x >= v for x in spreads)
            assert check(sc, b, pats, case, host=False, min_spread=v + 1).count("\n") == sum(x > v for x in spreads)
        for v in sorted(set(mafs))[1:3]:
            assert check(sc, b, pats, case, host=False, min_maf=v).count("\n") == sum(x >= v for x in mafs)
            assert check(sc, b, pats, case, host=False, min_maf=v + 1).count("\n") == sum(x > v for x in mafs)
        # sub-ranges continue the numbering and add up to the whole
        for cuts in ((0, 2, 5), (0, 1, 2, 3, 4, 5), (0, 0, 5, 5)):
            parts, pos, n_rows = [], 17, 0
            for r0, r1 in zip(cuts, cuts[1:]):
                t, n, nxt = b.score_rows(sc, CHROM, fake_position=pos, r0=r0, r1=r1)
                assert nxt == pos + n == pos + t.count("\n")
                assert b.score_rows(sc, CHROM, fake_position=None, r0=r0, r1=r1)[1] == n
                parts.append(t)
                pos, n_rows = nxt, n_rows + n
            assert "".join(parts) == text and n_rows == len(rows)


def test_scratch_budget(monkeypatch):
    """TFBS_SCORES_SCRATCH_MB of 0 (a region and a row at a time), 0.05 and the default: equal text."""
    case = SC.multi_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, case["pats"], case, host=False)
        for mb in ("0", "0.05"):
            monkeypatch.setenv("TFBS_SCORES_SCRATCH_MB", mb)
            assert b.score_rows(sc, CHROM)[0] == text, mb
        monkeypatch.delenv("TFBS_SCORES_SCRATCH_MB")
        assert b.score_rows(sc, CHROM)[0] == text


def test_pair_table_fallback():
    """8 193 distinct pairs: the region's rows come from the host function on the folded values."""
    case = SC.fallback_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        assert b.region_stats(0)[0] == 91
        text = check(sc, b, case["pats"], case)
    assert text.count("\n") >= 1 and all(len(fields_of(l)) == 9 + case["n"] for l in text.splitlines())


def test_device_grouped_and_host_built_regions():
    case = SC.multi_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        host = uploaded(sc, ps, case)
        text = check(sc, host, case["pats"], case, host=False)
        dev = uploaded(sc, ps, case, build_device=0)
        nd, nh = dev.build_stats()
        assert nd >= 3 and nh >= 1, (nd, nh)
        assert check(sc, dev, case["pats"], case) == text


def test_nothing_else_disturbed():
    """Around a call the region digests, a replayed step and the best / hits results are unchanged;
    the call's preconditions."""
    case = SC.multi_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    L = T.lib()
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        n = b.num_regions
        b.scan(sc, upload=False, reduce=True)
        want = [b.digest(r) for r in range(n)]
        for _ in range(3):  # (from the third step alike a graph replay)
            T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(n)] == want
        best, hits = b.best(sc), b.hits(sc)
        best_ms = sc.last_best_ms()
        text, rows, _ = b.score_rows(sc, CHROM)
        assert rows > 0
        ms = sc.last_scores_ms()
        assert len(ms) == 4 and all(m > 0 for m in ms)
        assert sc.last_best_ms() == best_ms
        assert [b.digest(r) for r in range(n)] == want
        T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(n)] == want
        assert np.array_equal(b.best(sc), best) and np.array_equal(b.hits(sc), hits)
        assert b.score_rows(sc, CHROM)[0] == text
        other = SC.build(ps, case)
        with pytest.raises(T.TfbsError) as ei:
            other.score_rows(sc, CHROM)
        assert ei.value.code == -14  # TFBS_E_STATE: not resident
        for r0, r1 in ((2, 1), (0, n + 1)):
            with pytest.raises(T.TfbsError) as ei:
                b.score_rows(sc, CHROM, r0=r0, r1=r1)
            assert ei.value.code == -1  # TFBS_E_ARG
        bare = uploaded(sc, ps, case, keep_membership=False)
        with pytest.raises(T.TfbsError) as ei:
            bare.score_rows(sc, CHROM)
        assert ei.value.code == -14  # made without membership


# ------------------------------------------------------------ run flow and command line
BEDS = [os.path.join(TD, "regions1.bed"), os.path.join(TD, "regions2.bed")]


def run_fixture(out, **kw):
    T.run("chr1", os.path.join(TD, "genotypes2.bcf"), BEDS, os.path.join(TD, "reference_genome.fa"),
          os.path.join(TD, "samples"), os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"], str(out), **kw)
    return T.bgzf_read(str(out))


def fixture_expected(ps, min_spread):
    """score_ref's text of the reference's test data: the merged regions through BcfReader and
    fasta_fetch, the per-haplotype-id sequences from the batch's distinct haplotypes and membership."""
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
    seqs = []
    for r in range(b.num_regions):
        order = [(tuple(c), tuple(p)) for c, p in H.library_order(b, r)]
        seqs.append([order[m] for m in b.membership(r)])
    regions = [{"merged": m} for m in merged]
    return S.expected_text("chr1", ps.to_list(), regions, beds, seqs, 0, min_spread)[0]


def test_run_flow_and_cli_scores_output(tmp_path):
    main = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    header = main[:main.index("\n") + 1]
    assert header.startswith("#CHROM\t")
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    want = header + fixture_expected(ps, 1)
    assert want.count("\n") > 1  # the fixture's one polymorphism moves a best score
    for k, kw in enumerate(({"regions_per_batch": 1}, {"regions_per_batch": 512},
                            {"devices": [0], "regions_per_batch": 1}, {"devices": [0, 0], "regions_per_batch": 1})):
        out, sout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("s%d.vcf.gz" % k)
        assert run_fixture(out, scores_output=str(sout), **kw) == main, kw
        assert T.bgzf_read(str(sout)) == want, kw
        assert not os.path.exists(str(sout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    out, sout = tmp_path / "cli.vcf.gz", tmp_path / "cli_scores.vcf.gz"
    r = subprocess.run([exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed",
                        ",".join(BEDS), "--reference", os.path.join(TD, "reference_genome.fa"), "--samples",
                        os.path.join(TD, "samples"), "--pwm_file", os.path.join(TD, "pwm_definitions.txt"),
                        "--pwm_threshold_directory", TD, "--pwm_threshold", "0.0001", "--pwm_names", "ACGT",
                        "--output", str(out), "--scores_output", str(sout), "--scores_min_spread", "1000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert T.bgzf_read(str(out)) == main
    assert T.bgzf_read(str(sout)) == header + fixture_expected(ps, 1000)
