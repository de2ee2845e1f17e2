"""The affinity rows (affinity_rows.hip) through RegionBatch.affinity_rows.  What the device's text
must equal is built by a route that shares no code with the new kernels: b.affinity()'s records,
folded per pattern id in Python through the membership, then the plain Python model
(affinity_rows_ref.py); and, from the same folded values, the host function
(tfbs_affinity_as_genotypes), byte for byte.  The cases are score_cases.py's and
affinity_rows_cases.py's (test_affinity_rows_cpu.py shows on the references alone that each bites).
Integer work: every comparison is exact."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import affinity_ref as A
import affinity_rows_cases as AC
import affinity_rows_ref as M
import best_ref as R
import oracle_py as O
import score_cases as SC
import score_ref as S
from helpers import GOLD, TD, T

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


def uploaded(sc, ps, case, **kw):
    b = SC.build(ps, case, **kw)
    b.upload(sc)
    return b


def folded(sc, b, pats, r0=0, r1=None):
    """Per region of [r0, r1) a function value(pid, range, haplotype id) -> (A, N) from the library's
    own affinity records and membership."""
    aff = b.affinity(sc)
    out = []
    for r in range(r0, b.num_regions if r1 is None else r1):
        ranges = b.ranges(r)
        if not ranges:
            out.append(None)
            continue
        sums, counts = b.affinity_by_sample(aff, r)  # [haplotype id][strand][range]
        strands = {pid: [i for i, p in enumerate(pats) if p.pattern_id == pid] for pid in {p.pattern_id for p in pats}}

        def value(pid, rng, x, sums=sums, counts=counts, ranges=ranges):
            k = ranges.index(rng)
            return (sum(int(sums[x, i, k]) for i in strands[pid]), sum(int(counts[x, i, k]) for i in strands[pid]))

        out.append(value)
    return out


def route_text(sc, b, pats, case, min_maf=0, min_spread=1, pos=1, r0=0, r1=None, host=False):
    """The expected (text, rows, next POS): records -> Python fold -> the model (host: -> the host function)."""
    beds, n = case["beds"], case["n"]
    regions = case["regions"][r0:b.num_regions if r1 is None else r1]
    vals = folded(sc, b, pats, r0, r1)
    tops = A.tops(pats)
    per_region = []
    for reg, value in zip(regions, vals):
        if value is None:
            per_region.append([])
        elif not host:
            per_region.append(M.rows_of(pats, reg, beds, n, value, min_maf, min_spread))
        else:
            rows = []
            for a, z, bi in sorted({(a, z, bi) for bi, a, z in R.inner_of(reg, beds) if z >= a}):
                for pid in sorted({p.pattern_id for p in pats}):
                    v = [value(pid, (a, z), x) for x in range(2 * n)]
                    if any(x[1] == 0 for x in v):
                        continue
                    first = next(i for i, p in enumerate(pats) if p.pattern_id == pid)
                    g = T.affinity_as_genotypes([x[0] for x in v[0::2]], [x[0] for x in v[1::2]], tops[first], min_spread)
                    if g is not None and g[0] >= min_maf:
                        rows.append((beds[bi][0], pats[first].name, a, z, g[1], g[2]))
            per_region.append(rows)
    return M.text_of(CHROM, per_region, pos)


def check(sc, b, pats, case, host=True, **kw):
    """affinity_rows == records -> fold -> model == records -> fold -> host function; the count-only call agrees."""
    got = b.affinity_rows(sc, CHROM, **kw)
    args = (kw.get("min_maf", 0), kw.get("min_spread", 1), kw.get("fake_position", 1))
    assert got == route_text(sc, b, pats, case, *args)
    if host:
        assert got == route_text(sc, b, pats, case, *args, host=True)
    assert b.affinity_rows(sc, CHROM, **dict(kw, fake_position=None)) == ("", got[1], None)
    return got[0]


def fields_of(line):
    return line.rstrip("\n").split("\t")


def field_lengths(line):
    return {len(f) + 1 for f in fields_of(line)[9:]}


@pytest.mark.parametrize("n", SC.SAMPLE_COUNTS)
def test_sample_counts(n):
    """One lane, a wave's edge, a tile's edge (512 samples), several tiles of the text kernel; the
    statistics kernel's 256 threads against the pairs; 8- and 11-byte fields mixed."""
    case = SC.sample_case(n)
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        text = check(sc, uploaded(sc, ps, case), case["pats"], case)
    assert (text == "") == (n == 1)
    for line in text.splitlines():
        assert len(fields_of(line)) == 9 + n
        if n >= 63:
            assert field_lengths(line) == {8, 11}


@pytest.mark.parametrize("kind", ["one", "two", "pairs"])
def test_haplotype_counts(kind):
    case = SC.haps_case(kind)
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, case["pats"], case)
        assert b.region_stats(0)[0] == {"one": 1, "two": 2, "pairs": 4}[kind]
    assert (text == "") == (kind == "one")


@pytest.mark.parametrize("name", ["patterns", "long", "none", "keys", "zero", "large"])
def test_patterns_keys_and_sums(name):
    """patterns: two strands per id that add, a dinucleotide id, a TFBS_KIND_OTHER id (no row) and a
    36-column strand whose sums are all 0 (no row); long: a 36-column strand inside the cutoff; none:
    a carried haplotype without a window under the narrow range; keys: two beds, nested, duplicated
    and empty ranges, forty ranges; zero: samples with x = 0, lo = -1; large: sums near 2^49."""
    case = (getattr(SC, name + "_case", None) or getattr(AC, name + "_case"))()
    pats = case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, pats, case)
        if name == "keys":
            assert len(b.ranges(0)) == 42
    assert text
    if name == "patterns":
        assert ",other," not in text and ",fr," in text and ",tie," in text and ",di2," in text
    if name == "long":
        assert ",long," in text
    if name == "none":
        assert "w.bed," in text and "n.bed," not in text
    if name == "zero":
        assert text == "7\t1\ta.bed,zero,%d-%d\t.\t.\t.\tPASS\tLOG2AFF=-1,41000;AFF=0,2199023255552;TOP=0;freqs=1/0/2" \
            "\tGT:DS\t1|1:2.0\t0|0:0.0\t1|1:1.9512\n" % case["regions"][0]["inner"][0][1:]
    if name == "large":
        xlo, xhi = (int(x) for x in fields_of(text)[7].split(";")[1][4:].split(","))
        assert xlo > 500 << 40 and xlo % (1 << 40) == 0 and xhi % (1 << 40) == 0 and xhi > xlo


def test_refused_set():
    """extreme_case's weights can wrap int32: refused exactly as b.affinity() refuses it, each time."""
    case = SC.extreme_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        with pytest.raises(T.TfbsError) as want:
            b.affinity(sc)
        for kw in ({}, {"fake_position": None}):
            with pytest.raises(T.TfbsError) as ei:
                b.affinity_rows(sc, CHROM, **kw)
            assert (ei.value.code, str(ei.value)) == (want.value.code, str(want.value))
        assert want.value.code == -1 and "can wrap int32" in str(want.value)
        assert sc.last_affinity_rows_ms() == (0.0, 0.0, 0.0, 0.0)
        assert b.score_rows(sc, CHROM)[1] == 1  # (the ctx goes on working)


def test_mlog2_kernel_on_the_table_boundaries():
    """The device function on every boundary of the table at six exponents, in one launch."""
    xs = AC.boundary_values()
    got = T.affinity_mlog2(xs, device=0)
    assert [(x, g, M.mlog2(x)) for x, g in zip(xs, got) if g != M.mlog2(x)] == []
    assert got == T.affinity_mlog2(xs)
    assert T.affinity_mlog2([], device=0) == [] and T.affinity_mlog2([0, 1, (1 << 64) - 1], device=0) == [-1, 0, 63999]


def test_pair_table_fallback():
    """8 193 distinct pairs: the region's rows come from the host function on the folded values."""
    case = SC.fallback_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        assert b.region_stats(0)[0] == 91
        text = check(sc, b, case["pats"], case, host=False)
    assert text.count("\n") >= 1 and all(len(fields_of(l)) == 9 + case["n"] for l in text.splitlines())


def test_scratch_budget(monkeypatch):
    """TFBS_AFFINITY_ROWS_SCRATCH_MB of 0 (a region and a row at a time), 0.05 and the default: equal text."""
    case = SC.multi_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        text = check(sc, b, case["pats"], case, host=False)
        assert text.count("\n") >= 8
        for mb in ("0", "0.05"):
            monkeypatch.setenv("TFBS_AFFINITY_ROWS_SCRATCH_MB", mb)
            assert b.affinity_rows(sc, CHROM)[0] == text, mb
        monkeypatch.delenv("TFBS_AFFINITY_ROWS_SCRATCH_MB")
        assert b.affinity_rows(sc, CHROM)[0] == text


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


def test_arguments():
    """min_maf and min_spread at the values that just keep and just drop a row; POS over sub-ranges;
    the call's preconditions."""
    case = SC.multi_case()
    pats = case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = uploaded(sc, ps, case)
        n = b.num_regions
        text = check(sc, b, pats, case, fake_position=17)
        rows = [fields_of(l) for l in text.splitlines()]
        assert [int(r[1]) for r in rows] == list(range(17, 17 + len(rows)))
        spreads, mafs = [], []
        for r in rows:
            info = dict(kv.split("=") for kv in r[7].split(";"))
            lo, hi = (int(x) for x in info["LOG2AFF"].split(","))
            xlo, xhi = (int(x) for x in info["AFF"].split(","))
            assert (lo, hi) == (M.mlog2(xlo), M.mlog2(xhi))
            spreads.append(hi - lo)
            mafs.append(S.maf_of(*(int(x) for x in info["freqs"].split("/"))))
        assert len(set(spreads)) > 3 and len(set(mafs)) > 2
        for v in sorted(set(spreads))[1:3]:  # v keeps the rows of spread v, v + 1 drops them
            assert check(sc, b, pats, case, host=False, min_spread=v).count("\n") == sum(x >= v for x in spreads)
            assert check(sc, b, pats, case, host=False, min_spread=v + 1).count("\n") == sum(x > v for x in spreads)
        assert b.affinity_rows(sc, CHROM, min_spread=0, fake_position=17)[0] == text
        for v in sorted(set(mafs))[1:3]:
            assert check(sc, b, pats, case, host=False, min_maf=v).count("\n") == sum(x >= v for x in mafs)
            assert check(sc, b, pats, case, host=False, min_maf=v + 1).count("\n") == sum(x > v for x in mafs)
        for cuts in ((0, 2, 5), (0, 1, 2, 3, 4, 5), (0, 0, 5, 5)):  # sub-ranges continue the numbering
            parts, pos, n_rows = [], 17, 0
            for r0, r1 in zip(cuts, cuts[1:]):
                t, k, nxt = b.affinity_rows(sc, CHROM, fake_position=pos, r0=r0, r1=r1)
                assert nxt == pos + k == pos + t.count("\n")
                assert b.affinity_rows(sc, CHROM, fake_position=None, r0=r0, r1=r1)[1] == k
                parts.append(t)
                pos, n_rows = nxt, n_rows + k
            assert "".join(parts) == text and n_rows == len(rows)
        other = SC.build(ps, case)
        with pytest.raises(T.TfbsError) as ei:
            other.affinity_rows(sc, CHROM)
        assert ei.value.code == -14  # TFBS_E_STATE: not resident
        for r0, r1 in ((2, 1), (0, n + 1)):
            with pytest.raises(T.TfbsError) as ei:
                b.affinity_rows(sc, CHROM, r0=r0, r1=r1)
            assert ei.value.code == -1  # TFBS_E_ARG
        bare = uploaded(sc, ps, case, keep_membership=False)
        with pytest.raises(T.TfbsError) as ei:
            bare.affinity_rows(sc, CHROM)
        assert ei.value.code == -14  # made without membership


def test_nothing_else_disturbed():
    """Around a call the region digests, a replayed step, the rows, the score rows, the affinity, best
    and hits records and their timers are unchanged; a batch's device bytes do not depend on it."""
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
        best, hits, aff, scores = b.best(sc), b.hits(sc), b.affinity(sc), b.score_rows(sc, CHROM)
        timers = (sc.last_best_ms(), sc.last_affinity_ms(), sc.last_scores_ms())
        main_rows = b.rows(CHROM)
        bytes_before = b.input_bytes
        text, rows, _ = b.affinity_rows(sc, CHROM)
        assert rows > 0
        ms = sc.last_affinity_rows_ms()
        assert len(ms) == 4 and all(m > 0 for m in ms)
        assert (sc.last_best_ms(), sc.last_affinity_ms(), sc.last_scores_ms()) == timers
        assert b.input_bytes == bytes_before and b.rows(CHROM) == main_rows
        assert [b.digest(r) for r in range(n)] == want
        T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(n)] == want
        assert np.array_equal(b.best(sc), best) and np.array_equal(b.hits(sc), hits) and np.array_equal(b.affinity(sc), aff)
        assert b.score_rows(sc, CHROM) == scores and b.rows(CHROM) == main_rows
        assert b.affinity_rows(sc, CHROM)[0] == text
    with scanner(ps) as sc:  # a ctx that never calls the feature: the same batch bytes, no timers
        b2 = uploaded(sc, ps, case)
        assert b2.input_bytes == bytes_before
        assert sc.last_affinity_rows_ms() == (0.0, 0.0, 0.0, 0.0)
        assert b2.score_rows(sc, CHROM) == scores  # (the shared frame made by the score rows alone)
        assert b2.affinity_rows(sc, CHROM)[0] == text  # (and then used by the affinity rows)


# ------------------------------------------------------------ run flow and command line
BEDS = [os.path.join(TD, "regions1.bed"), os.path.join(TD, "regions2.bed")]


def run_fixture(out, **kw):
    T.run("chr1", os.path.join(TD, "genotypes2.bcf"), BEDS, os.path.join(TD, "reference_genome.fa"),
          os.path.join(TD, "samples"), os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"], str(out), **kw)
    return T.bgzf_read(str(out))


def fixture_batch_text(ps, min_spread):
    """The batch API's text of the reference's test data: the merged regions through BcfReader and
    fasta_fetch into one batch, uploaded."""
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
    with scanner(ps) as sc:
        b.upload(sc)
        text = b.affinity_rows(sc, "chr1", min_spread=min_spread)[0]
        pats = ps.to_list()
        rows = [M.rows_of(pats, {"merged": m}, beds, len(rd.selected), v, 0, min_spread) if v else []
                for m, v in zip(merged, folded(sc, b, pats))]
        assert text == M.text_of("chr1", rows)[0]
    return text


def test_run_flow_and_cli_affinity_rows_output(tmp_path):
    main = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    header = main[:main.index("\n") + 1]
    assert header.startswith("#CHROM\t")
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    want = header + fixture_batch_text(ps, 1)
    assert want.count("\n") > 1  # the fixture's one polymorphism moves an affinity
    for k, kw in enumerate(({"regions_per_batch": 1}, {}, {"devices": [0, 0], "regions_per_batch": 1})):
        out, aout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("a%d.vcf.gz" % k)
        assert run_fixture(out, affinity_rows_output=str(aout), **kw) == main, kw
        assert T.bgzf_read(str(aout)) == want, kw
        assert not os.path.exists(str(aout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    base = [exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed", ",".join(BEDS),
            "--reference", os.path.join(TD, "reference_genome.fa"), "--samples", os.path.join(TD, "samples"), "--pwm_file",
            os.path.join(TD, "pwm_definitions.txt"), "--pwm_threshold_directory", TD, "--pwm_threshold", "0.0001",
            "--pwm_names", "ACGT"]
    spread = max(int(l.split("\t")[7].split(";")[0].split(",")[1]) - int(l.split("\t")[7].split(";")[0].split(",")[0][8:])
                 for l in want.splitlines()[1:])
    out, aout = tmp_path / "cli.vcf.gz", tmp_path / "cli_aff.vcf.gz"
    r = subprocess.run(base + ["--output", str(out), "--affinity_rows_output", str(aout), "--affinity_rows_min_spread",
                               str(spread)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert T.bgzf_read(str(out)) == main
    kept = T.bgzf_read(str(aout))
    assert kept == header + fixture_batch_text(ps, spread) and 1 < kept.count("\n") <= want.count("\n")
    r = subprocess.run(base + ["--output", str(tmp_path / "bad.vcf.gz"), "--affinity_rows_output", str(tmp_path / "b.vcf.gz"),
                               "--affinity_rows_min_spread", "wide"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--affinity_rows_min_spread" in r.stderr
    assert not os.path.exists(str(tmp_path / "bad.vcf.gz"))
