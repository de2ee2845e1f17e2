"""The mutation-scan kernel (scan_mutscan.hip) through RegionBatch.mutscan: per (pattern strand,
column of the region's reference window, other base) the best site covering the column before and
after the substitution, against the plain Python restatement (mutscan_ref.py, which rescores every
window); against the variant-effect kernel on the same substitutions as SNV records; the kinds
mask; the scratch budget and sub-ranges; the calls' contract; the run flow's and the command line's
--mutscan_output.  The cases are mutscan_cases.py's and dinuc_cases.py's; test_mutscan_cpu.py checks
from the model alone that each holds every kind.  Integer work: every comparison is exact."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import dinuc_cases as K
import effects_ref as E
import mutscan_cases as MC
import mutscan_ref as M
import test_gpu_effects as TE
from helpers import GOLD, TD, T, build_batch

pytestmark = pytest.mark.gpu

NUC = "ACGT"


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


def get_case(name):
    """(patterns, case) of a name; the model's list is cached under the name (mutscan_ref.expected)."""
    if name.startswith("edges_"):
        case = MC.case_edges()[name[6:]]
        return case["pats"], case
    if name == "special":
        case = MC.case_special_region()
        return case["pats"], case
    case = getattr(K, name)()
    pats = TE.case_patterns(case)
    if name == "case_geometry":
        pats = pats + [T.Pattern.OtherPattern("other", 50)]
    return pats, case


CASES = ["edges_short", "edges_long", "case_all_kernels", "case_n_and_indels", "special", "case_geometry"]


@pytest.mark.parametrize("name", CASES)
def test_reference_equality(name):
    """mutscan(kinds=MUT_ALL) field by field, sparse over the records that exist and sorted."""
    pats, case = get_case(name)
    want = M.expected(pats, case["regions"], key=name)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        got = b.mutscan(sc, kinds=T.MUT_ALL)  # no upload, no scan
        assert b.mutscan_count(sc, kinds=T.MUT_ALL) == len(want)
    assert not got["reserved"].any() and not got["reserved1"].any()
    got = M.as_tuples(got)
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g == w
    keys = [(x[0], x[2], x[1], x[4]) for x in got]  # (region, pattern, column, alt)
    assert keys == sorted(set(keys))
    if name == "case_geometry":  # the TFBS_KIND_OTHER strand and the strands longer than a region have no record
        other = len(pats) - 1
        assert other not in {x[2] for x in got}
        short = [r for r, reg in enumerate(case["regions"]) if len(reg["ref"]) < 9]
        assert short and all(len(pats[x[2]]) <= len(case["regions"][x[0]]["ref"]) for x in got)
    if name == "edges_long":  # the ring's limit: Lr through the ring, Lr + 1 and 2 Lr + 3 through the slow path
        Lr = T.mutscan_ring_max_length()
        assert {len(pats[x[2]]) for x in got} == {64, Lr, Lr + 1, 2 * Lr + 3}


def test_against_the_effects_kernel():
    """Every substitution of the special region as a one-carrier SNV record of a second batch: its
    effects() hold the mutation records' counts, scores, windows and positions."""
    pats, case = get_case("special")
    reg = case["regions"][0]
    codes = K.codes_of(reg["ref"])
    assert len(codes) == 124
    subs = [(c, b) for c in range(len(codes)) if codes[c] != 4 for b in range(4) if b != codes[c]]
    # (the three substitutions of a column on three haplotype ids: each patches alone)
    recs = [("car", reg["es"] + c, NUC[codes[c]], NUC[b], [(b - codes[c]) % 4 - 1]) for c, b in subs]
    reg2 = dict(reg, records=recs)
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        mut = M.as_tuples(b.mutscan(sc, kinds=T.MUT_ALL))
        b2 = E.build_batch(ps, case["n"], case["beds"], [reg2])
        eff = E.as_tuples(b2.effects(sc))
    assert len(eff) == len(subs) * len(pats) == len(mut)  # (every strand fits the region: dense)
    by = {(x[1], x[4], x[2]): x for x in mut}  # (column, alt, pattern)
    for x in eff:  # (region, variant, pattern, status, n_ref, ref_score, ref_window, n_alt, alt_score, alt_window, 4 positions)
        c, alt = subs[x[1]]
        m = by[(c, alt, x[2])]
        assert x[3] == E.SCORED
        assert x[4] == x[7] == m[7]
        assert x[5:7] == m[8:10] and x[8:10] == m[10:12] and x[10:14] == m[12:16]


def test_each_kinds_bit_and_the_count():
    pats, case = get_case("case_n_and_indels")
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        full = b.mutscan(sc, kinds=T.MUT_ALL)
        assert np.array_equal(b.mutscan(sc), full[full["kind"] < 3])  # the default: MUT_SITES
        for k in range(5):
            part = b.mutscan(sc, kinds=1 << k)
            assert len(part) >= 20 and np.array_equal(part, full[full["kind"] == k]), k
        assert np.array_equal(b.mutscan(sc, kinds="gain,none"), full[(full["kind"] == 0) | (full["kind"] == 4)])
        for mask in range(1, 32):
            assert b.mutscan_count(sc, kinds=mask) == int(((mask >> full["kind"].astype(np.int64)) & 1).sum()), mask
        assert b.mutscan_count(sc, 1, 2, kinds=5) == int(((full["region"] == 1) & np.isin(full["kind"], (0, 2))).sum())


def test_scratch_budget_and_subranges(monkeypatch):
    pats, case = get_case("case_n_and_indels")
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        full = b.mutscan(sc, kinds=T.MUT_ALL)
        assert len(full) > 1000 and b.num_regions == 3
        for mb in ("0", "0.01", "256"):  # 0: one region per chunk, one pair per fill
            monkeypatch.setenv("TFBS_MUTSCAN_SCRATCH_MB", mb)
            assert np.array_equal(b.mutscan(sc, kinds=T.MUT_ALL), full), mb
            assert b.mutscan_count(sc, kinds=T.MUT_ALL) == len(full), mb
        monkeypatch.delenv("TFBS_MUTSCAN_SCRATCH_MB")
        for r0 in range(4):
            for r1 in range(r0, 4):
                part = b.mutscan(sc, r0, r1, kinds=T.MUT_ALL)
                assert np.array_equal(part, full[(full["region"] >= r0) & (full["region"] < r1)]), (r0, r1)
        assert np.array_equal(np.concatenate([b.mutscan(sc, r, r + 1, kinds=T.MUT_ALL) for r in range(3)]), full)
    pats, case = get_case("edges_long")  # the slow path's fill, a pair at a time
    ps = T.PatternSet.from_patterns(pats)
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        full = b.mutscan(sc, kinds=T.MUT_SITES)
        monkeypatch.setenv("TFBS_MUTSCAN_SCRATCH_MB", "0")
        assert len(full) and np.array_equal(b.mutscan(sc, kinds=T.MUT_SITES), full)


def test_calls():
    pats, case = get_case("case_n_and_indels")
    ps = T.PatternSet.from_patterns(pats)
    L = T.lib()
    with scanner(ps) as sc:
        b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
        assert sc.last_mutscan_ms() == (0.0, 0.0, 0.0, 0.0)  # a ctx that never scanned mutations holds no state
        full = b.mutscan(sc, kinds=T.MUT_ALL)  # no upload needed
        ms = sc.last_mutscan_ms()
        assert len(ms) == 4 and all(m > 0 for m in ms)
        eff = b.effects(sc)
        b.scan(sc, reduce=True)
        want = [b.digest(r) for r in range(3)]
        rows = b.rows("chr1")[0]
        T.check(L.tfbs_step(sc.h, b.h))
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(3)] == want
        assert np.array_equal(b.mutscan(sc, kinds=T.MUT_ALL), full)
        for _ in range(3):  # (from the third step alike a graph replay)
            T.check(L.tfbs_step(sc.h, b.h))
            assert b.mutscan_count(sc, kinds=T.MUT_ALL) == len(full)
        T.check(L.tfbs_batch_reduce(sc.h, b.h))
        assert [b.digest(r) for r in range(3)] == want
        assert b.rows("chr1")[0] == rows
        assert np.array_equal(b.mutscan(sc, kinds=T.MUT_ALL), full)
        assert b.rows("chr1")[0] == rows and [b.digest(r) for r in range(3)] == want
        assert np.array_equal(b.effects(sc), eff)
        # a batch that keeps no variants; bad ranges; bad masks; another pattern set's scanner
        plain = build_batch(ps, case["n"], case["beds"], case["regions"])
        assert [plain.input_digest(r) for r in range(3)] == [b.input_digest(r) for r in range(3)]
        for call in (plain.mutscan, plain.mutscan_count):
            with pytest.raises(T.TfbsError) as ei:
                call(sc)
            assert ei.value.code == -14  # TFBS_E_STATE
        for call in (b.mutscan, b.mutscan_count):
            for r0, r1, kinds in ((2, 1, 7), (0, 4, 7), (0, 3, 0), (0, 3, 32)):
                with pytest.raises(T.TfbsError) as ei:
                    call(sc, r0, r1, kinds=kinds)
                assert ei.value.code == -1, (r0, r1, kinds)  # TFBS_E_ARG
        assert len(b.mutscan(sc, 1, 1)) == 0 and b.mutscan_count(sc, 1, 1) == 0
    empty = T.PatternSet.from_patterns([T.Pattern.OtherPattern("o", 0)])
    with scanner(empty) as sc:  # a set that scores nothing
        probe = T.RegionBatch(empty, 2, keep_variants=True)
        probe.add_bed("a.bed")
        es, ee = probe.ext(500, 520)
        probe.begin(500, 520, ("ACGT" * 20)[:ee - es + 1])
        probe.add_inner(0, 500, 520)
        probe.end()
        assert len(probe.mutscan(sc, kinds=T.MUT_ALL)) == 0 and probe.mutscan_count(sc, kinds=T.MUT_ALL) == 0
        with pytest.raises(T.TfbsError) as ei:
            b.mutscan(sc)
        assert ei.value.code == -1  # TFBS_E_ARG: another pattern set


# ------------------------------------------------------------ run flow and command line
def test_run_flow_and_cli_mutscan_output(tmp_path):
    main = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    ps = T.parse_pwm_files(os.path.join(TD, "pwm_definitions.txt"), TD, 0.0001, ["ACGT"])
    pats = ps.to_list()
    regions, beds, n = TE.fixture_regions(ps)
    assert len(regions) >= 2
    rows = M.expected(pats, regions)
    modes = {"default": (0, M.GAIN | M.LOSS), "all": ("gain,loss,change,same,none", M.ALL)}
    want = {k: M.HEADER + M.format_tsv("1", pats, regions, [x for x in rows if (mask >> x[5]) & 1])
            for k, (_, mask) in modes.items()}
    assert want["default"].count("\n") > 1 and len(want["all"]) > len(want["default"])
    with scanner(ps) as sc:  # the library's own formatter on its own records says the same
        b = E.build_batch(ps, n, beds, regions)
        mut = b.mutscan(sc, kinds=T.MUT_ALL)
        assert M.as_tuples(mut) == rows
        assert b.mutscan_tsv(mut, "1", header=True) == want["all"]
    k = 0
    for mode, (kinds, _) in modes.items():
        for kw in ({"regions_per_batch": 1}, {"regions_per_batch": 512}, {"devices": [0, 0], "regions_per_batch": 1}):
            k += 1
            out, mout = tmp_path / ("o%d.vcf.gz" % k), tmp_path / ("m%d.tsv.gz" % k)
            assert TE.run_fixture(out, mutscan_output=str(mout), mutscan_kinds=kinds, **kw) == main, (mode, kw)
            assert T.bgzf_read(str(mout)) == want[mode], (mode, kw)
            assert not os.path.exists(str(mout) + ".part")
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    for mode, (kinds, _) in modes.items():
        out, mout = tmp_path / ("cli_%s.vcf.gz" % mode), tmp_path / ("cli_%s.tsv.gz" % mode)
        r = subprocess.run([exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed",
                            ",".join(TE.BEDS), "--reference", os.path.join(TD, "reference_genome.fa"), "--samples",
                            os.path.join(TD, "samples"), "--pwm_file", os.path.join(TD, "pwm_definitions.txt"),
                            "--pwm_threshold_directory", TD, "--pwm_threshold", "0.0001", "--pwm_names", "ACGT",
                            "--output", str(out), "--mutscan_output", str(mout)] +
                           (["--mutscan_kinds", kinds] if kinds else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert T.bgzf_read(str(out)) == main
        assert T.bgzf_read(str(mout)) == want[mode]
        assert not os.path.exists(str(mout) + ".part")
