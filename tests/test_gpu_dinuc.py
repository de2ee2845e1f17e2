"""Dinucleotide PWMs on the GPU: scan_dinuc_kernel through the C ABI against the plain
Python restatement of the semantics (dinuc_ref.py), and, for dinucleotide PWMs that
embed a mono PWM, against the CPU oracle.  Integer work: every comparison is exact."""
import os
import random
import shutil
import subprocess

import pytest

import dinuc_ref as D
from helpers import GOLD, TD, T, build_batch, make_regions_synth, run_oracle, run_product, synth_patterns

pytestmark = pytest.mark.gpu

NUC = "ACGT"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


def rand_rows(rnd, L):
    return [[rnd.randint(-2000, 2000) for _ in range(16)] for _ in range(L - 1)]


def quantile_threshold(all_scores, frac=0.88):
    """An attained score with about 1 - frac of the scores strictly above it."""
    s = sorted(all_scores)
    return s[min(len(s) - 1, int(frac * len(s)))]


def make_set(rnd, lengths, per_length, calib):
    """per_length pattern ids x 2 strands for every length, thresholds at a quantile of the
    reference's own scores on `calib` (an attained score: equality must not hit)."""
    pats, pid = [], 0
    for L in lengths:
        for _ in range(per_length):
            rows = rand_rows(rnd, L)
            for d, rw in ((T.DIR_P, rows), (T.DIR_N, D.reverse_rows(rows))):
                pats.append(T.Pattern.DiPWM(rw, "di%d" % pid, pid, quantile_threshold(D.scores(rw, calib)), d))
            pid += 1
    return pats


def check_matches(sc, pats, codes, pos):
    hap = [(NUC[c] if c < 4 else "N", p) for c, p in zip(codes, pos)]
    got = sc.matches_all(hap)
    n = 0
    for i, p in enumerate(pats):
        want = D.matches(p.weights, p.min_score, codes, pos)
        assert got[i] == want, (i, len(p), len(codes))
        n += len(want)
    return n


def test_matches_fuzz_vs_reference():
    """Base lengths on either side of a k-mer block boundary (k = 3 and 5), one row and the
    maximum; haplotype lengths with no window, one window, and the 16-base word, 64-window
    chunk and 256-window pass edges; 9 pattern ids x 2 strands per length."""
    rnd = random.Random(101)
    lengths = [2, 3, 5, 6, 9, 17, 31, 32]
    calib = [rnd.randrange(4) for _ in range(300)]
    pats = make_set(rnd, lengths, 9, calib)
    hap_lens = sorted({L - 1 for L in lengths} | set(lengths) | {63, 64, 65, 255, 257})
    sc = T.Scanner(pats)
    try:
        hits = check_matches(sc, pats, calib, list(range(1000, 1300)))  # 300 bases
        # equality is a non-hit: every threshold is a score some window of calib attains
        for p in pats:
            assert p.min_score in D.scores(p.weights, calib)
        for n in hap_lens:
            codes = [rnd.randrange(4) for _ in range(n)]
            hits += check_matches(sc, pats, codes, list(range(5, 5 + n)))
    finally:
        sc.close()
    assert hits >= 20


def test_n_and_positions_vs_reference():
    """N (a pair holding one adds 0) as the first and the last base of windows, alone, at
    either end of the haplotype and as a run of 3; positions with a repeated value (inserted
    bases) and a gap (a deletion): start and end come from pos[i]."""
    rnd = random.Random(202)
    n = 300
    codes = [rnd.randrange(4) for _ in range(n)]
    for i in (0, 40, 100, 101, 102, 170, n - 1):
        codes[i] = 4
    pos, p = [], 7000
    for i in range(n):
        pos.append(p)
        if not 60 <= i < 64:  # four inserted bases repeat the position
            p += 1
        if i == 200:  # a deletion of 9 bases
            p += 9
    pats = make_set(rnd, [2, 4, 9, 16, 32], 3, codes)
    sc = T.Scanner(pats)
    try:
        hits = check_matches(sc, pats, codes, pos)
        hits += check_matches(sc, pats, codes, list(range(n)))
        hits += check_matches(sc, pats, [4] * 40 + codes[:30], list(range(70)))
    finally:
        sc.close()
    assert hits >= 20
    # the reference itself: some hit windows contain an N
    with_n = sum(1 for q in pats for i, v in enumerate(D.scores(q.weights, codes))
                 if v > q.min_score and 4 in codes[i:i + len(q)])
    assert with_n >= 1


def embedded(mono_set):
    """The dinucleotide set scoring N-free windows exactly as the mono set does."""
    return T.PatternSet.from_patterns([
        T.Pattern.DiPWM(D.embed_mono([w.acgtn[:4] for w in p.weights]), p.name, p.pattern_id, p.min_score,
                        p.direction) for p in mono_set.to_list()])


def nested_beds(regions):
    a, b = [], []
    for reg in regions:
        s, e = reg["merged"]
        a.append((s, e))
        # (a bed range is an inner peak only if it holds an end of the merged region, main.rs:62-72)
        b += [(s, s + 60), (s, s + 40), (s + 30, e), (s + 50, s + 70)]
    return [("a.bed", a), ("b.bed", b)]


@pytest.mark.parametrize("indel", [0, 30])
def test_full_flow_vs_oracle_by_embedding(tmp_path, indel):
    """keys and rows with embedded dinucleotide PWMs equal the oracle's on the mono PWMs,
    through the dense download, the device reduction and the device encoding."""
    mono, _ = synth_patterns(tmp_path, 6, 2, 31, thr=2e-3)
    di = embedded(mono)
    n = 8
    regions = make_regions_synth(5, 0, 3, n, mono.max_length, indel)
    assert all("N" not in r["ref"] for r in regions)
    beds = nested_beds(regions)
    okeys, orows, _ = run_oracle(mono, n, beds, regions)
    assert sum(sum(l) + sum(r) for k in okeys for l, r in k.values()) >= 20
    sc = T.Scanner(di)
    try:
        for reduce, encode in ((False, False), (True, False), (True, True)):
            pkeys, prows, _ = run_product(sc, di, n, beds, regions, reduce=reduce, encode=encode)
            assert pkeys == okeys, (reduce, encode)
            assert prows == orows, (reduce, encode)
    finally:
        sc.close()


def snv_regions(rnd, n_samples, lmax, specs):
    """SNV-only regions built by hand; specs: [(merged start, merged length)].  Returns the
    regions and, per region, the sequence (codes) of every haplotype id."""
    probe = T.RegionBatch(T.PatternSet.from_patterns([T.Pattern.DiPWM(rand_rows(rnd, lmax), "p", 0, 0)]), n_samples)
    regions, haps = [], []
    for s, ln in specs:
        e = s + ln - 1
        es, ee = probe.ext(s, e)
        ref = [rnd.randrange(4) for _ in range(ee - es + 1)]
        seqs = [list(ref) for _ in range(2 * n_samples)]
        recs = []
        for k in sorted(rnd.sample(range(len(ref)), 12)):
            alt = rnd.choice([c for c in range(4) if c != ref[k]])
            car = sorted(rnd.sample(range(2 * n_samples), rnd.randint(1, n_samples)))
            recs.append(("car", es + k, NUC[ref[k]], NUC[alt], car))
            for h in car:
                seqs[h][k] = alt
        regions.append({"merged": (s, e), "ref": "".join(NUC[c] for c in ref), "records": recs, "es": es})
        haps.append(seqs)
    return regions, haps


def expected_keys(pats, n_samples, beds, reg, seqs):
    """count_matches_by_sample from the reference: {(bed, range, pattern_id): (L, R)} of the
    keys some haplotype counts for."""
    out = {}
    cache = {}
    for bi, a, z in T.select_inner_peaks(reg["merged"], beds):
        for p in pats:
            key = (beds[bi][0], (a, z), p.pattern_id)
            left, right = out.get(key, ([0] * n_samples, [0] * n_samples))
            for h, seq in enumerate(seqs):
                ck = (id(p), tuple(seq))
                if ck not in cache:
                    cache[ck] = D.matches(p.weights, p.min_score, seq, list(range(reg["es"], reg["es"] + len(seq))))
                c = D.count_overlaps(cache[ck], (a, z))
                (left, right)[h & 1][h >> 1] += c
            out[key] = (left, right)
    return {k: v for k, v in out.items() if any(v[0]) or any(v[1])}


def test_true_dinucleotide_counts_through_a_batch():
    """Per (bed, inner range, pattern_id) left / right vectors of true dinucleotide PWMs on
    SNV-only regions, one with more inner ranges than a counting pass holds (8), one with
    none."""
    rnd = random.Random(303)
    n = 6
    calib = [rnd.randrange(4) for _ in range(400)]
    pats = make_set(rnd, [4, 7, 12], 3, calib)
    ps = T.PatternSet.from_patterns(pats)
    regions, haps = snv_regions(rnd, n, ps.max_length, [(5000, 120), (9000, 150), (20000, 60)])
    s0, s1 = regions[0]["merged"][0], regions[1]["merged"][0]
    beds = [("a.bed", [(s0, s0 + 119), (s1, s1 + 149)]),
            ("b.bed", [(s1, s1 + 30 + 7 * k) for k in range(6)] + [(s1 + 140 - 9 * k, s1 + 149) for k in range(5)] +
             [(s0, s0 + 50), (s0 + 20, s0 + 60)])]
    assert len(T.select_inner_peaks(regions[1]["merged"], beds)) == 12  # more than one pass of 8
    assert len(T.select_inner_peaks(regions[0]["merged"], beds)) == 2  # (s0 + 20, s0 + 60) holds neither end
    assert T.select_inner_peaks(regions[2]["merged"], beds) == []
    sc = T.Scanner(ps)
    try:
        b = build_batch(ps, n, beds, regions)
        b.scan(sc)
        total = 0
        for i, reg in enumerate(regions):
            want = expected_keys(pats, n, beds, reg, haps[i])
            assert b.keys(i) == want, i
            total += sum(sum(l) + sum(r) for l, r in want.values())
        assert b.keys(2) == {}
    finally:
        sc.close()
    assert total >= 20


def test_mixed_mono_and_dinucleotide_set(tmp_path):
    """Mono PWMs (matrix-core slots) and dinucleotide PWMs in one set: the mono keys are the
    oracle's, the dinucleotide keys those of a dinucleotide-only run, also after four
    tfbs_step calls (the captured step graph)."""
    mono, _ = synth_patterns(tmp_path, 6, 2, 31, thr=2e-3)
    ml = mono.to_list()
    n = 8
    regions = make_regions_synth(5, 0, 3, n, mono.max_length, 30)
    beds = nested_beds(regions)
    rnd = random.Random(404)
    calib = [NUC.index(c) for c in regions[0]["ref"]]
    first = max(p.pattern_id for p in ml) + 1
    dl = make_set(rnd, [5, 9, mono.max_length], 2, calib)
    for p in dl:
        p.pattern_id += first
    di_ids = {p.pattern_id for p in dl}
    okeys, _, _ = run_oracle(mono, n, beds, regions)
    di_only = T.PatternSet.from_patterns(dl)
    sc = T.Scanner(di_only)
    try:
        dkeys, _, _ = run_product(sc, di_only, n, beds, regions)
    finally:
        sc.close()
    assert sum(sum(l) + sum(r) for k in dkeys for l, r in k.values()) >= 20
    mixed = T.PatternSet.from_patterns(ml + dl)
    assert mixed.plan_stats(mfma=True)["n_mfma_strands"] > 0 and mixed.dinuc_stats()["n_strands"] == len(dl)
    sc = T.Scanner(mixed)
    try:
        def split(b):
            ks = [b.keys(i) for i in range(b.num_regions)]
            return ([{k: v for k, v in r.items() if k[2] not in di_ids} for r in ks],
                    [{k: v for k, v in r.items() if k[2] in di_ids} for r in ks])
        b = build_batch(mixed, n, beds, regions)
        b.scan(sc, reduce=True)
        assert split(b) == (okeys, dkeys)
        for _ in range(4):
            T.check(T.lib().tfbs_step(sc.h, b.h))
        T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
        assert split(b) == (okeys, dkeys)
    finally:
        sc.close()


def test_run_flow_and_cli_with_dipwm_file(tmp_path):
    """tfbs_run and the command line with --dipwm_file alone on the reference's test data:
    the embedding of pwm_definitions.txt's ACGT gives expected_output_2's rows under the
    dinucleotide pattern's name."""
    mono = [[float(x) for x in line.split()] for line in open(os.path.join(TD, "pwm_definitions.txt"))
            if not line.startswith(">") and line.strip()]
    thr = tmp_path / "thr"
    thr.mkdir()
    shutil.copy(os.path.join(TD, "ACGT.thr"), str(thr / "DIACGT.thr"))
    di_file = tmp_path / "di.txt"
    with open(str(di_file), "w") as f:
        f.write(">DIACGT\n")
        for row in D.embed_mono(mono):
            f.write("\t".join("%.1f" % x for x in row) + "\n")
    want = open(os.path.join(GOLD, "expected_output_2.vcf")).read().replace(",ACGT,", ",DIACGT,")
    assert ",DIACGT," in want and "COUNTS=2,4" in want  # (the fixture's one row: 14 hits over 4 samples)
    beds = [os.path.join(TD, "regions1.bed"), os.path.join(TD, "regions2.bed")]
    out = tmp_path / "out.vcf.gz"
    T.run("chr1", os.path.join(TD, "genotypes2.bcf"), beds, os.path.join(TD, "reference_genome.fa"),
          os.path.join(TD, "samples"), None, str(thr), 0.0001, ["DIACGT"], str(out), dipwm_file=str(di_file))
    assert T.bgzf_read(str(out)) == want
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    out2 = tmp_path / "cli.vcf.gz"
    r = subprocess.run([exe, "--chromosome", "chr1", "--input", os.path.join(TD, "genotypes2.bcf"), "--bed",
                        ",".join(beds), "--reference", os.path.join(TD, "reference_genome.fa"), "--samples",
                        os.path.join(TD, "samples"), "--dipwm_file", str(di_file), "--pwm_threshold_directory",
                        str(thr), "--pwm_threshold", "0.0001", "--pwm_names", "DIACGT", "--output", str(out2)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert T.bgzf_read(str(out2)) == want
