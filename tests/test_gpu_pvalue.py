"""Thresholds from a p-value on the device (score_dist.hip): every case of the host tests
against the model and the host twin, bit for bit; chunks of mixed strands under three
scratch budgets; spans at the kernels' tile edges; the run flow and the command line."""
import os
import subprocess

import pytest

import pvalue_cases as K
from helpers import GOLD, TD, T

pytestmark = pytest.mark.gpu

HOST, DEV = -1, 0
TFBS_E_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def all_set():
    return K.pattern_set(K.ALL)


@pytest.fixture
def scratch_mb():
    """Sets TFBS_PVALUE_SCRATCH_MB (read at the call) and puts it back."""
    old = os.environ.get("TFBS_PVALUE_SCRATCH_MB")

    def set_(v):
        if v is None:
            os.environ.pop("TFBS_PVALUE_SCRATCH_MB", None)
        else:
            os.environ["TFBS_PVALUE_SCRATCH_MB"] = v
    yield set_
    set_(old)


@pytest.mark.parametrize("k", range(len(K.ALL)), ids=[c[0] for c in K.ALL])
def test_tails_equal_the_model_and_the_host(all_set, k):
    got = K.check_tails(all_set, k, K.ALL[k], DEV)
    assert got == all_set.score_tails(k, K.probes(K.model(K.ALL[k])), device=HOST)


def test_carries(all_set):
    at = {c[0]: k for k, c in enumerate(K.ALL)}
    assert all_set.score_tails(at["carry_mono_32_equal"], [159, 160, 161], device=DEV) == [2 ** 64, 2 ** 64, 0]
    assert all_set.score_tails(at["carry_mono_63_zero"], [-1, 0, 1], device=DEV) == [2 ** 126, 2 ** 126, 0]
    assert all_set.score_tails(at["carry_di_32_equal"], [-94, -93, -92], device=DEV) == [2 ** 64, 2 ** 64, 0]
    assert all_set.score_tails(at["carry_di_32_zero"], [0, 1], device=DEV) == [2 ** 64, 0]


def test_thresholds_equal_the_model_and_the_host(all_set):
    K.check_thresholds(all_set, K.ALL, DEV)
    for p in K.pvalues(7):
        assert all_set.pvalue_thresholds(p, device=DEV) == all_set.pvalue_thresholds(p, device=HOST), p
    ps = K.pattern_set([K.GOLDEN_ACGT])
    for p, want in [(0.01, 3000), (13 / 256, 2000), (12.999 / 256, 3000), (1 / 256, 3000), (0.5 / 256, 4000),
                    (0.0, 4000), (0.999, 0)]:
        assert ps.pvalue_thresholds(p, device=DEV) == [want], p


def test_random_strands_and_reverse_strands():
    import random

    import pvalue_ref as R
    rnd = random.Random(99)
    cases = [("r%d" % k, "mono", K.rand_mono(rnd, rnd.randint(1, 24), -2000, 2000)) for k in range(6)] + \
            [("rd%d" % k, "di", K.rand_di(rnd, rnd.randint(2, 12), -2000, 2000)) for k in range(4)]
    K.check_thresholds(K.pattern_set(cases), cases, DEV, seed=11)
    for case in [c for c in K.ENUM + K.LONG if c[1] == "mono"][:6] + [c for c in K.ENUM + K.LONG if c[1] == "di"][:6]:
        name, kind, w = case
        rev = (name + "_rev", kind, R.reverse_mono(w) if kind == "mono" else R.reverse_di(w))
        ps = T.PatternSet.from_patterns([K.pattern(case, 0), K.pattern(rev, 0, T.DIR_N)])
        m = K.probes(K.model(case))
        assert ps.score_tails(0, m, device=DEV) == ps.score_tails(1, m, device=DEV) == [K.model(case).tail(v) for v in m]
        th = ps.pvalue_thresholds(0.003, device=DEV)
        assert th[0] == th[1] == K.model(case).threshold(0.003)


def test_loader_on_the_device_equals_the_host(tmp_path):
    import random
    rnd = random.Random(5)
    with open(str(tmp_path / "mono.txt"), "w") as f:
        for k in range(3):
            f.write(">m%d\n" % k)
            for col in K.rand_mono(rnd, 9 + k, -2000, 2000):
                f.write("\t".join("%.3f" % (v / 1000.0) for v in col) + "\n")
    with open(str(tmp_path / "di.txt"), "w") as f:
        f.write(">d0\n")
        for row in K.rand_di(rnd, 7, -2000, 2000):
            f.write("\t".join("%.3f" % (v / 1000.0) for v in row) + "\n")
    names = ["m0", "m2", "d0"]
    kw = dict(dipwm_file=str(tmp_path / "di.txt"), pvalue=0.002)
    dev = T.parse_pwm_files(str(tmp_path / "mono.txt"), None, 0.0, names, device=DEV, **kw).to_list()
    host = T.parse_pwm_files(str(tmp_path / "mono.txt"), None, 0.0, names, device=HOST, **kw).to_list()
    assert dev == host and [(p.name, p.pattern_id) for p in dev] == [("m0", 0)] * 2 + [("m2", 1)] * 2 + [("d0", 2)] * 2


def test_limits_on_the_device():
    ok = K.pattern_set([("wide", "mono", [[0, 0, 0, 2 ** 24 - 1]]), ("wide_di", "di", [[0] * 15 + [2 ** 22 - 1]])])
    assert ok.score_tails(0, [0, 1, 2 ** 24 - 1, 2 ** 24], device=DEV) == [4, 1, 1, 0]
    assert ok.score_tails(1, [0, 1, 2 ** 22 - 1, 2 ** 22], device=DEV) == [16, 1, 1, 0]
    assert ok.pvalue_thresholds(0.2, device=DEV) == [2 ** 24 - 1, 0] == ok.pvalue_thresholds(0.2, device=HOST)
    for bad in (("wider", "mono", [[0, 0, 0, 2 ** 24]]), ("wider_di", "di", [[0] * 15 + [2 ** 22]]),
                ("long", "mono", [[0, 1, 2, 3]] * 64), ("wraps", "mono", [[2 ** 30] * 4] * 2)):
        ps = K.pattern_set([K.GOLDEN_ACGT, bad])
        for call in (lambda: ps.pvalue_thresholds(0.01, device=DEV), lambda: ps.score_tails(1, [0], device=DEV)):
            with pytest.raises(T.TfbsError) as e:
                call()
            assert e.value.code == TFBS_E_ARG and ("'%s'" % bad[0]) in str(e.value)
    ps = T.PatternSet.from_patterns([K.pattern(K.GOLDEN_ACGT, 0), T.Pattern.OtherPattern("o", 1),
                                     T.Pattern.PWM([], "empty", 2, -5)])
    assert ps.pvalue_thresholds(0.01, device=DEV) == [3000, 0, 0]
    assert ps.score_tails(2, [-1, 0, 1], device=DEV) == [1, 1, 0]
    with pytest.raises(T.TfbsError) as e:
        ps.score_tails(1, [0], device=DEV)
    assert e.value.code == TFBS_E_ARG
    for p in (1.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(T.TfbsError) as e:
            ps.pvalue_thresholds(p, device=DEV)
        assert e.value.code == TFBS_E_ARG


def test_chunks_of_mixed_strands_under_three_budgets(scratch_mb):
    """Mono and dinucleotide strands of L = 1, 2, 7, 8, 32, 33, 63 in one call: both parities,
    finished strands beside running ones, under a budget of 0 (a strand per chunk), a small
    fraction (a few per chunk) and the default (one chunk)."""
    import random
    rnd = random.Random(31)
    cases = []
    for L in (63, 1, 2, 7, 8, 32, 33):
        cases.append(("mix_mono_%d" % L, "mono", K.shaped_mono(rnd, L)))
        if 2 <= L <= 32:
            cases.append(("mix_di_%d" % L, "di", K.shaped_di(rnd, L)))
    cases += [("mix_mono_8k", "mono", K.shaped_mono(rnd, 8, scale=1000, mag=4)), ("mix_mono_1b", "mono", [[3, -3, 0, 9]])]
    ps = K.pattern_set(cases)
    want = {p: [K.model(c).threshold(p) for c in cases] for p in (0.0, 1e-4, 0.03, 0.7)}
    for mb in ("0", "0.25", None):
        scratch_mb(mb)
        for p, w in want.items():
            assert ps.pvalue_thresholds(p, device=DEV) == w, (mb, p)
        for k in (0, 1, len(cases) - 2):
            K.check_tails(ps, k, cases[k], DEV)
    scratch_mb(None)
    assert ps.pvalue_thresholds(0.03, device=HOST) == want[0.03]


def test_tile_edges(scratch_mb):
    """Final spans T - 1, T, T + 1 and 2 T + 1 for both tile widths: an L = 2 strand of weights
    {0, 0, 0, S - 1} and a zero column; and strands whose mass sits only in the lowest and the
    highest bin.  The gather and the 128-bit suffix sum cross tiles."""
    cases = []
    for T_ in sorted(set(T.pvalue_tile_widths())):
        for S in (T_ - 1, T_, T_ + 1, 2 * T_ + 1):
            cases.append(("edge_%d" % S, "mono", [[0, 0, 0, S - 1], [0, 0, 0, 0]]))
            cases.append(("edge_di_%d" % S, "di", [[0] * 15 + [S - 1], [0] * 16]))
            cases.append(("ends_%d" % S, "mono", [[0, 0, S - 1, S - 1]] + [[0, 0, 0, 0]] * 31))  # 2^63 + 2^63
    ps = K.pattern_set(cases)
    for mb in ("0", None):
        scratch_mb(mb)
        for k, c in enumerate(cases):
            d = K.model(c)
            assert len(d.scores) == 2 and d.smax - d.smin + 1 == int(c[0].split("_")[-1])
            K.check_tails(ps, k, c, DEV)
        K.check_thresholds(ps, cases, DEV, seed=3)


def _thr_dir(tmp_path, ps):
    """A threshold directory that gives every strand's own min_score back at 0.5."""
    d = tmp_path / "thr"
    d.mkdir()
    for p in ps.to_list():
        f = d / (p.name + ".thr")
        f.write_text("%.3f 1.0\n" % (p.min_score / 1000.0))
        assert T.parse_threshold_file(str(f), 0.5) == p.min_score
    return str(d)


def test_run_flow_and_cli_with_a_pvalue(tmp_path):
    """tfbs_run_ex with pwm_pvalue and no threshold directory writes the text of a run whose
    directory holds pvalue_thresholds' own numbers; the same pair once through the CLI."""
    pwm = os.path.join(TD, "pwm_definitions.txt")
    beds = [os.path.join(TD, "regions1.bed"), os.path.join(TD, "regions2.bed")]
    args = ("chr1", os.path.join(TD, "genotypes2.bcf"), beds, os.path.join(TD, "reference_genome.fa"),
            os.path.join(TD, "samples"), pwm)
    texts = {}
    for n, p in enumerate((0.01, 0.3)):
        ps = T.parse_pwm_files(pwm, None, 0.0, ["ACGT"], pvalue=p, device=DEV)
        assert [q.min_score for q in ps.to_list()] == [3000 if p == 0.01 else 1000] * 2
        sub = tmp_path / ("p%d" % n)
        sub.mkdir()
        thr = _thr_dir(sub, ps)
        a, b = sub / "pvalue.vcf.gz", sub / "dir.vcf.gz"
        T.run(*args, None, 0.0, ["ACGT"], str(a), pwm_pvalue=p)
        T.run(*args, thr, 0.5, ["ACGT"], str(b))
        texts[p] = T.bgzf_read(str(a))
        assert texts[p] == T.bgzf_read(str(b))
        assert texts[p].count("\n") > 1
        if p == 0.01:  # (score > 3000 is score > 3999: the fixture's own threshold)
            assert texts[p] == open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    assert texts[0.01] != texts[0.3] and "COUNTS=4,6" in texts[0.3]
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    out = tmp_path / "cli.vcf.gz"
    r = subprocess.run([exe, "--chromosome", "chr1", "--input", args[1], "--bed", ",".join(beds), "--reference", args[3],
                        "--samples", args[4], "--pwm_file", pwm, "--pwm_pvalue", "0.3", "--pwm_names", "ACGT",
                        "--output", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert T.bgzf_read(str(out)) == texts[0.3]
    r = subprocess.run([exe, "--chromosome", "chr1", "--input", args[1], "--bed", ",".join(beds), "--reference", args[3],
                        "--pwm_file", pwm, "--pwm_pvalue", "1.5", "--pwm_names", "ACGT", "--output", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--pwm_pvalue" in r.stderr
