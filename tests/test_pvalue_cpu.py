"""Thresholds from a p-value on the host twin (device = -1): exact score distributions
against the model of pvalue_ref.py, the threshold rule, the limits, the copy and the
loader."""
import math
import random

import pytest

import pvalue_cases as K
import pvalue_ref as R
from helpers import T

TFBS_E_ARG = -1
TFBS_E_NOPATTERN = -13
HOST = -1


@pytest.fixture(scope="module")
def all_set():
    return K.pattern_set(K.ALL)


def test_model_dp_equals_enumeration():
    for name, kind, w in K.ENUM:
        assert R.counts_dp(kind, w) == R.counts_enum(kind, w), name


@pytest.mark.parametrize("k", range(len(K.ALL)), ids=[c[0] for c in K.ALL])
def test_tails_equal_the_model(all_set, k):
    K.check_tails(all_set, k, K.ALL[k], HOST)


def test_carries(all_set):
    at = {c[0]: k for k, c in enumerate(K.ALL)}
    assert all_set.score_tails(at["carry_mono_32_equal"], [159, 160, 161], device=HOST) == [2 ** 64, 2 ** 64, 0]
    assert all_set.score_tails(at["carry_mono_63_zero"], [-1, 0, 1], device=HOST) == [2 ** 126, 2 ** 126, 0]
    assert all_set.score_tails(at["carry_di_32_equal"], [-94, -93, -92], device=HOST) == [2 ** 64, 2 ** 64, 0]
    assert all_set.score_tails(at["carry_di_32_zero"], [0, 1], device=HOST) == [2 ** 64, 0]
    # the halves as the C ABI hands them out: hi = 1, lo = 0
    import ctypes as C
    lo, hi = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    T.check(T.lib().tfbs_patterns_score_tails(all_set.h, HOST, at["carry_mono_32_equal"], (C.c_int32 * 1)(160), 1, lo, hi))
    assert (hi[0], lo[0]) == (1, 0)


@pytest.mark.parametrize("kind", ["mono", "di"])
def test_reverse_strand_has_the_forward_table(kind):
    for case in [c for c in K.ENUM + K.LONG if c[1] == kind][:6]:
        name, _, w = case
        rev = (name + "_rev", kind, R.reverse_mono(w) if kind == "mono" else R.reverse_di(w))
        ps = T.PatternSet.from_patterns([K.pattern(case, 0), K.pattern(rev, 0, T.DIR_N)])
        m = K.probes(K.model(case))
        fwd = ps.score_tails(0, m, device=HOST)
        assert fwd == ps.score_tails(1, m, device=HOST) == [K.model(case).tail(v) for v in m], name
        th = ps.pvalue_thresholds(0.003, device=HOST)
        assert th[0] == th[1]


GOLDEN_RULE = [(0.01, 3000), (13 / 256, 2000), (12.999 / 256, 3000), (1 / 256, 3000), (0.5 / 256, 4000), (0.0, 4000),
               (0.999, 0)]


def test_threshold_rule_on_the_golden_pwm():
    ps = K.pattern_set([K.GOLDEN_ACGT])
    assert ps.score_tails(0, [0, 1000, 2000, 3000, 4000, 4001], device=HOST) == [256, 175, 67, 13, 1, 0]
    for p, want in GOLDEN_RULE:
        assert ps.pvalue_thresholds(p, device=HOST) == [want], p
        assert K.model(K.GOLDEN_ACGT).threshold(p) == want, p


def test_thresholds_at_random_p_equal_the_model(all_set):
    K.check_thresholds(all_set, K.ALL, HOST)
    rnd = random.Random(99)
    cases = [("r%d" % k, "mono", K.rand_mono(rnd, rnd.randint(1, 24), -2000, 2000)) for k in range(6)] + \
            [("rd%d" % k, "di", K.rand_di(rnd, rnd.randint(2, 12), -2000, 2000)) for k in range(4)]
    K.check_thresholds(K.pattern_set(cases), cases, HOST, seed=11)


def test_other_strand_keeps_its_min_score():
    ps = T.PatternSet.from_patterns([K.pattern(K.GOLDEN_ACGT, 0, min_score=77), T.Pattern.OtherPattern("o", 1),
                                     K.pattern(K.ENUM[4], 2)])
    th = ps.pvalue_thresholds(0.01, device=HOST)
    assert th == [3000, 0, K.model(K.ENUM[4]).threshold(0.01)]
    with pytest.raises(T.TfbsError) as e:
        ps.score_tails(1, [0], device=HOST)
    assert e.value.code == TFBS_E_ARG and "'o'" in str(e.value)


def _refused(ps, name):
    with pytest.raises(T.TfbsError) as e:
        ps.pvalue_thresholds(0.01, device=HOST)
    assert e.value.code == TFBS_E_ARG and ("'%s'" % name) in str(e.value), str(e.value)
    with pytest.raises(T.TfbsError) as e:
        ps.score_tails(len(ps) - 1, [0], device=HOST)
    assert e.value.code == TFBS_E_ARG and ("'%s'" % name) in str(e.value), str(e.value)


def test_limits_span():
    ok = K.pattern_set([("wide", "mono", [[0, 0, 0, 2 ** 24 - 1]])])
    assert ok.score_tails(0, [0, 1, 2 ** 24 - 1, 2 ** 24], device=HOST) == [4, 1, 1, 0]
    assert ok.pvalue_thresholds(0.25, device=HOST) == [0] and ok.pvalue_thresholds(0.2, device=HOST) == [2 ** 24 - 1]
    _refused(K.pattern_set([K.GOLDEN_ACGT, ("wider", "mono", [[0, 0, 0, 2 ** 24]])]), "wider")
    row = [0] * 15 + [2 ** 22 - 1]
    okd = K.pattern_set([("wide_di", "di", [row])])
    assert okd.score_tails(0, [0, 1, 2 ** 22 - 1, 2 ** 22], device=HOST) == [16, 1, 1, 0]
    _refused(K.pattern_set([("wider_di", "di", [[0] * 15 + [2 ** 22]])]), "wider_di")
    # the bound is the columns' extremes summed, as the tables are sized
    _refused(K.pattern_set([("two", "mono", [[0, 0, 0, 2 ** 23], [0, 0, 0, 2 ** 23]])]), "two")


def test_limits_length_wrap_and_p():
    _refused(K.pattern_set([("long", "mono", [[0, 1, 2, 3]] * 64)]), "long")
    big = 2 ** 30
    _refused(K.pattern_set([("wraps", "mono", [[big, big, big, big - 1]] * 2)]), "wraps")
    _refused(K.pattern_set([("wraps_neg", "mono", [[-big, -big, -big, -big + 1]] * 2)]), "wraps_neg")
    # the largest sum that cannot wrap passes
    edge = K.pattern_set([("edge", "mono", [[big, big, big, big - 1], [big - 1, big - 1, big - 1, big - 2]])])
    assert edge.score_tails(0, [2 * big - 1], device=HOST) == [9]
    ps = K.pattern_set([K.GOLDEN_ACGT])
    for p in (1.0, -0.1, float("nan"), float("inf"), -float("inf"), 1.5):
        with pytest.raises(T.TfbsError) as e:
            ps.pvalue_thresholds(p, device=HOST)
        assert e.value.code == TFBS_E_ARG, p
    assert ps.pvalue_thresholds(math.nextafter(1.0, 0.0), device=HOST) == [0]


def test_empty_strand():
    ps = T.PatternSet.from_patterns([T.Pattern.PWM([], "empty", 0, -5)])
    assert ps.score_tails(0, [-1, 0, 1], device=HOST) == [1, 1, 0]
    assert ps.pvalue_thresholds(0.5, device=HOST) == [0]


def test_with_min_scores_keeps_everything_else(all_set):
    base = all_set.to_list()
    ms = [1000 * k - 7 for k in range(len(base))]
    copy = all_set.with_min_scores(ms)
    got = copy.to_list()
    assert [p.min_score for p in got] == ms
    assert [p.min_score for p in all_set.to_list()] == [p.min_score for p in base]  # the original is untouched
    for a, b in zip(base, got):
        assert (a.name, a.pattern_id, a.weights, a.direction, a.kind) == (b.name, b.pattern_id, b.weights, b.direction,
                                                                          b.kind)
    assert [copy.name_of(p.pattern_id) for p in got] == [all_set.name_of(p.pattern_id) for p in base]
    assert copy.max_length == all_set.max_length
    with pytest.raises(ValueError):
        all_set.with_min_scores(ms[:-1])


def _write_defs(path, defs, fmt):
    with open(path, "w") as f:
        for name, rows in defs:
            f.write(">%s\n" % name)
            for r in rows:
                f.write("\t".join(fmt % (v / 1000.0) for v in r) + "\n")


def test_loader_gives_the_di_loaders_ids_without_a_directory(tmp_path):
    rnd = random.Random(5)
    mono = [("m%d" % k, K.rand_mono(rnd, 6 + k, -2000, 2000)) for k in range(4)]
    di = [("d%d" % k, K.rand_di(rnd, 4 + k, -2000, 2000)) for k in range(3)]
    _write_defs(tmp_path / "mono.txt", mono, "%.3f")
    _write_defs(tmp_path / "di.txt", di, "%.3f")
    names = ["m0", "m2", "missing", "d1", "d2", "m3"]
    thr = tmp_path / "thr"
    thr.mkdir()
    for n in names:
        (thr / (n + ".thr")).write_text("1.0 0.5\n")
    want = T.parse_pwm_files(str(tmp_path / "mono.txt"), str(thr), 0.1, names, True, dipwm_file=str(tmp_path / "di.txt"))
    got = T.parse_pwm_files(str(tmp_path / "mono.txt"), None, 0.0, names, True, dipwm_file=str(tmp_path / "di.txt"),
                            pvalue=0.004, device=HOST)
    a, b = want.to_list(), got.to_list()
    assert len(a) == len(b) == 10
    for x, y in zip(a, b):
        assert (x.name, x.pattern_id, x.weights, x.direction, x.kind) == (y.name, y.pattern_id, y.weights, y.direction,
                                                                          y.kind)
    assert [p.min_score for p in b] == want.pvalue_thresholds(0.004, device=HOST)
    cases = [(p.name, "mono" if p.kind == T.KIND_PWM else "di",
              [w.acgtn[:4] for w in p.weights] if p.kind == T.KIND_PWM else p.weights) for p in b]
    assert [p.min_score for p in b] == [R.Dist(R.counts_dp(k, w), R.length(k, w)).threshold(0.004) for _, k, w in cases]
    # forward only, one file, nothing named, a refused definition
    fwd = T.parse_pwm_files(None, None, 0.0, ["d0"], False, dipwm_file=str(tmp_path / "di.txt"), pvalue=0.5, device=HOST)
    assert [(p.name, p.pattern_id, p.direction) for p in fwd.to_list()] == [("d0", 0, T.DIR_P)]
    with pytest.raises(T.TfbsError) as e:
        T.parse_pwm_files(str(tmp_path / "mono.txt"), None, 0.0, ["nobody"], pvalue=0.5, device=HOST)
    assert e.value.code == TFBS_E_NOPATTERN
    _write_defs(tmp_path / "long.txt", [("ok", K.rand_mono(rnd, 5)), ("toolong", K.rand_mono(rnd, 64))], "%.3f")
    with pytest.raises(T.TfbsError) as e:
        T.parse_pwm_files(str(tmp_path / "long.txt"), None, 0.0, ["ok", "toolong"], pvalue=0.5, device=HOST)
    assert e.value.code == TFBS_E_ARG and "'toolong'" in str(e.value)
    with pytest.raises(T.TfbsError) as e:
        T.parse_pwm_files(str(tmp_path / "mono.txt"), None, 0.0, ["m0"], pvalue=1.0, device=HOST)
    assert e.value.code == TFBS_E_ARG


def test_run_ext_layouts():
    import ctypes as C
    from find_tfbs_amd import _capi
    assert C.sizeof(_capi.tfbs_run_ext_pvalue) == C.sizeof(_capi.tfbs_run_ext_scores) + 8
    assert _capi.tfbs_run_ext_pvalue.pwm_pvalue.offset == C.sizeof(_capi.tfbs_run_ext_scores)
    assert all(w > 0 for w in T.pvalue_tile_widths())
