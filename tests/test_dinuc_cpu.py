"""Dinucleotide PWMs (TFBS_KIND_DIPWM) on the host: the ABI round trip, the file
parser, the limits, the plan part, the invariance of a mono set's plan, the plan's lookup
tables against the reference, and the reference-only conditions of the GPU count cases."""
import os
import random

import pytest

import dinuc_cases as K
import dinuc_ref as D
from helpers import T, synth_patterns

TFBS_E_ARG = -1


def rand_rows(rnd, L, lo=-2000, hi=2000):
    return [[rnd.randint(lo, hi) for _ in range(16)] for _ in range(L - 1)]


def write_di_file(path, defs, extra=None):
    """defs: [(name, rows of 16 floats given as strings)]; extra: {name: lines put
    between its rows (malformed rows)}."""
    with open(path, "w") as f:
        for name, rows in defs:
            f.write(">%s\n" % name)
            for k, r in enumerate(rows):
                f.write("\t".join(r) + "\n")
                if extra and name in extra and k == 0:
                    for line in extra[name]:
                        f.write(line + "\n")


def write_thr(dirname, name, lines):
    with open(os.path.join(dirname, name + ".thr"), "w") as f:
        for score, pv in lines:
            f.write("%s %s\n" % (score, pv))


def fmt_rows(rnd, R):
    return [["%.3f" % rnd.uniform(-2, 2) for _ in range(16)] for _ in range(R)]


def test_create_get_round_trip_and_max_length():
    rnd = random.Random(1)
    rows = rand_rows(rnd, 7)
    pats = [T.Pattern.DiPWM(rows, "di", 3, 1234, T.DIR_P),
            T.Pattern.DiPWM(D.reverse_rows(rows), "di", 3, 1234, T.DIR_N),
            T.Pattern.PWM([T.Weight(1, 2, 3, 4)] * 5, "mono", 0, 7)]
    assert len(pats[0]) == 7 and len(pats[0].weights) == 6
    ps = T.PatternSet.from_patterns(pats)
    got = ps.to_list()
    assert got == pats
    assert got[0].kind == T.KIND_DIPWM == 2 and len(got[0]) == 7
    assert ps.max_length == 7  # bases, not rows: above the mono PWM's 5
    assert ps.name_of(3) == "di"
    assert T.PatternSet.from_patterns([T.Pattern.DiPWM(rand_rows(rnd, 2), "x", 0, 0)]).max_length == 2


def test_parser_two_definitions_ids_and_reverse(tmp_path):
    rnd = random.Random(2)
    d = str(tmp_path)
    defs = [("DIA", fmt_rows(rnd, 4)), ("SKIP", fmt_rows(rnd, 3)), ("DIB", fmt_rows(rnd, 9))]
    # a row of 15 fields and one of 4 are skipped, as the mono parser skips rows whose count is not 4
    extra = {"DIA": ["\t".join(["0.5"] * 15), "1 2 3 4"]}
    write_di_file(os.path.join(d, "di.txt"), defs, extra)
    for name in ("DIA", "DIB"):
        write_thr(d, name, [("9.5", "0.5"), ("3.25", "0.01"), ("1.0", "0.00001")])
    # SKIP is asked for but no line of its threshold file qualifies: it is not loaded and,
    # as in the mono parser (pattern.rs:66-81), still takes a pattern id
    write_thr(d, "SKIP", [("1.0", "0.00001")])
    ps = T.parse_pwm_files(None, d, 0.001, ["DIA", "SKIP", "DIB"], True, dipwm_file=os.path.join(d, "di.txt"))
    pl = ps.to_list()
    assert [(p.name, p.pattern_id, p.direction, p.kind) for p in pl] == [
        ("DIA", 0, T.DIR_P, 2), ("DIA", 0, T.DIR_N, 2), ("DIB", 2, T.DIR_P, 2), ("DIB", 2, T.DIR_N, 2)]
    assert [len(p) for p in pl] == [5, 5, 10, 10]
    assert all(p.min_score == 3250 for p in pl)  # the last line with p-value > 0.001
    for (name, rows), p in zip([defs[0], defs[2]], [pl[0], pl[2]]):
        assert p.weights == [[T.parse_weight(x) for x in r] for r in rows]
    assert pl[1].weights == D.reverse_rows(pl[0].weights)
    assert pl[3].weights == D.reverse_rows(pl[2].weights)
    fwd = T.parse_pwm_files(None, d, 0.001, ["DIB"], False, dipwm_file=os.path.join(d, "di.txt")).to_list()
    assert [(p.pattern_id, p.direction) for p in fwd] == [(0, T.DIR_P)]  # definitions not asked for take no id
    with pytest.raises(T.TfbsError):  # nothing selected
        T.parse_pwm_files(None, d, 0.001, ["NOPE"], True, dipwm_file=os.path.join(d, "di.txt"))


def test_parser_ids_continue_after_the_mono_file(tmp_path):
    rnd = random.Random(3)
    mono, names = synth_patterns(tmp_path, 5, 2, 4)
    d = str(tmp_path)
    write_di_file(os.path.join(d, "di.txt"), [("DIX", fmt_rows(rnd, 3)), ("DIY", fmt_rows(rnd, 5))])
    for name in ("DIX", "DIY"):
        write_thr(os.path.join(d, "thr"), name, [("2.0", "0.5")])
    wanted = [names[1], names[3], "DIY"]
    both = T.parse_pwm_files(os.path.join(d, "pwms.txt"), os.path.join(d, "thr"), 1e-4, wanted, True,
                             dipwm_file=os.path.join(d, "di.txt"))
    only = T.parse_pwm_files(os.path.join(d, "pwms.txt"), os.path.join(d, "thr"), 1e-4, wanted[:2], True)
    bl, ol = both.to_list(), only.to_list()
    assert bl[:len(ol)] == ol  # the mono file's patterns exactly as without the dinucleotide file
    assert [p.pattern_id for p in ol] == [0, 0, 1, 1]
    assert [(p.name, p.pattern_id, p.kind) for p in bl[len(ol):]] == [("DIY", 2, 2), ("DIY", 2, 2)]
    assert both.max_length == max(only.max_length, 6)


def test_limits_return_e_arg():
    rnd = random.Random(4)
    ok = T.PatternSet.from_patterns([T.Pattern.DiPWM(rand_rows(rnd, 32), "max", 0, 0)])
    assert ok.max_length == 32
    for bad in ([T.Pattern.DiPWM(rand_rows(rnd, 33), "long", 0, 0)],
                [T.Pattern.DiPWM([], "short", 0, 0)],
                [T.Pattern.DiPWM(rand_rows(rnd, 5), "a", 4, 0), T.Pattern.PWM([T.Weight(1, 2, 3, 4)] * 5, "b", 4, 0)]):
        with pytest.raises(T.TfbsError) as e:
            T.PatternSet.from_patterns(bad)
        assert e.value.code == TFBS_E_ARG
        assert "dinucleotide" in str(e.value)


def test_limits_in_the_parser(tmp_path):
    rnd = random.Random(5)
    d = str(tmp_path)
    write_di_file(os.path.join(d, "di.txt"), [("LONG", fmt_rows(rnd, 32)), ("EMPTY", [])])
    for name in ("LONG", "EMPTY"):
        write_thr(d, name, [("2.0", "0.5")])
    for name in ("LONG", "EMPTY"):
        with pytest.raises(T.TfbsError) as e:
            T.parse_pwm_files(None, d, 0.001, [name], True, dipwm_file=os.path.join(d, "di.txt"))
        assert e.value.code == TFBS_E_ARG


def test_dinuc_stats_counts_strands_and_tiles():
    rnd = random.Random(6)
    assert T.PatternSet.from_patterns([T.Pattern.PWM([T.Weight(1, 2, 3, 4)] * 5, "m", 0, 0)]).dinuc_stats() == {
        "n_strands": 0, "n_tiles": 0, "lut_bytes": 0}
    pats = []
    for pid in range(40):  # 80 strands of 32 bases: more lookup tables than one tile's LDS holds
        rows = rand_rows(rnd, 32)
        pats += [T.Pattern.DiPWM(rows, "d%d" % pid, pid, 0, T.DIR_P),
                 T.Pattern.DiPWM(D.reverse_rows(rows), "d%d" % pid, pid, 0, T.DIR_N)]
    st = T.PatternSet.from_patterns(pats).dinuc_stats()
    assert st["n_strands"] == 80
    assert st["n_tiles"] >= 2
    assert st["lut_bytes"] > 0 and st["lut_bytes"] % 16 == 0
    st1 = T.PatternSet.from_patterns(pats[:2]).dinuc_stats()
    assert st1["n_strands"] == 2 and st1["n_tiles"] == 1


@pytest.mark.parametrize("n_pwms,config,seed", [(10, 2, 2), (600, 3, 3)])
def test_mono_plan_is_invariant_under_an_appended_dipwm(tmp_path, n_pwms, config, seed):
    """The C2 / C3 synthetic mono sets: the plan statistics, the patterns and the count
    slots of the existing patterns are the same with an unrelated dinucleotide PWM
    appended to the set."""
    mono, _ = synth_patterns(tmp_path, n_pwms, config, seed)
    ml = mono.to_list()
    rnd = random.Random(7)
    rows = rand_rows(rnd, 11)
    pid = max(p.pattern_id for p in ml) + 1
    plus = T.PatternSet.from_patterns(ml + [T.Pattern.DiPWM(rows, "di", pid, 100, T.DIR_P),
                                            T.Pattern.DiPWM(D.reverse_rows(rows), "di", pid, 100, T.DIR_N)])
    for mfma in (False, True):
        assert plus.plan_stats(mfma=mfma) == mono.plan_stats(mfma=mfma)
    assert plus.to_list()[:len(ml)] == ml
    assert plus.dinuc_stats()["n_strands"] == 2 and mono.dinuc_stats()["n_strands"] == 0


# ---------------------------------------------------------------------------------------
# The plan's lookup tables, evaluated on the host the way the kernel's lookup loop reads
# them (PatternSet.dinuc_lut_scores), against dinuc_ref.py.  Nothing here knows k.
# ---------------------------------------------------------------------------------------
def check_lut(pats, rnd, n_images):
    """Every strand of the set on n_images random windows, each scored twice with different
    bases after its L-th: both equal the reference's score of the window."""
    ps = T.PatternSet.from_patterns(pats)
    wrapped = 0
    for i, p in enumerate(pats):
        L = len(p)
        wins = [[rnd.randrange(4) for _ in range(L)] for _ in range(n_images)]
        a = [w + [rnd.randrange(4) for _ in range(32 - L)] for w in wins]
        b = [w + [3 - c for c in x[L:]] for w, x in zip(wins, a)]  # every base past L differs
        want = [D.score(p.weights, w, 0) for w in wins]
        ga, gb = ps.dinuc_lut_scores(i, a), ps.dinuc_lut_scores(i, b)
        assert ga == want, (i, L, p.pattern_id)
        assert gb == want, (i, L, p.pattern_id)
        wrapped += sum(1 for w in wins if not K.INT32_MIN <= K.exact_sum(p.weights, w, 0) <= K.INT32_MAX)
    return ps, wrapped


def test_lut_scores_every_length():
    """Base lengths 2..32, both strands, in one set (neighbouring lengths share units) and
    each length alone (a unit padded to two strands)."""
    rnd = random.Random(11)
    pats = []
    for L in range(2, 33):
        rows = rand_rows(rnd, L)
        pats += [T.Pattern.DiPWM(rows, "d%d" % L, L, 0, T.DIR_P),
                 T.Pattern.DiPWM(D.reverse_rows(rows), "d%d" % L, L, 0, T.DIR_N)]
    check_lut(pats, rnd, 100)
    for L in range(2, 33):
        check_lut(pats[2 * (L - 2):2 * (L - 2) + 2], rnd, 10)


def test_lut_scores_units_of_mixed_lengths_and_padded_units():
    """Strands of one pattern_id with lengths (3, 32), (2, 17, 31) and (4, 4, 7, 31, 32): a
    short strand's blocks past its length read 0 beside a long one's; sets of 1, 2, 3, 5 and
    6 strands: units padded to 1, 2 or 3 real strands.  (With the five strands cut into units
    in creation order, 4 4 7 31 | 32, the k = 5 build refused the set: two units of full depth
    are more than its tile holds.  The planner now packs a pattern_id's strands longest first.)"""
    rnd = random.Random(12)
    calib = [rnd.randrange(4) for _ in range(100)]
    pats = []
    for pid, lengths in enumerate(((3, 32), (2, 17, 31), (4, 4, 7, 31, 32))):
        pats += K.strands(rnd, pid, lengths, calib)
    ps, _ = check_lut(pats, rnd, 60)
    assert ps.dinuc_stats()["n_strands"] == 10
    five, rest = pats[5:], sorted(pats[5:], key=len, reverse=True)
    lut_bytes = lambda ps_: T.PatternSet.from_patterns(ps_).dinuc_stats()["lut_bytes"]
    assert [len(p) for p in five] == [4, 4, 7, 31, 32]
    assert lut_bytes(five) == lut_bytes(rest[:4]) + lut_bytes(rest[4:])  # packed as 32 31 7 4 | 4
    lens = (9, 2, 32, 5, 17, 3)
    for total in (1, 2, 3, 5, 6):
        some = [T.Pattern.DiPWM(rand_rows(rnd, lens[k]), "s%d" % k, k // 2, 0, k & 1) for k in range(total)]
        check_lut(some, rnd, 40)


def test_lut_scores_across_tiles_and_the_slot_cap():
    """70 ids of 2-3 bases (one and two strands) beside 9 two-strand ids of 32: more than the
    64 slots of a tile."""
    rnd = random.Random(13)
    calib = [rnd.randrange(4) for _ in range(100)]
    pats = []
    for k in range(70):
        pats += K.strands(rnd, 100 + k, [(2,), (3, 2), (3,), (2, 2)][k % 4], calib)
    for k in range(9):
        pats += K.both_strands(rnd, k, 32, calib)
    ps, _ = check_lut(pats, rnd, 30)
    assert ps.dinuc_stats()["n_tiles"] >= 2


def test_lut_scores_wrap():
    """Weights of +-2^30, +-(2^31 - 1) and -2^31 among small ones: the tables' partial sums
    and the sum over blocks wrap as the specification's int32 sum does."""
    rnd = random.Random(14)
    pats = [T.Pattern.DiPWM(K.wrap_rows(rnd, L), "w%d" % k, k, 0) for k, L in enumerate((2, 3, 4, 5, 6, 9, 13, 17, 32))]
    _, wrapped = check_lut(pats, rnd, 100)
    assert wrapped >= 100  # windows whose exact sum lies outside int32


def test_lut_scores_argument_errors():
    rnd = random.Random(15)
    ps = T.PatternSet.from_patterns([T.Pattern.PWM([T.Weight(1, 2, 3, 4)] * 5, "m", 0, 0),
                                     T.Pattern.DiPWM(rand_rows(rnd, 4), "d", 1, 0)])
    assert len(ps.dinuc_lut_scores(1, [[0] * 32])) == 1 and ps.dinuc_lut_scores(1, []) == []
    for i, img in ((0, [0] * 32), (2, [0] * 32), (1, [0] * 31 + [4])):
        with pytest.raises(T.TfbsError) as e:
            ps.dinuc_lut_scores(i, [img])
        assert e.value.code == TFBS_E_ARG


# ---------------------------------------------------------------------------------------
# The cases of test_gpu_dinuc_counts.py (dinuc_cases.py): what makes them bite, checked on
# the reference alone.
# ---------------------------------------------------------------------------------------
def attains_thresholds(case):
    """Every threshold but INT32_MIN / INT32_MAX is a score of a window of the first region's
    reference haplotype (the calibration sequence): equality is scanned, and is no hit."""
    return all(p.min_score in D.scores(p.weights, case["calib"]) for p in case["pats"]
               if K.INT32_MIN < p.min_score < K.INT32_MAX)


def test_cases_every_pattern_id_counts():
    for case in (K.case_tiles(), K.case_geometry(), K.case_many_haplotypes(), K.case_n_and_indels(),
                 K.case_reduction(), K.case_all_kernels()):
        assert K.ids_with_a_key(case["want"]) == {p.pattern_id for p in case["pats"]}
        assert K.total_hits(case["want"]) >= 100
        assert attains_thresholds(case)
    # the wrap case: an id whose threshold is INT32_MAX can have no key; every other id has one
    case = K.case_wrap()
    never = {p.pattern_id for p in case["pats"] if p.min_score == K.INT32_MAX}
    assert len(never) == 5
    assert K.ids_with_a_key(case["want"]) == {p.pattern_id for p in case["pats"]} - never
    assert K.total_hits(case["want"]) >= 100
    for p in case["pats"]:  # attained, or (the fourth threshold of each strand) an attained score minus 1
        if K.INT32_MIN < p.min_score < K.INT32_MAX:
            sc = D.scores(p.weights, case["calib"])
            assert p.min_score in sc or p.min_score + 1 in sc


def test_case_tiles_plan():
    case = K.case_tiles()
    ps = T.PatternSet.from_patterns(case["pats"])
    assert ps.dinuc_stats()["n_tiles"] >= 3 and ps.dinuc_stats()["n_strands"] == 122
    assert all(len(T.select_inner_peaks(r["merged"], case["beds"])) == 3 for r in case["regions"])


def test_case_geometry_shapes():
    case = K.case_geometry()
    assert tuple(len(r["ref"]) - 2 + 1 for r in case["regions"]) == K.GEOMETRY_WINDOWS
    assert all(len(set(sq)) >= 3 for sq in case["seqs"])  # several distinct haplotypes in every region
    assert sum(len(set(sq)) for sq in case["seqs"]) > 128
    assert len(set(K.case_many_haplotypes()["seqs"][0])) > 128


def test_case_n_and_indels_conditions():
    case = K.case_n_and_indels()
    st = case["stats"]
    assert st["with_n"] >= 5 and st["after_indel"] >= 5
    assert st["n_first"] >= 5 and st["n_last"] >= 5  # N as a hit window's first and as its last base
    assert st["n_in_indel_haplotype"] >= 5  # N and positions in one haplotype
    refs = [r["ref"] for r in case["regions"]]
    assert refs[0][0] == "N" and refs[0][-1] == "N" and "NNN" in refs[0]
    r1 = case["regions"][1]
    assert any(len(ref) == 6 and len(alt) == 1 and pos + 5 == r1["ee"] for _, pos, ref, alt, _ in r1["records"])
    kinds = {(len(ref), len(alt)) for r in case["regions"] for _, _, ref, alt, _ in r["records"]}
    assert kinds == {(1, 1), (1, 4), (6, 1)}  # SNVs, insertions of 3, deletions of 5


def test_case_reduction_shapes_and_row_reconstruction():
    """Region 0 has 40 inner ranges (more than 32), region 1's doubled range doubles its counts;
    rebuild_rows reproduces the oracle's own rows from the oracle's keys on the mono set."""
    case = K.case_reduction()
    inner = [T.select_inner_peaks(r["merged"], case["beds"]) for r in case["regions"]]
    assert len(inner[0]) == 41 and len({i[1] for i in inner[0]}) == 1
    assert len(inner[1]) == 3 and inner[1][0] == inner[1][1]
    s1, e1 = case["regions"][1]["merged"]
    once = K.expected_keys(case["pats"], case["n"], [("a.bed", [(s1, e1)])], case["regions"][1], case["seqs"][1])
    assert once and all(case["want"][1][k] == ([2 * x for x in l], [2 * x for x in r]) for k, (l, r) in once.items())
    names = {p.pattern_id: p.name for p in case["mono"]}
    assert case["mono_rows"].count("\n") >= 10
    assert K.rebuild_rows(case["mono_keys"], case["beds"], names.get) == case["mono_rows"]
    f = K.case_all_kernels()
    names = {p.pattern_id: p.name for p in f["mono"]}
    assert K.rebuild_rows(f["mono_keys"], f["beds"], names.get) == f["mono_rows"]


def test_case_wrap_really_wraps():
    case = K.case_wrap()
    outside = hit_min = equal = 0
    for codes, _ in set(case["seqs"][0]):
        for p in case["pats"]:
            for i, v in enumerate(D.scores(p.weights, codes)):
                outside += not K.INT32_MIN <= K.exact_sum(p.weights, codes, i) <= K.INT32_MAX
                hit_min += p.min_score == K.INT32_MIN and v == K.INT32_MIN  # the one score INT32_MIN rejects
                equal += v == p.min_score
    assert outside >= 100 and hit_min >= 1 and equal >= 10
    assert {p.min_score for p in case["pats"]} >= {K.INT32_MIN, K.INT32_MAX}
    assert len(case["pats"]) % 4 == 1  # the last unit holds one real strand and three padding strands


def test_case_all_kernels_plan():
    f = K.case_all_kernels()
    mixed = T.PatternSet.from_patterns(sorted(f["mono"] + f["pats"], key=lambda p: p.pattern_id))
    st = mixed.plan_stats(mfma=True)
    assert st["n_mfma_strands"] > 0 and st["n_quad_strands"] > 0 and st["n_generic_strands"] > 0
    assert mixed.plan_stats(mfma=False)["n_octet_strands"] > 0 and mixed.dinuc_stats()["n_strands"] == 14
    di, mono = {p.pattern_id for p in f["pats"]}, {p.pattern_id for p in f["mono"]}
    assert min(di) < min(mono) and any(min(mono) < d < max(mono) for d in di) and max(di) > max(mono)
    assert sum(sum(l) + sum(r) for k in f["mono_keys"] for l, r in k.values()) >= 100
    assert {k[2] for ks in f["mono_keys"] for k in ks} == mono
