"""Dinucleotide PWMs (TFBS_KIND_DIPWM) on the host: the ABI round trip, the file
parser, the limits, the plan part and the invariance of a mono set's plan."""
import os
import random

import pytest

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
