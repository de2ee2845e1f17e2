"""The strands the p-value tests run, on the host twin (test_pvalue_cpu.py) and on the device
(test_gpu_pvalue.py), and the checks both share.  The model's table of a case is made once."""
import random

import pvalue_ref as R
from helpers import T


def rand_mono(rnd, L, lo=-32, hi=31, scale=1):
    return [[scale * rnd.randint(lo, hi) for _ in range(4)] for _ in range(L)]


def rand_di(rnd, L, lo=-32, hi=31, scale=1):
    return [[scale * rnd.randint(lo, hi) for _ in range(16)] for _ in range(L - 1)]


def shaped_mono(rnd, L, scale=1, mag=32):
    """Random columns with, in turn, two bases in one bin, an all-negative column, an
    all-positive one and a constant one."""
    cols = rand_mono(rnd, L, -mag, mag - 1, scale)
    for j in range(L):
        if j % 5 == 1:
            cols[j][rnd.randrange(4)] = cols[j][rnd.randrange(4)]
            cols[j][3] = cols[j][0]
        elif j % 5 == 2:
            cols[j] = [-scale * rnd.randint(1, mag) for _ in range(4)]
        elif j % 5 == 3:
            cols[j] = [scale * rnd.randint(1, mag - 1) for _ in range(4)]
        elif j % 11 == 4:
            cols[j] = [scale * 3] * 4
    return cols


def shaped_di(rnd, L, scale=1, mag=32):
    rows = rand_di(rnd, L, -mag, mag - 1, scale)
    for j in range(L - 1):
        if j % 5 == 1:
            rows[j][5] = rows[j][0]
            rows[j][10] = rows[j][15]
        elif j % 5 == 2:
            rows[j] = [-scale * rnd.randint(1, mag) for _ in range(16)]
        elif j % 5 == 3:
            rows[j] = [scale * rnd.randint(1, mag - 1) for _ in range(16)]
    return rows


def _cases():
    rnd = random.Random(20240611)
    enum, long_, carry = [], [], []
    for L in (1, 2, 5, 8):
        enum.append(("enum_mono_%d" % L, "mono", shaped_mono(rnd, L)))
    for L in (2, 3, 6):
        enum.append(("enum_di_%d" % L, "di", shaped_di(rnd, L)))
    for L in (16, 31, 32, 33, 63):
        long_.append(("mono_%d" % L, "mono", shaped_mono(rnd, L)))
    # multiples of 1 000 in [-4 000, 3 000]: mostly empty bins, some 10^5 of them
    long_.append(("mono_32_k", "mono", shaped_mono(rnd, 32, scale=1000, mag=4)))
    long_.append(("mono_63_k", "mono", shaped_mono(rnd, 63, scale=1000, mag=4)))
    for L in (17, 32):
        long_.append(("di_%d" % L, "di", shaped_di(rnd, L)))
    long_.append(("di_17_k", "di", shaped_di(rnd, 17, scale=1000, mag=4)))
    # carries: one bin holding 2^64 (hi = 1, lo = 0), and 2^126.  A dinucleotide strand has
    # at most 32 bases (check_dipwm_length), so 2^64 is the most one of its bins holds.
    carry.append(("carry_mono_32_equal", "mono", [[5, 5, 5, 5]] * 32))
    carry.append(("carry_mono_63_zero", "mono", [[0, 0, 0, 0]] * 63))
    carry.append(("carry_di_32_equal", "di", [[-3] * 16] * 31))
    carry.append(("carry_di_32_zero", "di", [[0] * 16] * 31))
    return enum, long_, carry


ENUM, LONG, CARRY = _cases()
GOLDEN_ACGT = ("golden_acgt", "mono", [[1000, 0, 0, 0], [0, 1000, 0, 0], [0, 0, 1000, 0], [0, 0, 0, 1000]])
ALL = ENUM + LONG + CARRY + [GOLDEN_ACGT]

_MODEL = {}


def model(case):
    """The model's table of a case (enumeration for the ENUM cases), made once."""
    name, kind, w = case
    if name not in _MODEL:
        cnt = R.counts_enum(kind, w) if case in ENUM else R.counts_dp(kind, w)
        _MODEL[name] = R.Dist(cnt, R.length(kind, w))
    return _MODEL[name]


def pattern(case, pid, direction=None, min_score=0):
    name, kind, w = case
    d = T.DIR_P if direction is None else direction
    if kind == "mono":
        return T.Pattern.PWM([T.Weight(*c) for c in w], name, pid, min_score, d)
    return T.Pattern.DiPWM(w, name, pid, min_score, d)


def pattern_set(cases):
    return T.PatternSet.from_patterns([pattern(c, k) for k, c in enumerate(cases)])


def probes(dist):
    """Every integer from smin - 1 to smax + 1, or, over a wide range, every attained score
    and its two neighbours."""
    if dist.smax - dist.smin <= 20000:
        return list(range(dist.smin - 1, dist.smax + 2))
    s = {dist.smin - 1, dist.smax + 1}
    for v in dist.scores:
        s.update((v - 1, v, v + 1))
    return sorted(s)


def pvalues(seed):
    rnd = random.Random(seed)
    ps = [0.0, 0.999, 0.5, 1e-4, 0.01, 2.0 ** -60, 2.0 ** -126, 1.0 - 2.0 ** -53, 5e-324]
    ps += [rnd.random() for _ in range(4)]
    ps += [rnd.random() * 10.0 ** -rnd.randint(1, 30) for _ in range(6)]
    return ps


def check_tails(ps, i, case, device):
    d = model(case)
    m = probes(d)
    got = ps.score_tails(i, m, device=device)
    want = [d.tail(v) for v in m]
    assert got == want, (case[0], device, next((m[k], got[k], want[k]) for k in range(len(m)) if got[k] != want[k]))
    return got


def check_thresholds(ps, cases, device, seed=7):
    for p in pvalues(seed):
        got = ps.pvalue_thresholds(p, device=device)
        want = [model(c).threshold(p) for c in cases]
        assert got == want, (p, device, [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w])
