"""Inputs on the edges of the matrix-core filter (mfma.cpp, scan_mfma.hip), shared by
test_filter_cases_cpu.py (which proves, from the decoded plan and the oracle, that every
case sits on the edge it claims) and test_gpu_filter.py (which runs them).

A case is a pattern set, the image budget it is planned with, haplotypes ("ACGTN" strings)
and `marks`: the places the CPU test looks at.  Where a family depends on the common
threshold T0 the plan chooses for its super tile, it is built for the T0 read back from
the plan and rebuilt until the two agree (fixed_point).

Strands are laid out by the plan in ascending (length, pattern id) order, 64 per tile, so
with one pattern id per strand and one length per family the id order is the place order.

With scale 8 (D = C - min_score = |T0|) the digit of a weight w' = -m, m on the FP6 grid,
is m itself: U = score - C exactly, "U > T0" is "score > min_score", and a window can be
put on the threshold to the unit."""
import functools
import random

from helpers import T
import filter_ref as F

GRID = sorted(set(F.GRID8))


def decompose(m):
    """m as a sum of grid magnitudes, largest first."""
    out = []
    while m:
        g = max(x for x in GRID if x <= m)
        out.append(g)
        m -= g
    return out


class Case:
    def __init__(self, name, patterns, haps, lds_kb=0, marks=None):
        self.name, self.patterns, self.haps, self.lds_kb = name, patterns, haps, lds_kb
        self.marks = marks or {}
        self.pset = T.PatternSet.from_patterns(patterns)

    @functools.cached_property
    def plan(self):
        return F.FilterPlan(self.pset.mfma_plan(self.lds_kb))

    def with_budget(self, lds_kb):
        return Case("%s@%dk" % (self.name, lds_kb), self.patterns, self.haps, lds_kb, self.marks)


def pwm(rows, pid, min_score):
    return T.Pattern.PWM([T.Weight(*r) for r in rows], "P%d" % pid, pid, min_score)


def fixed_point(build):
    """build(t0) -> Case whose marks["super"] names the super tile the family lives in;
    rebuilt until that super tile's t0 is the t0 the family was built for."""
    t0 = -32
    for _ in range(12):
        case = build(t0)
        got = case.plan.supers[case.marks.get("super", 0)]["t0"]
        if got == t0:
            return case
        t0 = got
    raise AssertionError("no threshold the plan keeps for %s" % case.name)


# ---------------------------------------------------------------------------
# field neighbours
# ---------------------------------------------------------------------------
NB_LEN = 26


def _neighbours(t0):
    """26-column strands of scale 8 under t0 (min_score = t0, C = 0): "min" reaches U = t0 - 1023
    (V = 0) on the windows W1 (all T) and W2 (a G at column ke), "edge" U = t0 + 1 on W1 (a hit)
    and U = t0 on W2 (a tie), "zero" U = 0 on both, "clip" has 26 columns of 60."""
    a = -t0
    zero = [0, 0, 0, 0]
    ms = decompose(F.FIELD_BIAS + a)        # the minimum strand: W1 and W2 reach T0 - 1023
    es = decompose(a - 1)                   # the edge strand: W1 at T0 + 1, W2 (G at column ke) at T0
    ke = len(es)
    assert len(ms) <= NB_LEN and ke < NB_LEN

    def rows(digits, g_extra=None):
        r = [[0, 0, -m, -m] for m in digits] + [list(zero) for _ in range(NB_LEN - len(digits))]
        if g_extra is not None:
            r[g_extra] = [0, 0, -1, 0]
        return r
    m_rows, e_rows = rows(ms), rows(es, ke)
    z_rows = [[-5, -5, 0, 0] for _ in range(NB_LEN)]
    k_rows = [[0, 0, -60, -60] for _ in range(NB_LEN)]   # 26 x 60 > 1023 - T0: clipped
    # places 0-7 (strand pairs 0-3) are one lane half's, 8-11 the other's: at W1 and W2 no even
    # place of the first half fires, so there the odd field alone decides whether the lane fires
    order = [("min", m_rows), ("edge", e_rows), ("clip", k_rows), ("edge", e_rows), ("min", m_rows),
             ("edge", e_rows), ("min", m_rows), ("edge", e_rows), ("edge", e_rows), ("min", m_rows),
             ("zero", z_rows), ("edge", e_rows)]
    pats = [pwm(r, pid + 1, -a) for pid, (_, r) in enumerate(order)]
    w1 = "T" * NB_LEN
    w2 = "T" * ke + "G" + "T" * (NB_LEN - ke - 1)
    haps = {}
    marks = {"roles": [k for k, _ in order], "t0": t0, "w": {}, "super": 0}
    for lead in (0, 15, 16, 31, 2):  # the planted windows at phases 0, 15, 16 and 31 (W2 of lead 2)
        hap = "A" * lead + w1 + "AAA" + w2 + "A" * 7
        haps["lead%d" % lead] = hap
        marks["w"]["lead%d" % lead] = (lead, lead + NB_LEN + 3)
    return Case("neighbours", pats, haps, 0, marks)


@functools.lru_cache(None)
def neighbours():
    return fixed_point(_neighbours)


# ---------------------------------------------------------------------------
# every strand place
# ---------------------------------------------------------------------------
EP_LEN = 8


def _word(k):
    return "G" + "".join("ACGT"[(k >> (2 * d)) & 3] for d in range(4)) + "TCA"


@functools.lru_cache(None)
def every_place(n):
    """n literal strands of 8 columns (a mismatch costs the largest digit, so a window is a
    candidate iff it is the word iff it hits), each planted once, 9 bases apart: the window
    phases run through all 32.  Haplotype "n": N at bases 31 and 32, at the first column of
    one planted window and the last of another, the rest as "plain"."""
    pats, words = [], []
    for k in range(n):
        w = _word(k)
        words.append(w)
        pats.append(pwm([[100 if "ACGT"[b] == ch else -100 for b in range(4)] for ch in w], k + 1, 100 * EP_LEN - 1))
    lead = "CC"
    hap = lead + "A".join(words) + "ACC"
    at = [len(lead) + 9 * k for k in range(n)]
    withn = list(hap)
    nat = [p for p in (31, 32) if p < len(hap)]
    if n >= 2:
        nat += [at[0], at[1] + EP_LEN - 1]
    for p in nat:
        withn[p] = "N"
    return Case("every_place_%d" % n, pats, {"plain": hap, "n": "".join(withn)}, 0,
                {"at": at, "n_at": nat})


# ---------------------------------------------------------------------------
# depths, super tiles, windows
# ---------------------------------------------------------------------------
DEPTH_LENS = [(1, 4), (5, 20), (8, 40), (9, 30), (12, 4), (16, 30), (17, 30), (24, 34), (25, 20), (32, 20)]


def _consensus(rows):
    return "".join("ACGT"[max(range(4), key=lambda b: r[b])] for r in rows)


@functools.lru_cache(None)
def depths():
    """Four tiles of depths 1, 2, 3 and 4 (strand lengths 1, 5, 8 | 9, 12, 16 | 17, 24 |
    25, 32): a depth-1 and a depth-2 tile in class 0, both classes.  Haplotypes: every
    window count of the issue's list for either class, planted best windows (the last one
    ending at the last base; the very last base is a length-1 strand's), one haplotype past
    1024 bases, one with N."""
    rnd = random.Random(77)
    pats, cons, pid = [], {}, 0
    for L, count in DEPTH_LENS:
        for k in range(count):
            pid += 1
            if L == 1:
                rows = [[500 if b == k else -rnd.randint(200, 900) for b in range(4)]]
            else:
                rows = [[rnd.randint(-1000, 1000) for _ in range(4)] for _ in range(L)]
            best = sum(max(r) for r in rows)
            pats.append(pwm(rows, pid, best - rnd.randint(1, 600)))
            cons.setdefault(L, []).append(_consensus(rows))
    lmin = (1, 17)

    def hap(n, seed):
        r = random.Random(seed)
        s = [r.choice("ACGT") for _ in range(n)]
        # best windows of a strand of each length where they fit, the longest class's shortest last
        p = 0
        for L, _ in DEPTH_LENS:
            w = cons[L][seed % len(cons[L])]
            if p + L <= n - 17:
                s[p:p + L] = w
                p += L + (seed % 3)
        if n >= 17:
            s[n - 17:] = cons[17][seed % len(cons[17])]
        return "".join(s)
    haps = {}
    counts = (31, 32, 33, 63, 64, 65)
    lengths = {0, 1, lmin[1] - 1, lmin[1]} | {lmin[0] + k - 1 for k in counts} | {lmin[1] + k - 1 for k in counts}
    for n in sorted(lengths):
        haps["n%d" % n] = hap(n, 1000 + n)
    haps["n1100"] = hap(1100, 5)
    withn = list(hap(200, 9))
    for p in (0, 31, 32, 63, 64, 120, 199):
        withn[p] = "N"
    haps["withn"] = "".join(withn)
    return Case("depths", pats, haps, 0, {"lmin": lmin, "counts": counts})


# ---------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def lists():
    """16 strands (both lane halves' strand pairs) that every window hits: each pair of
    window tiles fires all 64 lanes twice and lists 1024 candidates."""
    rnd = random.Random(3)
    pats = []
    for k in range(16):
        rows = [[rnd.randint(-10, 10) for _ in range(4)] for _ in range(EP_LEN)]
        pats.append(pwm(rows, k + 1, sum(min(r) for r in rows) - 1))
    r = random.Random(4)
    return Case("lists", pats, {"n200": "".join(r.choice("ACGT") for _ in range(200))})


# ---------------------------------------------------------------------------
# scales
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def scales():
    """Weight spans 1, 7, 8, 1000 and 2^20, mixed / all-negative / all-positive columns,
    thresholds just under the best score, and strands that cannot hit (min_score >= C)."""
    rnd = random.Random(13)
    pats, cons, pid = [], [], 0
    for span in (1, 7, 8, 1000, 1 << 20):
        for kind in range(3):
            lo, hi = ((-span, span), (-span, -1), (1, span))[kind]
            for L in (5, 12, 20, 30):
                pid += 1
                rows = [[rnd.randint(lo, hi) for _ in range(4)] for _ in range(L)]
                best = sum(max(r) for r in rows)
                pats.append(pwm(rows, pid, best - rnd.randint(1, 1 + span * L // 3)))
                cons.append(_consensus(rows))
        for extra in (0, 5):  # never: D = C - min_score <= 0
            pid += 1
            rows = [[rnd.randint(-span, span) for _ in range(4)] for _ in range(11)]
            pats.append(pwm(rows, pid, sum(max(0, max(r)) for r in rows) + extra))
            cons.append(_consensus(rows))
    r = random.Random(14)
    haps = {}
    for h in range(3):
        parts = [c for i, c in enumerate(cons) if i % 3 == h]
        haps["h%d" % h] = "".join(p + r.choice("ACGT") for p in parts)[:420]
    withn = list(haps["h0"])
    for p in range(7, len(withn), 41):
        withn[p] = "N"
    haps["withn"] = "".join(withn)
    return Case("scales", pats, haps)


@functools.lru_cache(None)
def t0mix():
    """A tile of short literal strands (class 0) and long random ones (class 1): two super tiles whose
    common thresholds differ."""
    rnd = random.Random(5)
    pats, cons = [], []
    for k in range(64):
        w = _word(k)
        if k % 8 == 0:
            cons.append(w)
        pats.append(pwm([[100 if "ACGT"[b] == ch else -100 for b in range(4)] for ch in w], k + 1, 100 * EP_LEN - 1))
    for k in range(10):
        rows = [[rnd.randint(-1000, 1000) for _ in range(4)] for _ in range(24)]
        cons.append(_consensus(rows))
        pats.append(pwm(rows, 65 + k, sum(max(r) for r in rows) - rnd.randint(1, 600)))
    return Case("t0mix", pats, {"h": "C".join(cons) + "CC"})


def all_cases():
    d = depths()
    return [neighbours()] + [every_place(n) for n in (1, 2, 63, 64, 65)] + [d, d.with_budget(8), t0mix(), lists(),
                                                                            scales()]
