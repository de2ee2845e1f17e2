"""What the affinity-row tests add to score_cases.py: the two cases at the ends of the sums' range,
and the values that sit on the logarithm's table boundaries.  A case is score_cases' dictionary,
built once per process and never modified."""
import functools
import os
import random
import re

import dinuc_cases as K
import score_cases as SC
from helpers import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "find-tfbs_amd", "csrc", "affinity_log_table.hpp")
NUC = "ACGT"


@functools.lru_cache(None)
def zero_case():
    """A 1-column PWM with weights 0 (A) and -30000 (C, G, T) under an inner range of one base: top
    is 0, an A weighs 2^40 and any other base 0 (30000 lies beyond the weight's cutoff, 27725).  C in
    the reference, C>A carried by both haplotypes of sample 0 and one of sample 2: the sums are 2^41,
    0 and 2^40, so lo = mlog2(0) = -1, hi = 41000, and sample 2 at 40000 takes an 11-byte field."""
    rnd = random.Random(19)
    n = 3
    probe = SC.probe_batch(1, n)
    s, e = 1900, 1919
    es, ee = probe.ext(s, e)
    ref = [rnd.randrange(4) for _ in range(ee - es + 1)]
    k = s - es + 7
    ref[k] = 1
    reg = {"merged": (s, e), "ref": "".join(NUC[c] for c in ref), "es": es, "ee": ee,
           "records": [("car", es + k, "C", "A", [0, 1, 4])], "inner": [(0, es + k, es + k)]}
    pats = [T.Pattern.PWM([T.Weight(0, -30000, -30000, -30000)], "zero", 0, 0)]
    return SC.finish({"pats": pats, "n": n, "beds": [("a.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def large_case():
    """An all-zero-weight strand of four columns over the whole merged range of 300 bases: top is 0
    and every window weighs 2^40, so a haplotype's sum is its window count times 2^40 and a sample's
    lies near 2^49.  Two deletions (12 and 30 bases) with different carriers change the counts."""
    rnd = random.Random(23)
    n = 8
    reg = SC.region(rnd, 4, n, 5000, 300, [])
    idx = reg["merged"][0] - reg["es"]
    K.add_deletion(reg, idx + 40, 12, [1, 4, 5, 10])
    K.add_deletion(reg, idx + 150, 30, [2, 5, 7, 11, 12])
    reg["inner"] = [(0,) + reg["merged"]]
    pats = [T.Pattern.PWM([T.Weight(0, 0, 0, 0)] * 4, "flat", 0, 0)]
    return SC.finish({"pats": pats, "n": n, "beds": [("a.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def long_case():
    """A strand of 36 columns whose weights stay within +-300, so that its windows lie inside the
    weight's cutoff (score_cases.patterns_case's 36-column strand has weights up to 3000: every
    window lies beyond 27725 below its top, every sum is 0 and it writes no affinity row), beside a
    6-column strand; SNVs every nine bases under narrow and wide ranges."""
    rnd = random.Random(36)
    n = 9
    reg = SC.region(rnd, 36, n, 24000, 60, [(4 + 9 * j, rnd.sample(range(2 * n), rnd.randint(1, 7))) for j in range(6)])
    s = reg["merged"][0]
    reg["inner"] = [(0,) + reg["merged"], (1, s + 10, s + 30)] + [(1, s + 4 + 9 * j, s + 5 + 9 * j) for j in range(6)]
    pats = [SC.mono(rnd, 36, "long", 3, lo=-300, hi=300), SC.mono(rnd, 6, "m6", 5)]
    return SC.finish({"pats": pats, "n": n, "beds": [("a.bed", []), ("b.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def committed_table():
    """The 1 000 constants of the committed header."""
    vals = [int(x, 16) for x in re.findall(r"0x([0-9A-F]{16})ull", open(TABLE).read())]
    assert len(vals) == 1000
    return vals


BOUNDARY_EXPONENTS = (1, 13, 40, 41, 62, 63)


@functools.lru_cache(None)
def boundary_values():
    """The values at which mlog2 steps: 0, 1, 2, 3, 2^63 - 1, 2^63, 2^64 - 1; for every j and every e of
    BOUNDARY_EXPONENTS the boundary b = ceil(P[j] / 2^(63 - e)) -- the least x of exponent e whose
    normalised value reaches P[j] -- and its neighbours b - 1 and b + 1; 4 000 random values, half of
    them of a random bit length."""
    P = committed_table()
    xs = [0, 1, 2, 3, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]
    for e in BOUNDARY_EXPONENTS:
        sh = 63 - e
        for p in P:
            b = (p + (1 << sh) - 1) >> sh
            xs += [b - 1, b, b + 1]
    rnd = random.Random(1000)
    xs += [rnd.getrandbits(64) for _ in range(2000)]
    xs += [rnd.getrandbits(rnd.randint(1, 64)) for _ in range(2000)]
    return tuple(x for x in xs if 0 <= x < 1 << 64)
