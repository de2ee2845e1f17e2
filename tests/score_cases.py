"""The pattern sets and regions of the score-row tests (test_gpu_scores.py), each the smallest
that reaches its path; test_scores_cpu.py checks with score_ref.py alone that each case bites.
A case is {"pats", "n", "beds", "regions", "seqs"}: seqs[r][x] = (codes, positions) of haplotype
id x of region r (dinuc_cases.hap_sequences).  A region may carry its own "inner" list
[(bed index, start, end)] (ranges that no bed selection would give); build() adds it as it is.
A case is built once per process and never modified."""
import functools
import random

import dinuc_cases as K
import encode_cases as E
from helpers import T

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
NUC = "ACGT"


def build(ps, case, **kw):
    """The case's regions as one RegionBatch (kw: RegionBatch's, build_device for instance)."""
    b = T.RegionBatch(ps, case["n"], **kw)
    for name, _ in case["beds"]:
        b.add_bed(name)
    for reg in case["regions"]:
        s, e = reg["merged"]
        b.begin(s, e, reg["ref"])
        for bi, a, z in (reg["inner"] if "inner" in reg else T.select_inner_peaks((s, e), case["beds"])):
            b.add_inner(bi, a, z)
        for rec in reg["records"]:
            b.add_record_carriers(rec[1], rec[2], rec[3], rec[4])
        b.end()
    return b


def mono(rnd, L, name, pid, direction=T.DIR_P, lo=-3000, hi=3000):
    return T.Pattern.PWM([T.Weight(*[rnd.randint(lo, hi) for _ in range(4)]) for _ in range(L)], name, pid, 0, direction)


def probe_batch(lmax, n):
    """A batch of a set whose longest pattern covers lmax bases: RegionBatch.ext sizes the regions."""
    return T.RegionBatch(T.PatternSet.from_patterns([mono(random.Random(0), lmax, "p", 0)]), n)


def region(rnd, lmax, n, s, length, sites):
    """A merged range of `length` bases from s; sites: [(index in the merged range, carrier ids)],
    an SNV each (a site without carriers is left out).  A best score is a maximum over the windows
    that start or end inside a range, so a range as wide as the region seldom moves with one SNV:
    the cases put narrow ranges ("inner") on their sites."""
    probe = probe_batch(lmax, n)
    e = s + length - 1
    es, ee = probe.ext(s, e)
    ref = [rnd.randrange(4) for _ in range(ee - es + 1)]
    recs = []
    for idx, car in sorted(sites):
        k = s - es + idx
        if car:
            recs.append(("car", es + k, NUC[ref[k]], NUC[(ref[k] + 1 + rnd.randrange(3)) % 4], sorted(car)))
    return {"merged": (s, e), "ref": "".join(NUC[c] for c in ref), "records": recs, "es": es, "ee": ee}


def finish(case):
    case["seqs"] = [K.hap_sequences(reg, case["n"]) for reg in case["regions"]]
    return case


SAMPLE_COUNTS = (1, 2, 63, 64, 65, 511, 512, 513, 1025)


@functools.lru_cache(None)
def sample_case(n):
    """n samples over three SNVs whose carriers follow the sample index (mod 3, mod 5, odd / mod 7):
    six and more distinct pairs, neighbours with different sums, so 8- and 11-byte fields mix all
    along a row."""
    rnd = random.Random(1064)  # (the same reference and weights for every n)
    pats = [mono(rnd, 6, "m6", 0), mono(rnd, 9, "m9", 1), mono(rnd, 9, "m9", 1, T.DIR_N)]
    a = [2 * s for s in range(n) if s % 3 == 0]
    b = [2 * s + 1 for s in range(n) if s % 5 in (0, 1)]
    c = [2 * s for s in range(n) if s % 2 == 1] + [2 * s + 1 for s in range(n) if s % 7 == 3]
    reg = region(rnd, 9, n, 7000, 24, [(10, a), (11, b), (12, c)])
    reg["inner"] = [(0,) + reg["merged"], (0, 7010, 7012)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def haps_case(kind):
    """one: no record, one distinct haplotype; two: one SNV; pairs: six samples over four
    distinct haplotypes whose (left, right) pairs all differ."""
    rnd = random.Random(77)
    pats = [mono(rnd, 6, "m6", 0)]
    n, sites = {"one": (5, []), "two": (5, [(8, [1, 2, 6])]),
                "pairs": (6, [(8, [1, 4, 5, 9]), (14, [3, 6, 8, 9])])}[kind]
    reg = region(rnd, 6, n, 3000, 24, sites)
    reg["inner"] = [(0,) + reg["merged"], (0, 3008, 3014)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def patterns_case():
    """Pattern id 0: a forward and a reverse strand of independent weights (each wins somewhere);
    1: two strands of the same weights (a tie between strands); 2: a dinucleotide PWM, both strands;
    3: a strand of 36 columns; 4: a TFBS_KIND_OTHER pattern (none everywhere: no row)."""
    rnd = random.Random(5)
    n = 9
    regs = [region(rnd, 36, n, 20000 + 400 * r, 60,
                   [(4 + 9 * j, rnd.sample(range(2 * n), rnd.randint(1, 7))) for j in range(6)]) for r in range(2)]
    calib = K.codes_of(regs[0]["ref"])
    tie = mono(rnd, 7, "tie", 1)
    pats = [mono(rnd, 6, "fr", 0), mono(rnd, 6, "fr", 0, T.DIR_N), tie,
            T.Pattern.PWM(tie.weights, "tie", 1, 0, T.DIR_N)] + K.both_strands(rnd, 2, 5, calib) + \
        [mono(rnd, 36, "long", 3), T.Pattern.OtherPattern("other", 4)]
    for r in regs:
        s = r["merged"][0]
        r["inner"] = [(0,) + r["merged"], (1, s + 10, s + 30)] + [(1, s + 4 + 9 * j, s + 5 + 9 * j) for j in range(6)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", []), ("b.bed", [])], "regions": regs})


@functools.lru_cache(None)
def extreme_case():
    """A 1-column PWM with weights INT32_MAX (A) and INT32_MIN (C, G, T) under an inner range of one
    base, C in the reference, C>A carried by both haplotypes of sample 0 and one of sample 2: the
    sums are 2 INT32_MAX, 2 INT32_MIN and -1, the spread 2^33 - 2."""
    rnd = random.Random(9)
    n = 3
    probe = probe_batch(1, n)
    s, e = 900, 919
    es, ee = probe.ext(s, e)
    ref = [rnd.randrange(4) for _ in range(ee - es + 1)]
    k = s - es + 7
    ref[k] = 1
    reg = {"merged": (s, e), "ref": "".join(NUC[c] for c in ref), "es": es, "ee": ee,
           "records": [("car", es + k, "C", "A", [0, 1, 4])], "inner": [(0, es + k, es + k)]}
    pats = [T.Pattern.PWM([T.Weight(INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN)], "one", 0, 0)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", [])], "regions": [reg]})


NONE_L = 6


@functools.lru_cache(None)
def none_case():
    """A deletion of 12 bases carried by two haplotype ids: under the 2-base inner range inside it
    (n.bed) the deletion haplotype has no window (none starts or ends there), so that candidate
    writes no row although the other haplotypes' values differ (an SNV beside it); under a
    wider range around it (w.bed) every haplotype has a value."""
    rnd = random.Random(21)
    n = 6
    reg = region(rnd, NONE_L, n, 11000, 50, [(20, [0, 3, 7])])
    idx = reg["merged"][0] - reg["es"] + 10
    K.add_deletion(reg, idx, 12, [5, 8])
    a = reg["es"] + idx + 8
    reg["inner"] = [(0, a, a + 1), (1, a - 12, a + 12)]
    pats = [mono(rnd, NONE_L, "m6", 0)]
    return finish({"pats": pats, "n": n, "beds": [("n.bed", []), ("w.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def keys_case():
    """Two beds; forty distinct inner ranges in a.bed, the first of them listed twice (written
    once); in b.bed a range of a.bed again (a row per bed), nested ranges and an empty one."""
    rnd = random.Random(40)
    n = 7
    reg = region(rnd, 8, n, 50000, 150, [(6 + 14 * j, rnd.sample(range(2 * n), rnd.randint(1, 6))) for j in range(10)])
    s = reg["merged"][0]
    inner = [(0, s + 3 * i, s + 3 * i + 20) for i in range(40)] + [(0, s, s + 20)]
    inner += [(1, s + 15, s + 35), (1, s + 10, s + 100), (1, s + 20, s + 50), (1, s + 30, s + 29)]
    rnd.shuffle(inner)
    reg["inner"] = inner
    pats = [mono(rnd, 8, "m8", 3), mono(rnd, 5, "m5", 1)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", []), ("b.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def fallback_case():
    """91 distinct haplotypes (level k carries the first k of 90 SNVs) over 8 293 samples whose
    pairs are encode_cases.pair_list's 8 193 distinct ones: one more than the pair table lists."""
    rnd = random.Random(91)
    pairs = E.pair_list(8193, "shuffled", 3)
    lev = [l[1] for p in pairs for l in p]
    n = len(pairs)
    sites = [(2 + j, [h for h in range(2 * n) if lev[h] > j]) for j in range(90)]
    reg = region(rnd, 6, n, 90000, 96, sites)
    reg["inner"] = [(0,) + reg["merged"], (0, 90010, 90012), (0, 90040, 90070)]
    pats = [mono(rnd, 6, "m6", 0)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", [])], "regions": [reg]})


@functools.lru_cache(None)
def multi_case():
    """Five regions: 0-1 and 3 with a few SNVs (grouped on the device when the batch asks for it),
    2 with 70 records (more than the device grouper takes: built on the host), 4 without a record."""
    rnd = random.Random(314)
    n = 40
    ids = range(2 * n)
    regs = []
    for r, n_sites in enumerate((4, 6, 70, 5, 0)):
        regs.append(region(rnd, 9, n, 30000 + 500 * r, 90,
                           [(1 + j * (88 // max(n_sites, 1)), rnd.sample(ids, rnd.randint(1, 5 if n_sites > 9 else 30)))
                            for j in range(n_sites)]))
    pats = [mono(rnd, 6, "m6", 0), mono(rnd, 9, "m9", 2), mono(rnd, 9, "m9", 2, T.DIR_N)]
    for r in regs:
        s = r["merged"][0]
        r["inner"] = [(0,) + r["merged"], (1, s + 20, s + 60), (1, s + 1, s + 3), (1, s + 22, s + 24)]
    return finish({"pats": pats, "n": n, "beds": [("a.bed", []), ("b.bed", [])], "regions": regs})
