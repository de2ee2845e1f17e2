"""The pattern sets, regions and expected keys of the LUT and generic count-path tests.

Everything expected here comes from lut_ref.py (plain Python) and from the oracle's
patch_haplotype; nothing is fed from the library's scan or plan.  test_lut_cpu.py checks the
model against the oracle and the conditions that make the cases bite; test_gpu_lut_counts.py
compares the product with the same expectations.  A case is built once per process
(functools.lru_cache) and never modified.
"""
import functools
import random

import dinuc_cases as K
import dinuc_ref as D
import lut_ref as R
from helpers import T

INT32_MIN, INT32_MAX = K.INT32_MIN, K.INT32_MAX
codes_of = K.codes_of


def pwm(cols, name, pid, thr, direction=T.DIR_P):
    return T.Pattern.PWM([T.Weight(*c) for c in cols], name, pid, thr, direction)


def rand_cols(rnd, L, lo=-2000, hi=2000):
    return [[rnd.randint(lo, hi) for _ in range(4)] for _ in range(L)]


def narrow_cols(rnd, L):
    """Weights of +-1000: a strand of 32 columns stays within 32768 of its best score."""
    return rand_cols(rnd, L, -1000, 1000)


def deep_cols(rnd, L):
    """Columns whose first gives one base 40000: the windows that start with it score far above
    the rest, so a threshold among the rest lies more than 32768 below the best score."""
    cols = rand_cols(rnd, L)
    cols[0][rnd.randrange(4)] = 40000
    return cols


def a_high_cols(rnd, L):
    """A is every column's highest weight and positive: an N scored as A raises the sum."""
    return [[rnd.randint(1200, 2000)] + [rnd.randint(-2000, 1000) for _ in range(3)] for _ in range(L)]


def a_low_cols(rnd, L):
    """A is every column's lowest weight and negative: an N scored as A lowers the sum."""
    return [[rnd.randint(-2000, -1200)] + [rnd.randint(-1000, 2000) for _ in range(3)] for _ in range(L)]


def wrap_cols(rnd, L):
    """About a third of the weights are +-2^30, +-(2^31 - 1) or -2^31: sums leave int32."""
    return [[rnd.choice(K.BIG) if rnd.random() < 0.35 else rnd.randint(-3, 3) for _ in range(4)] for _ in range(L)]


def quad_cols(rnd, L):
    """2^30 for A in column 0 and -2^30 for C in column 1: a window can span 2^31, which keeps the
    strand off the matrix cores (and off the octet units)."""
    cols = rand_cols(rnd, L)
    cols[0][0] = 1 << 30
    cols[1][1] = -(1 << 30)
    return cols


def revcomp(cols):
    return [list(reversed(c)) for c in reversed(cols)]


def wrapped_scores(cols, codes):
    return [D.wrap32(v) for v in K.mono_scores(cols, codes)]


def attained(cols, calib, frac, above=None):
    sc = wrapped_scores(cols, calib)
    if above is not None:
        sc = [v for v in sc if v > above]
    return K.attained_threshold(sc, frac)


def strand(rnd, pid, L, calib, frac, cols_of=rand_cols, direction=T.DIR_P, name=None, above=None):
    cols = cols_of(rnd, L)
    return pwm(cols, name or "m%d" % pid, pid, attained(cols, calib, frac, above), direction)


def both_strands(rnd, pid, L, calib, frac=0.88, cols_of=rand_cols, name=None, above=None):
    cols = cols_of(rnd, L)
    fwd = pwm(cols, name or "m%d" % pid, pid, attained(cols, calib, frac, above), T.DIR_P)
    rev = pwm(revcomp(cols), fwd.name, pid, attained(revcomp(cols), calib, frac, above), T.DIR_N)
    return [fwd, rev]


def probe_batch(lmax, n_samples=1):
    """A batch of a set whose longest pattern has lmax columns: RegionBatch.ext sizes the regions."""
    return T.RegionBatch(T.PatternSet.from_patterns([pwm([[0, 0, 0, 0]] * lmax, "p", 0, 0)]), n_samples)


def plant(reg, idx, bases):
    """Writes `bases` (codes 0-3) into the reference from index idx (no record may lie there)."""
    lo, hi = reg["es"] + idx, reg["es"] + idx + len(bases) - 1
    assert all(not (lo <= r[1] + k <= hi) for r in reg["records"] for k in range(len(r[2])))
    ref = reg["ref"]
    reg["ref"] = ref[:idx] + "".join(K.NUC[c] for c in bases) + ref[idx + len(bases):]
    assert len(reg["ref"]) == len(ref)


def window_stats(case, pats=None):
    """Model-only counts over the distinct haplotypes' windows: hits with an N first / last, windows
    whose decision with N scored as A differs from the exact one in each direction (and those of
    them on strands of 32 columns or more than 32), hits starting past an indel, sums outside
    int32, windows tied with the threshold."""
    st = dict.fromkeys(("n_first", "n_last", "a_hits_exact_not", "exact_hits_a_not", "differ_32", "differ_long",
                        "after_indel", "outside_int32", "tied", "hits"), 0)
    for sq in case["seqs"]:
        for codes, pos in set(sq):
            brk = next((j for j in range(len(pos) - 1) if pos[j + 1] != pos[j] + 1), None)
            as_a = [0 if c == 4 else c for c in codes]
            has_n = 4 in codes
            for p in pats or case["pats"]:
                L = len(p)
                ex = R.exact_scores(p, codes)
                ta = R.exact_scores(p, as_a) if has_n else ex
                for i, v in enumerate(ex):
                    hit = D.wrap32(v) > p.min_score
                    hit_a = D.wrap32(ta[i]) > p.min_score
                    st["hits"] += hit
                    st["n_first"] += hit and codes[i] == 4
                    st["n_last"] += hit and codes[i + L - 1] == 4
                    st["a_hits_exact_not"] += hit_a and not hit
                    st["exact_hits_a_not"] += hit and not hit_a
                    st["differ_32"] += hit != hit_a and L == 32
                    st["differ_long"] += hit != hit_a and L > 32
                    st["after_indel"] += hit and brk is not None and i > brk
                    st["outside_int32"] += not INT32_MIN <= v <= INT32_MAX
                    st["tied"] += D.wrap32(v) == p.min_score
    return st


# ---------------------------------------------------------------------------------------
# a. several tiles, both unit kinds
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case_tiles():
    """66 ids of 1-3 columns with one and two strands (pattern_ids 10..75), 9 two-strand ids of 32
    columns and one five-strand id of 4, 4, 7, 31 and 32 columns among them (pattern_ids 0..9): more
    than 64 slots and more blocks than a tile holds, slot order unlike the id order.  Every third
    strand is a deep one (its threshold more than 32768 below its best: a quad strand), so octet and
    quad units share tiles and ids have a strand of each kind; neither kind's strands fill their
    units."""
    rnd = random.Random(2101)
    n = 4
    probe = probe_batch(32)
    regions = [K.make_region(rnd, probe, n, 40000, 80, 10), K.make_region(rnd, probe, n, 50000, 83, 10)]
    calib = codes_of(regions[0]["ref"])
    pats, count = [], 0

    def add(pid, lengths, frac):
        nonlocal count
        for k, L in enumerate(lengths):
            deep = count % 3 == 2
            pats.append(strand(rnd, pid, L, calib, 0.5 if deep else frac,
                               deep_cols if deep else narrow_cols if L > 30 else rand_cols,
                               T.DIR_N if k & 1 else T.DIR_P))
            count += 1
    for k in range(66):
        add(10 + k, [(1,), (2, 2), (3,), (1, 3)][k % 4], 0.7)
    for pid in range(10):
        add(pid, (4, 4, 7, 31, 32) if pid == 4 else (32, 32), 0.88)
    for i, p in enumerate(pats):
        best = sum(max(c) for c in R.columns(p))
        assert (best - p.min_score > 32768) == (i % 3 == 2) == (not R.is_octet(p)), (i, best, p.min_score)
    beds = []
    for name, cut in (("a.bed", None), ("b.bed", 40)):
        beds.append((name, [(r["merged"][0], r["merged"][1] if cut is None else r["merged"][0] + cut)
                            for r in regions]))
    beds.append(("c.bed", [(r["merged"][0] + 30, r["merged"][1]) for r in regions]))
    return R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# b. window and haplotype geometry
# ---------------------------------------------------------------------------------------
GEOMETRY_WINDOWS = (1, 63, 64, 65, 128, 129, 191, 192, 193, 256, 257, 513)
GEOMETRY_LENGTHS = (1, 4, 5, 9, 32)


@functools.lru_cache(None)
def case_geometry():
    """Ten strands of 1, 4, 5, 9 and 32 columns in one tile; one region per window count of
    GEOMETRY_WINDOWS for the 1-column strands (= the haplotype's length): the 64-window chunk and
    256-window pass edges, the three-chunk tail, two passes and a tail.  The 32-column strands have
    31 windows fewer, or none.  Haplotypes shorter than an extended range come from a reference cut
    short, as at a contig end.  A last region's random carriers among 70 samples give more than 128
    distinct haplotypes: more than one workgroup's share, the last group partial."""
    rnd = random.Random(2202)
    n = 70
    probe = probe_batch(32, n)
    regions = []
    for k, nwin in enumerate(GEOMETRY_WINDOWS):
        s = 10000 + 3000 * k
        if nwin < 63:
            regions.append(K.make_region(rnd, probe, n, s, 1, 2, ref_len=nwin, max_car=3))
        else:
            regions.append(K.make_region(rnd, probe, n, s, nwin - 62, 4, max_car=3))
        assert len(regions[-1]["ref"]) == nwin
    regions.append(K.make_region(rnd, probe, n, 60000, 40, 24, max_car=n))
    calib = codes_of(regions[-2]["ref"])
    pats = []
    for pid, L in enumerate(GEOMETRY_LENGTHS):
        pats += both_strands(rnd, pid, L, calib, frac=0.8)
    beds = [("a.bed", [(r["es"], r["ee"]) for r in regions]),
            ("b.bed", [r["merged"] for r in regions] + [(r["merged"][0], r["merged"][0] + 70) for r in regions])]
    return R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# c. N and indels
# ---------------------------------------------------------------------------------------
N_LENGTHS = (3, 6, 11, 20, 31, 32)


@functools.lru_cache(None)
def case_n_and_indels():
    """Three regions: N as a run of 3, alone (the first base of some windows, the last of others,
    column 31 of a 32-column strand's, the base just past a strand's last column) and at both ends
    of the reference; SNV carriers; insertions of 3 bases; deletions of 5, one running to the last
    base of the extended range.  Per length a strand whose A weights are its columns' highest (the
    table, which holds N as A, hits where the exact score does not), one whose A weights are the
    lowest (the reverse), and both strands of a random PWM of 9 and of 32 columns."""
    rnd = random.Random(2304)
    n = 6
    probe = probe_batch(32)
    H = list(range(2 * n))
    r0 = K.make_region(rnd, probe, n, 60000, 90, 6, n_at=(0, -1, 50, 51, 52, 75, 99, 121), avoid=set(range(28, 34)) |
                       set(range(84, 94)), max_car=4)
    K.add_insertion(r0, 30, "GTA", rnd.sample(H, 4))
    K.add_deletion(r0, 86, 5, rnd.sample(H, 4))
    r1 = K.make_region(rnd, probe, n, 70000, 70, 6, n_at=(0, 33, 60, 90), avoid=set(range(120, 132)) |
                       set(range(18, 24)), max_car=4)
    last = len(r1["ref"]) - 1
    K.add_deletion(r1, last - 5, 5, rnd.sample(H, 5))
    K.add_insertion(r1, 20, "CCA", rnd.sample(H, 3))
    r2 = K.make_region(rnd, probe, n, 80000, 64, 5, n_at=(-1, 26, 27, 28, 44, 70, 100), avoid=set(range(20, 26)) |
                       set(range(58, 68)), max_car=4)
    K.add_insertion(r2, 22, "TTG", rnd.sample(H, 5))
    K.add_deletion(r2, 60, 5, rnd.sample(H, 5))
    regions = [r0, r1, r2]
    calib = codes_of(r0["ref"])
    pats, pid = [], 0
    for L in N_LENGTHS:
        pats.append(strand(rnd, pid, L, calib, 0.75, a_high_cols, name="ahi%d" % L))
        pats.append(strand(rnd, pid + 1, L, calib, 0.75, a_low_cols, T.DIR_N, name="alo%d" % L))
        pid += 2
    for L in (9, 32):
        pats += both_strands(rnd, pid, L, calib, frac=0.8)
        pid += 1
    beds = [("a.bed", [r["merged"] for r in regions]),
            ("b.bed", [(r["es"], r["merged"][0] + 10) for r in regions] + [(r["merged"][1] - 5, r["ee"] + 3)
                                                                           for r in regions])]
    case = R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})
    case["stats"] = window_stats(case)
    return case


# ---------------------------------------------------------------------------------------
# d. reduction paths
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case_reduction():
    """Regions with 40, 8 and 9 nested inner ranges sharing the merged start (the counting passes
    take 8 at a time: five full passes, one exactly full, one with a single range left), and a
    region whose bed lists one range twice."""
    rnd = random.Random(2405)
    n = 5
    probe = probe_batch(31)
    regions = [K.make_region(rnd, probe, n, 30000, 110, 10), K.make_region(rnd, probe, n, 33000, 60, 8),
               K.make_region(rnd, probe, n, 36000, 60, 8), K.make_region(rnd, probe, n, 39000, 60, 8)]
    calib = codes_of(regions[0]["ref"])
    pats = []
    for pid, L in enumerate((4, 7, 12, 31)):
        pats += both_strands(rnd, pid, L, calib, frac=0.8)
    (s0, e0), (s1, e1), (s2, e2), (s3, e3) = [r["merged"] for r in regions]
    beds = [("a.bed", [(s0, s0 + 20 + 2 * k) for k in range(40)] + [(s1, s1 + 20 + 4 * k) for k in range(8)] +
             [(s2, s2 + 20 + 4 * k) for k in range(9)] + [(s3, e3), (s3, e3)]),
            ("b.bed", [(s3 + 10, e3)])]
    assert [len(T.select_inner_peaks(r["merged"], beds)) for r in regions] == [40, 8, 9, 3]
    return R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# e. arithmetic edges
# ---------------------------------------------------------------------------------------
def octet_edge_strands(rnd, calib, pid):
    """Pairs of strands on either side of each clause of the octet rule (the first of a pair is an
    octet strand, the second a quad one), every threshold but the first pair's an attained score."""
    pats = []
    # biased threshold exactly -32768 and -32769: columns of +-4000 (a block's range <= 32000)
    cols = rand_cols(rnd, 12, -4000, 4000)
    top = sum(max(c) for c in cols)
    for k, thr in enumerate((top - 32768, top - 32769)):
        pats.append(pwm(cols, "bias%d" % k, pid + k, thr))
    # one block whose range is 32767, then 32768
    for k, rng in enumerate((32767, 32768)):
        cols = [[0, rng - 3000] + [rnd.randint(0, rng - 3000) for _ in range(2)]]
        cols += [[0, 1000] + [rnd.randint(0, 1000) for _ in range(2)] for _ in range(3)]
        for c in cols:
            rnd.shuffle(c)
        pats.append(pwm(cols, "range%d" % k, pid + 2 + k, attained(cols, calib, 0.6)))
    # the blocks' magnitudes sum to 2^30 - 1, then to 2^30: four blocks near 2^28, ranges small
    for k, target in enumerate(((1 << 30) - 1, 1 << 30)):
        cols = rand_cols(rnd, 16, 0, 1500)
        rest = target - sum(max(c) for c in cols)
        for b in range(4):
            off = rest // 4 if b < 3 else rest - 3 * (rest // 4)
            cols[4 * b] = [w + off for w in cols[4 * b]]
        pats.append(pwm(cols, "mag%d" % k, pid + 4 + k, attained(cols, calib, 0.6)))
    for k, p in enumerate(pats):
        assert R.is_octet(p) == (k % 2 == 0), p
    return pats


@functools.lru_cache(None)
def case_arithmetic():
    """Per length one strand of wrap_cols under four thresholds -- INT32_MIN (every score but
    INT32_MIN hits), INT32_MAX (none), an attained score and that score minus 1 -- each its own
    pattern_id; the octet rule's edges (octet_edge_strands); one strand more, so that the last quad
    unit is padded.  The reference holds the all-lowest and the all-highest window of the two `bias`
    strands (twelve columns of +-4000: the lowest window's 16-bit sum saturates on the way)."""
    rnd = random.Random(2506)
    n = 4
    probe = probe_batch(32)
    reg = K.make_region(rnd, probe, n, 90000, 70, 8, n_at=(40,), avoid=set(range(60, 90)))
    calib = codes_of(reg["ref"])
    pats, pid = [], 0
    for L in (2, 3, 6, 13, 32):
        cols = wrap_cols(rnd, L)
        att = attained(cols, calib, 0.6)
        for thr in (INT32_MIN, INT32_MAX, att, max(INT32_MIN, att - 1)):
            pats.append(pwm(cols, "w%d" % pid, pid, thr))
            pid += 1
    edges = octet_edge_strands(rnd, calib, pid)
    pats += edges
    pid += len(edges)
    pats.append(strand(rnd, pid, 7, calib, 0.6, wrap_cols))
    plant(reg, 62, R.extreme_window(edges[0], False))
    plant(reg, 76, R.extreme_window(edges[0], True))
    s, e = reg["merged"]
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 25), (s + 35, e)])]
    case = R.finish({"pats": pats, "n": n, "regions": [reg], "beds": beds, "calib": calib, "edges": edges})
    case["stats"] = window_stats(case)
    return case


# ---------------------------------------------------------------------------------------
# f. the generic kernel
# ---------------------------------------------------------------------------------------
GENERIC_LENGTHS = (33, 36, 64, 65, 100)


@functools.lru_cache(None)
def case_generic():
    """Both strands of 33 (A the highest weight), 36 (A the lowest), 64, 65 and 100 columns and one
    pattern_id with strands of 5 and 36 columns: six generic tiles.  Region 0 has 9 nested inner
    ranges, N inside long windows, an insertion and a deletion, and more than 256 windows; region
    1's reference is cut short to 50 bases, shorter than three of the lengths; region 2 has N at
    both ends of the reference."""
    rnd = random.Random(2607)
    n = 4
    probe = probe_batch(100)
    H = list(range(2 * n))
    r0 = K.make_region(rnd, probe, n, 100000, 100, 6, n_at=(40, 41, 150, 260), avoid=set(range(58, 64)) |
                       set(range(198, 208)), max_car=3)
    K.add_insertion(r0, 60, "GTA", rnd.sample(H, 3))
    K.add_deletion(r0, 200, 5, rnd.sample(H, 3))
    r1 = K.make_region(rnd, probe, n, 110000, 1, 3, ref_len=50, n_at=(20,), max_car=3)
    r2 = K.make_region(rnd, probe, n, 120000, 40, 5, n_at=(0, -1, 90, 130), max_car=3)
    regions = [r0, r1, r2]
    assert len(r0["ref"]) - 33 + 1 > 256
    calib = codes_of(r0["ref"])
    pats = []
    for pid, (L, cols_of) in enumerate(zip(GENERIC_LENGTHS, (a_high_cols, a_low_cols, rand_cols, rand_cols, rand_cols))):
        pats += both_strands(rnd, pid, L, calib, frac=0.85, cols_of=cols_of)
    pats.append(strand(rnd, 5, 5, calib, 0.85))
    pats.append(strand(rnd, 5, 36, calib, 0.85, direction=T.DIR_N))
    s0, e0 = r0["merged"]
    beds = [("a.bed", [(s0, s0 + 20 + 8 * k) for k in range(9)] + [r1["merged"], r2["merged"]]),
            ("b.bed", [(r2["es"], r2["merged"][0] + 10), (r2["merged"][1] - 5, r2["ee"])])]
    assert len(T.select_inner_peaks(r0["merged"], beds)) == 9
    case = R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})
    case["stats"] = window_stats(case)
    return case


# ---------------------------------------------------------------------------------------
# g. LUT groups between matrix-core groups
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case_interleaved():
    """Pattern_ids 0..11, each both strands, a pair (2 k, 2 k + 1) of one length: the even ids are
    matrix-core eligible, the odd ones carry quad_cols' 2^30 / -2^30 column pair and stay on the LUT
    path, so the slot order alternates between the two.  Id 12 has an eligible strand and a quad
    one: its group stays on the LUT path and brings an octet strand there."""
    rnd = random.Random(2708)
    n = 5
    probe = probe_batch(16)
    regions = [K.make_region(rnd, probe, n, 20000, 100, 10), K.make_region(rnd, probe, n, 23000, 90, 10)]
    K.add_insertion(regions[1], 50, "ACA", rnd.sample(range(2 * n), 3))
    calib = codes_of(regions[0]["ref"])
    pats = []
    for pid in range(12):
        L = 6 + 2 * (pid // 2)
        if pid & 1:
            pats += both_strands(rnd, pid, L, calib, 0.5, quad_cols, above=1 << 29)
        else:
            pats += both_strands(rnd, pid, L, calib, 0.85)
    pats.append(strand(rnd, 12, 16, calib, 0.85))
    pats.append(strand(rnd, 12, 16, calib, 0.5, quad_cols, T.DIR_N, above=1 << 29))
    beds = [("a.bed", [r["merged"] for r in regions]),
            ("b.bed", [(r["merged"][0], r["merged"][0] + 40) for r in regions])]
    return R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# h. one pattern_id larger than a tile
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case_big_group():
    """Pattern_id 0 has 9 octet and 5 quad strands of 32 columns: two units of each kind, 32 blocks,
    128 KiB of tables in one tile (a tile's default is 20 blocks, 80 KiB).  Its last strand has
    quad_cols' column pair, which keeps the group off the matrix cores.  Ids 1 and 2 are small."""
    rnd = random.Random(2809)
    n = 4
    probe = probe_batch(32)
    regions = [K.make_region(rnd, probe, n, 70000, 80, 8)]
    calib = codes_of(regions[0]["ref"])
    pats = []
    for k in range(14):
        deep = k >= 9
        pats.append(strand(rnd, 0, 32, calib, 0.5 if deep else 0.85, deep_cols if deep else narrow_cols,
                           T.DIR_N if k & 1 else T.DIR_P, name="big"))
    pats[13] = strand(rnd, 0, 32, calib, 0.5, quad_cols, T.DIR_N, name="big", above=1 << 29)
    pats += both_strands(rnd, 1, 8, calib, 0.85) + both_strands(rnd, 2, 12, calib, 0.85)
    assert [R.is_octet(p) for p in pats[:14]] == [True] * 9 + [False] * 5
    s, e = regions[0]["merged"]
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 30), (s + 20, e)])]
    return R.finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


def refused_group():
    """One pattern_id of 41 octet strands of 32 columns: six units, 48 blocks, 192 KiB."""
    rnd = random.Random(2910)
    cols = [rand_cols(rnd, 32) for _ in range(41)]
    return [pwm(c, "huge", 0, sum(max(x) for x in c) - 9000, T.DIR_N if k & 1 else T.DIR_P) for k, c in enumerate(cols)]


CASES = {"tiles": case_tiles, "geometry": case_geometry, "n_and_indels": case_n_and_indels,
         "reduction": case_reduction, "arithmetic": case_arithmetic, "generic": case_generic,
         "interleaved": case_interleaved, "big_group": case_big_group}
