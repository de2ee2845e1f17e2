"""The pattern sets, regions and expected keys of the dinucleotide count-path tests.

Everything expected here comes from dinuc_ref.py (plain Python) and from the oracle's
patch_haplotype; nothing is fed from the library's scan.  test_dinuc_cpu.py checks the
conditions that make the cases bite (hits in every pattern_id, windows with N, hits past an
indel, sums that wrap ...) on the reference alone; test_gpu_dinuc_counts.py compares the
product with the same expectations.  A case is built once per process (functools.lru_cache)
and never modified.
"""
import functools
import random
import tempfile

import dinuc_ref as D
import oracle_py as O
from helpers import T, make_regions_synth, run_oracle, synth_patterns

NUC = "ACGTN"
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
BIG = [1 << 30, -(1 << 30), INT32_MAX, -INT32_MAX, INT32_MIN]


def rand_rows(rnd, L, lo=-2000, hi=2000):
    return [[rnd.randint(lo, hi) for _ in range(16)] for _ in range(L - 1)]


def wrap_rows(rnd, L):
    """Rows whose sums leave int32: about a third of the weights are +-2^30, +-(2^31 - 1) or -2^31."""
    return [[rnd.choice(BIG) if rnd.random() < 0.35 else rnd.randint(-3, 3) for _ in range(16)] for _ in range(L - 1)]


def exact_sum(rows, codes, i):
    """The unwrapped score (an N pair adds 0)."""
    return sum(row[4 * codes[i + j] + codes[i + j + 1]] for j, row in enumerate(rows)
               if codes[i + j] != 4 and codes[i + j + 1] != 4)


def attained_threshold(all_scores, frac=0.88):
    """A score of `all_scores` with about 1 - frac of them strictly above it, and at least
    one: where the quantile is the maximum itself, the next score below it."""
    s = sorted(all_scores)
    v = s[min(len(s) - 1, int(frac * len(s)))]
    below = [x for x in s if x < v]
    return below[-1] if v == s[-1] and below else v


def strands(rnd, pid, lengths, calib, name=None, rows_of=rand_rows, frac=0.88):
    """One pattern_id with a strand of independent rows per length, directions alternating;
    every threshold is a score that the strand attains on `calib`."""
    out = []
    for k, L in enumerate(lengths):
        rows = rows_of(rnd, L)
        out.append(T.Pattern.DiPWM(rows, name or "di%d" % pid, pid, attained_threshold(D.scores(rows, calib), frac),
                                   T.DIR_N if k & 1 else T.DIR_P))
    return out


def both_strands(rnd, pid, L, calib, name=None, frac=0.88):
    rows = rand_rows(rnd, L)
    return [T.Pattern.DiPWM(rw, name or "di%d" % pid, pid, attained_threshold(D.scores(rw, calib), frac), d)
            for d, rw in ((T.DIR_P, rows), (T.DIR_N, D.reverse_rows(rows)))]


def probe_batch(lmax, n_samples=1):
    """A batch of a set whose longest pattern covers lmax bases: RegionBatch.ext sizes the regions."""
    ps = T.PatternSet.from_patterns([T.Pattern.DiPWM(rand_rows(random.Random(0), lmax), "p", 0, 0)])
    return T.RegionBatch(ps, n_samples)


def codes_of(ref):
    return [NUC.index(c) for c in ref]


def make_region(rnd, probe, n_samples, s, merged_len, n_sites, ref_len=None, n_at=(), avoid=(), max_car=None):
    """A merged range of merged_len bases from s with n_sites SNVs at distinct positions (random
    carriers), none on an N or on an index of `avoid`.  ref_len: a reference cut short, as at
    a contig end.  n_at: indices of the reference that hold an N (negative: from its end)."""
    e = s + merged_len - 1
    es, ee = probe.ext(s, e)
    n = ee - es + 1 if ref_len is None else ref_len
    ref = [rnd.randrange(4) for _ in range(n)]
    for i in n_at:
        ref[i] = 4
    free = [i for i in range(n) if ref[i] != 4 and i not in avoid]
    recs = []
    for k in sorted(rnd.sample(free, min(n_sites, len(free)))):
        alt = rnd.choice([c for c in range(4) if c != ref[k]])
        car = sorted(rnd.sample(range(2 * n_samples), rnd.randint(1, max_car or n_samples)))
        recs.append(("car", es + k, NUC[ref[k]], NUC[alt], car))
    return {"merged": (s, e), "ref": "".join(NUC[c] for c in ref), "records": recs, "es": es, "ee": ee}


def add_insertion(reg, idx, bases, carriers):
    a = reg["ref"][idx]
    reg["records"].append(("car", reg["es"] + idx, a, a + bases, sorted(carriers)))
    reg["records"].sort(key=lambda r: r[1])


def add_deletion(reg, idx, n_deleted, carriers):
    """The n_deleted bases after index idx go; REF is the anchor plus them, ALT the anchor."""
    r = reg["ref"][idx:idx + n_deleted + 1]
    assert len(r) == n_deleted + 1 and "N" not in r
    reg["records"].append(("car", reg["es"] + idx, r, r[0], sorted(carriers)))
    reg["records"].sort(key=lambda r: r[1])


def hap_sequences(reg, n_samples):
    """Per haplotype id (2 * sample + side): (codes, positions), patched by the oracle's
    patch_haplotype from the id's own diff list.  Distinct diff lists must give distinct
    sequences here: where two give the same one, the reference keeps only one group's
    carriers (its HashMap insert), which these cases keep out of the way."""
    refh = [(c, reg["es"] + i) for i, c in enumerate(reg["ref"])]
    diffs = [[] for _ in range(2 * n_samples)]
    for _, pos, r, a, car in reg["records"]:
        for h in car:
            diffs[h].append((pos, r, a))
    cache = {}
    for d in diffs:
        key = tuple(d)
        if key not in cache:
            hp = O.patch_haplotype((reg["es"], reg["ee"]), d, refh)
            assert not isinstance(hp, int), hp
            cache[key] = (tuple(NUC.index(c) for c, _ in hp), tuple(p for _, p in hp))
    assert len(set(cache.values())) == len(cache), "two diff lists patch to one sequence"
    return [cache[tuple(d)] for d in diffs]


def expected_keys(pats, n_samples, beds, reg, seqs):
    """count_matches_by_sample from the reference, per haplotype id: {(bed, range, pattern_id):
    (L, R)} of the keys that some haplotype counts for.  A range that a bed lists twice is
    counted twice."""
    inner = T.select_inner_peaks(reg["merged"], beds)
    out = {}
    for p in pats:
        per_seq = {}
        for h, seq in enumerate(seqs):
            if seq not in per_seq:
                ms = D.matches(p.weights, p.min_score, seq[0], seq[1])
                per_seq[seq] = [D.count_overlaps(ms, (a, z)) for _, a, z in inner]
            for (bi, a, z), c in zip(inner, per_seq[seq]):
                if c:
                    lr = out.setdefault((beds[bi][0], (a, z), p.pattern_id), ([0] * n_samples, [0] * n_samples))
                    lr[h & 1][h >> 1] += c
    return out


def finish(case):
    """Adds the haplotype sequences and the expected keys of every region."""
    case["seqs"] = [hap_sequences(reg, case["n"]) for reg in case["regions"]]
    case["want"] = [expected_keys(case["pats"], case["n"], case["beds"], reg, sq)
                    for reg, sq in zip(case["regions"], case["seqs"])]
    return case


def total_hits(want):
    return sum(sum(l) + sum(r) for w in want for l, r in w.values())


def ids_with_a_key(want):
    return {k[2] for w in want for k in w}


def rebuild_rows(keys_per_region, beds, name_of, chrom="chr1", min_maf=0):
    """The rows of main.rs:415-429 from per-region keys: ordered by (inner start, inner end, bed,
    pattern_id), one row per key whose counts vary (counts_as_genotypes), numbered from 1."""
    bed_index = {name: i for i, (name, _) in enumerate(beds)}
    out, fake = [], 1
    for keys in keys_per_region:
        for (bed, (s, e), pid), (l, r) in sorted(keys.items(), key=lambda kv: (kv[0][1][0], kv[0][1][1],
                                                                             bed_index[kv[0][0]], kv[0][2])):
            g = O.counts_as_genotypes(l, r)
            if g is None or g[0] < min_maf:
                continue
            out.append("%s\t%d\t%s,%s,%d-%d\t.\t.\t.\tPASS\t%s\tGT:DS%s\n" % (chrom.replace("chr", ""), fake, bed,
                                                                              name_of(pid), s, e, g[1], g[2]))
            fake += 1
    return "".join(out)


# ---------------------------------------------------------------------------------------
# a. several tiles through counts
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case_tiles():
    """66 ids of 2-3 bases with one and two strands (pattern_ids 10..75), 9 two-strand ids of 32
    bases and one five-strand id of 4, 4, 7, 31 and 32 bases among them (pattern_ids 0..9): more
    than 64 slots and more lookup blocks than a tile holds, slot order unlike the id order."""
    rnd = random.Random(1101)
    n = 4
    probe = probe_batch(32)
    regions = [make_region(rnd, probe, n, 40000, 80, 10), make_region(rnd, probe, n, 50000, 83, 10)]
    calib = codes_of(regions[0]["ref"])
    pats = []
    for k in range(66):
        pats += strands(rnd, 10 + k, [(2,), (2, 2), (3,), (2, 3)][k % 4], calib, frac=0.7)
    for pid in range(10):
        if pid == 4:
            pats += strands(rnd, pid, (4, 4, 7, 31, 32), calib)
        else:
            pats += both_strands(rnd, pid, 32, calib)
    beds = []
    for name, cut in (("a.bed", None), ("b.bed", 40)):
        beds.append((name, [(r["merged"][0], r["merged"][1] if cut is None else r["merged"][0] + cut)
                            for r in regions]))
    beds.append(("c.bed", [(r["merged"][0] + 30, r["merged"][1]) for r in regions]))
    return finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# b. window and haplotype geometry
# ---------------------------------------------------------------------------------------
GEOMETRY_WINDOWS = (1, 63, 64, 65, 128, 129, 191, 192, 193, 256, 257)


def geometry_set(rnd, calib):
    pats = []
    for pid, L in enumerate((2, 5, 9)):
        pats += both_strands(rnd, pid, L, calib, frac=0.8)
    return pats


@functools.lru_cache(None)
def case_geometry():
    """Six strands of 2, 5 and 9 bases; one region per window count of GEOMETRY_WINDOWS (haplotype
    length - 2 + 1): the 64-window chunk and 256-window pass edges, the three-chunk tail.  One
    window needs a haplotype of 2 bases, less than any extended range: that region's reference
    is cut short, as at a contig end.  12 samples with SNVs."""
    rnd = random.Random(1202)
    n = 12
    probe = probe_batch(9)
    regions = []
    for k, nwin in enumerate(GEOMETRY_WINDOWS):
        hap_len = nwin + 1
        s = 10000 + 3000 * k
        if hap_len < 17:
            regions.append(make_region(rnd, probe, n, s, 1, 2, ref_len=hap_len, max_car=6))
        else:
            regions.append(make_region(rnd, probe, n, s, hap_len - 16, 8, max_car=6))
        assert len(regions[-1]["ref"]) == hap_len
    calib = codes_of(regions[-1]["ref"])
    pats = geometry_set(rnd, calib)
    beds = [("a.bed", [(r["es"], r["ee"]) for r in regions]),
            ("b.bed", [r["merged"] for r in regions] + [(r["merged"][0], r["merged"][0] + 70) for r in regions])]
    return finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


@functools.lru_cache(None)
def case_many_haplotypes():
    """One region of 70 samples whose random carriers give more than 128 distinct haplotypes:
    more than one workgroup's share, the last group partial."""
    rnd = random.Random(1203)
    n = 70
    probe = probe_batch(9, n)
    regions = [make_region(rnd, probe, n, 20000, 75, 14, max_car=n)]
    calib = codes_of(regions[0]["ref"])
    pats = geometry_set(rnd, calib)
    s, e = regions[0]["merged"]
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 30), (s + 20, e)])]
    return finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# c. N and indels with true pair weights
# ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case_n_and_indels():
    """Three regions: N as a run of 3, alone (the first base of some windows, the last of others)
    and at both ends of the reference; SNV carriers; an insertion of 3 bases; a deletion of 5;
    a deletion that runs to the last base of the extended range."""
    rnd = random.Random(1304)
    n = 6
    lmax = 20
    probe = probe_batch(lmax)
    H = list(range(2 * n))
    # region 0: N at both ends, a run of 3 and two single N; insertion and deletion
    r0 = make_region(rnd, probe, n, 60000, 90, 6, n_at=(0, -1, 50, 51, 52, 75, 99), avoid=set(range(28, 34)) |
                     set(range(84, 94)), max_car=4)
    add_insertion(r0, 30, "GTA", rnd.sample(H, 4))
    add_deletion(r0, 86, 5, rnd.sample(H, 4))
    # region 1: a deletion of 5 running to the last base of the extended range, single N
    r1 = make_region(rnd, probe, n, 70000, 70, 6, n_at=(0, 33, 60), avoid=set(range(96, 108)) | set(range(18, 24)),
                     max_car=4)
    last = len(r1["ref"]) - 1
    add_deletion(r1, last - 5, 5, rnd.sample(H, 5))
    add_insertion(r1, 20, "CCA", rnd.sample(H, 3))
    # region 2: a run of N right after an insertion, single N before and after a deletion
    r2 = make_region(rnd, probe, n, 80000, 64, 5, n_at=(-1, 26, 27, 28, 44, 70), avoid=set(range(20, 26)) |
                     set(range(58, 68)), max_car=4)
    add_insertion(r2, 22, "TTG", rnd.sample(H, 5))
    add_deletion(r2, 60, 5, rnd.sample(H, 5))
    regions = [r0, r1, r2]
    calib = codes_of(r0["ref"])
    pats = []
    for pid, L in enumerate((3, 3, 6, 6, 11, 11, 20, 20)):
        pats += both_strands(rnd, pid, L, calib, frac=0.8)
    beds = [("a.bed", [r["merged"] for r in regions]),
            ("b.bed", [(r["es"], r["merged"][0] + 10) for r in regions] + [(r["merged"][1] - 5, r["ee"] + 3)
                                                                           for r in regions])]
    case = finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})
    # the hits of the distinct haplotypes: how many windows hold an N, how many start past an indel
    with_n = after_indel = n_first = n_last = both = 0
    for sq in case["seqs"]:
        for codes, pos in set(sq):
            brk = next((j for j in range(len(pos) - 1) if pos[j + 1] != pos[j] + 1), None)
            for p in pats:
                L = len(p)
                for i, v in enumerate(D.scores(p.weights, codes)):
                    if v > p.min_score:
                        has_n = 4 in codes[i:i + L]
                        with_n += has_n
                        n_first += codes[i] == 4
                        n_last += codes[i + L - 1] == 4
                        after_indel += brk is not None and i > brk
                        both += has_n and brk is not None
    case["stats"] = {"with_n": with_n, "after_indel": after_indel, "n_first": n_first, "n_last": n_last,
                     "n_in_indel_haplotype": both}
    return case


# ---------------------------------------------------------------------------------------
# d. reduction paths
# ---------------------------------------------------------------------------------------
def reduction_beds(regions):
    s0, e0 = regions[0]["merged"]
    s1, e1 = regions[1]["merged"]
    assert e0 - s0 >= 20 + 2 * 39
    return [("a.bed", [(s0, s0 + 20 + 2 * k) for k in range(40)] + [(s1, e1), (s1, e1)]),  # 40 nested; one twice
            ("b.bed", [(s0, e0), (s1 + 10, e1)])]


@functools.lru_cache(None)
def case_reduction():
    """A dinucleotide-only set and the same strands beside mono PWMs; region 0 has 40 nested
    inner ranges sharing the merged start (five counting passes of 8), region 1's bed lists one
    range twice.  Mono keys come from the oracle, dinucleotide keys from the reference."""
    rnd = random.Random(1405)
    n = 5
    with tempfile.TemporaryDirectory() as tmpdir:
        mono, _ = synth_patterns(tmpdir, 4, 2, 31, thr=2e-3)
    ml = mono.to_list()
    lmax = mono.max_length
    assert 9 <= lmax <= 32
    probe = probe_batch(lmax)
    regions = [make_region(rnd, probe, n, 30000, 110, 10), make_region(rnd, probe, n, 33000, 60, 8)]
    calib = codes_of(regions[0]["ref"])
    first = max(p.pattern_id for p in ml) + 1
    di = []
    for k, L in enumerate((4, 7, lmax - 1, lmax)):  # both sets extend a region by the same lmax
        di += both_strands(rnd, first + k, L, calib, frac=0.8)
    beds = reduction_beds(regions)
    case = finish({"pats": di, "n": n, "regions": regions, "beds": beds, "calib": calib})
    okeys, orows, _ = run_oracle(mono, n, beds, regions)
    case.update(mono=ml, mono_keys=okeys, mono_rows=orows)
    return case


# ---------------------------------------------------------------------------------------
# e. arithmetic edges
# ---------------------------------------------------------------------------------------
def wrap_strands(rnd, calib, lengths=(2, 3, 6, 13, 32)):
    """Per length one strand of wrap_rows under four thresholds -- INT32_MIN (every score but
    INT32_MIN hits), INT32_MAX (none), an attained score and that score minus 1 -- each its
    own pattern_id, and one strand more, so that the last unit is padded."""
    pats, pid = [], 0
    for L in lengths:
        rows = wrap_rows(rnd, L)
        att = attained_threshold(D.scores(rows, calib), 0.6)
        for thr in (INT32_MIN, INT32_MAX, att, max(INT32_MIN, att - 1)):
            pats.append(T.Pattern.DiPWM(rows, "w%d" % pid, pid, thr, T.DIR_P))
            pid += 1
    rows = wrap_rows(rnd, 7)
    pats.append(T.Pattern.DiPWM(rows, "w%d" % pid, pid, attained_threshold(D.scores(rows, calib), 0.6), T.DIR_P))
    return pats


@functools.lru_cache(None)
def case_wrap():
    rnd = random.Random(1506)
    n = 4
    probe = probe_batch(32)
    regions = [make_region(rnd, probe, n, 90000, 70, 8, n_at=(40,))]
    calib = codes_of(regions[0]["ref"])
    pats = wrap_strands(rnd, calib)
    s, e = regions[0]["merged"]
    beds = [("a.bed", [(s, e)]), ("b.bed", [(s, s + 25), (s + 35, e)])]
    return finish({"pats": pats, "n": n, "regions": regions, "beds": beds, "calib": calib})


# ---------------------------------------------------------------------------------------
# f. all four kernels in one set
# ---------------------------------------------------------------------------------------
def mono_scores(w4, codes):
    L = len(w4)
    return [sum(0 if codes[i + j] == 4 else w4[j][codes[i + j]] for j in range(L)) for i in range(len(codes) - L + 1)]


@functools.lru_cache(None)
def case_all_kernels():
    """Matrix-core-eligible mono PWMs (pattern_ids 3, 5 .. 13), a mono PWM with weights of 2^30
    and -2^30 (15: the 32-bit quad path), one of 36 columns (17: the generic kernel) and dinucleotide ids
    0, 1, 2 (below every mono id), 4, 8, 12 (between them) and 20.  Regions with indels."""
    rnd = random.Random(1607)
    n = 6
    with tempfile.TemporaryDirectory() as tmpdir:
        synth, _ = synth_patterns(tmpdir, 6, 2, 31, thr=2e-3)
    mono = synth.to_list()
    for p in mono:
        p.pattern_id = 3 + 2 * p.pattern_id
    lmax = 36
    regions = make_regions_synth(7, 0, 3, n, lmax, 30)
    for r in regions:
        r["es"] = r["merged"][0] - lmax + 1
        r["ee"] = r["merged"][1] + lmax - 1
    calib = codes_of(regions[0]["ref"])
    quad = [[rnd.randint(-2000, 2000) for _ in range(4)] for _ in range(9)]
    quad[0][0] = 1 << 30  # with -2^30 in the next column a window can span 2^31: not matrix-core eligible
    quad[1][1] = -(1 << 30)
    thr = attained_threshold([v for v in mono_scores(quad, calib) if v > (1 << 29)], 0.5)
    mono.append(T.Pattern.PWM([T.Weight(*w) for w in quad], "quad", 15, thr))
    long_ = [[rnd.randint(-2000, 2000) for _ in range(4)] for _ in range(36)]
    mono.append(T.Pattern.PWM([T.Weight(*w) for w in long_], "long", 17,
                              attained_threshold(mono_scores(long_, calib), 0.9)))
    di = []
    for pid, L in ((0, 5), (1, 32), (2, 2), (4, 9), (8, 17), (12, 12), (20, 31)):
        di += both_strands(rnd, pid, L, calib, frac=0.85)
    s = [r["merged"] for r in regions]
    beds = [("a.bed", s), ("b.bed", [x for a, z in s for x in ((a, a + 60), (a, a + 40), (a + 30, z), (a + 50, a + 70))])]
    case = finish({"pats": di, "n": n, "regions": regions, "beds": beds, "calib": calib})
    mono_set = T.PatternSet.from_patterns(mono)
    assert mono_set.max_length == lmax
    okeys, orows, _ = run_oracle(mono_set, n, beds, regions)
    case.update(mono=mono, mono_keys=okeys, mono_rows=orows)
    return case
