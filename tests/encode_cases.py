"""The cases that pin the device genotype encoding (pair_table_kernel, key_encode_kernel)
and the device BGZF writer (bgzf_gpu.hip) at their limits.

The driver chooses every sample's total exactly.  Pattern_id 1 is a one-column PWM that
scores 'A' on the forward strand and 'T' on the reverse strand, pattern_ids 2.. score 'A'
only; min_score 999, L_max 1, so the extended window is the merged range and a
haplotype's count is the number of its A (and T) bases.  A haplotype is a *level* (D, k): it
carries one deletion of D bases (0: none) and the A->C SNVs at the region's first k 'A'
positions (nested carrier sets), which takes D + k hits away on an A/T-only reference and k
on any other.  Distinct levels are distinct haplotypes, so the list of (left level, right
level) per sample fixes the number of distinct totals, their range, the number of distinct
ordered haplotype pairs and -- through the sample order -- the genotype text's run
structure.

Nothing here comes from the library: test_encode_cases_cpu.py proves with the oracle alone
that every case sits on its edge, test_gpu_encode_edges.py compares the product with the
oracle's rows on the same cases.  A case is built once per process and never modified.
"""
import functools
import random

from helpers import T, run_oracle

N_IDS = 12          # pattern_ids registered (a case uses the first n_ids of them)
REGION_LEN = 1400
LONG_LEN = 33100    # the two range cases (about test_long_region_vs_oracle's 33 kb)
DEL_AT = 250        # index of a deletion's anchor base in a long region
REGION_STEP = 40000
BLOCK_TEXT = 65280  # uncompressed bytes of a full BGZF block
MAX_PAIRS = 8192    # kEncMaxPairs
N_MIX = 8293        # the mixed batch's samples (the largest case's)

LO_TEXT, HI_TEXT = "0|0:0.0", "1|1:2.0"


@functools.lru_cache(maxsize=None)
def pattern_set(n_ids):
    pats = [T.Pattern.PWM([T.Weight(1000, 0, 0, 0)], "A1", 1, 999, T.DIR_P),
            T.Pattern.PWM([T.Weight(0, 0, 0, 1000)], "A1", 1, 999, T.DIR_N)]
    for pid in range(2, n_ids + 1):
        pats.append(T.Pattern.PWM([T.Weight(1000, 0, 0, 0)], "A%d" % pid, pid, 999, T.DIR_P))
    return T.PatternSet.from_patterns(pats)


@functools.lru_cache(maxsize=None)
def reference(kind, seed, length):
    rnd = random.Random(seed)
    return "".join(rnd.choice("AT" if kind == "at" else "AACGT") for _ in range(length))


def snv(k):
    return (0, k)


def region_spec(pairs, kind="mix", seed=1, length=REGION_LEN):
    """pairs: per sample its (left level, right level)."""
    return {"kind": kind, "seed": seed, "length": length, "pairs": [tuple(p) for p in pairs]}


def reduction(level):
    return level[0] + level[1]


def build_region(spec, s0, n_samples=None):
    """helpers.build_batch's region dict of a spec at merged start s0; n_samples: pad the
    sample list with copies of its last pair (same levels, totals and pairs)."""
    ref = reference(spec["kind"], spec["seed"], spec["length"])
    pairs = list(spec["pairs"])
    if n_samples is not None:
        assert n_samples >= len(pairs)
        pairs += [pairs[-1]] * (n_samples - len(pairs))
    lev = [l for p in pairs for l in p]
    a_idx = [i for i, c in enumerate(ref) if c == "A"]
    kmax = max(l[1] for l in lev)
    dels = sorted({l[0] for l in lev if l[0]})
    assert kmax < len(a_idx)
    recs = []
    by_k = sorted(range(len(lev)), key=lambda h: -lev[h][1])  # carriers of SNV j: the haplotypes with k > j
    n_car = 0
    cars = []
    for j in range(kmax - 1, -1, -1):
        while n_car < len(by_k) and lev[by_k[n_car]][1] > j:
            n_car += 1
        cars.append((j, sorted(by_k[:n_car])))
    for j, car in reversed(cars):
        recs.append(("car", s0 + a_idx[j], "A", "C", car))
    if dels:
        assert spec["kind"] == "at" and (kmax == 0 or a_idx[kmax - 1] < DEL_AT) and DEL_AT + dels[-1] < len(ref)
        for d in dels:
            recs.append(("car", s0 + DEL_AT, ref[DEL_AT:DEL_AT + d + 1], ref[DEL_AT],
                         [h for h in range(len(lev)) if lev[h][0] == d]))
    return {"merged": (s0, s0 + len(ref) - 1), "ref": ref, "records": recs}


# ---------------------------------------------------------------------------------------
# sample lists

def sum_set(rnd, nv, R):
    """nv distinct reductions in [0, R]: both ends, the totals around the 32-bit word
    boundaries of key_encode_kernel's bitmap (lo + 32, 31, 33, 64, 63, 65, ...: the lowest
    total is the reduction R), then random ones."""
    first = [0, R] + [R - x for x in (32, 31, 33, 64, 63, 65, 1, 96, 95, 97)]
    out = []
    for v in first:
        if len(out) < nv and 0 <= v <= R and v not in out:
            out.append(v)
    rest = [v for v in range(R + 1) if v not in out]
    rnd.shuffle(rest)
    out += rest[:nv - len(out)]
    assert len(out) == nv
    return sorted(out)


def split(rnd, d, K):
    """d = a + b with both levels <= K, a != b where d allows it."""
    lo, hi = max(0, d - K), min(K, d)
    a = rnd.randint(lo, hi)
    if 2 * a == d and lo < hi:
        a = a - 1 if a > lo else a + 1
    return (a, d - a)


def value_pairs(seed, nv, n, R):
    """n samples with exactly nv distinct totals of range R; beyond the first nv samples the
    same total comes from the swapped pair and from another split."""
    rnd = random.Random(seed)
    K = (R + 1) // 2 + 2
    sums = sum_set(rnd, nv, R)
    pairs = [split(rnd, d, K) for d in sums]
    for i in range(n - nv):
        a, b = pairs[(i // 2 + 1) % nv]
        if i % 2 == 0 and a != b:
            pairs.append((b, a))
        else:
            for _ in range(20):
                c = split(rnd, a + b, K)
                if c not in ((a, b), (b, a)):
                    break
            pairs.append(c)
    rnd.shuffle(pairs)
    return [(snv(a), snv(b)) for a, b in pairs]


def pair_list(n_pairs, order, seed):
    """The first n_pairs ordered pairs (a, b) of 91 levels, 100 of them once more (40 times
    the first, so that sorted a wave starts with equal pairs); sorted or shuffled."""
    allp = [(a, b) for a in range(91) for b in range(91)][:n_pairs]
    rnd = random.Random(seed)
    pairs = allp + [allp[0]] * 40 + rnd.sample(allp[1:], 60)
    if order == "sorted":
        pairs.sort()
    else:
        rnd.shuffle(pairs)
    return [(snv(a), snv(b)) for a, b in pairs]


def with_runs(pairs):
    """pairs, then runs of the lowest total's pair (8-byte text: 40 and 33 samples), the
    highest's (32) and another's (11-byte text: 24, 23 and 30), each behind a sample of a
    fourth text: the runs bgzf_block_kernel's serial writer cuts into matches of <= 258 bytes."""
    by_sum = sorted(pairs, key=lambda p: reduction(p[0]) + reduction(p[1]))
    hi, lo = by_sum[0], by_sum[-1]
    mids = [p for p in by_sum if reduction(p[0]) + reduction(p[1]) not in
            (reduction(hi[0]) + reduction(hi[1]), reduction(lo[0]) + reduction(lo[1]))]
    mid, sep = mids[len(mids) // 2], mids[0]
    assert reduction(mid[0]) + reduction(mid[1]) != reduction(sep[0]) + reduction(sep[1])
    out = list(pairs)
    for p, count in ((lo, 40), (lo, 33), (hi, 32), (mid, 24), (mid, 23), (mid, 30)):
        out += [sep] + [p] * count
    return out + [sep]


def from_sums(sums):
    return [(snv(d // 2), snv(d - d // 2)) for d in sums]


def value_sums(width):
    """12 (4-bit codes) or 40 (8-bit codes) reductions; 0 is the highest total ('1|1:2.0'),
    the largest the lowest ('0|0:0.0')."""
    return [0] + [3 + 3 * i for i in range(10 if width == 4 else 38)] + [150]


def run_sums(width):
    """Sorted-order structure: runs of the 8-byte texts of 32 and 33 samples, of an 11-byte
    text of 23 and 24, runs of 960, 961 and 1 100 samples that start off a 64-sample group,
    and a run of 2 500 samples across the first block boundary."""
    V = value_sums(width)
    hi, lo, mid = V[0], V[-1], V[1:-1]
    seps = mid[6:8]
    out = list(V)
    state = {"sep": 0}

    def sep():
        out.append(seps[state["sep"] & 1])
        state["sep"] += 1

    def run(v, count, start_mod=None):
        sep()
        if start_mod is not None:
            while len(out) % 64 != start_mod:
                sep()
        out.extend([v] * count)

    run(lo, 32), run(lo, 33), run(hi, 32), run(hi, 33)
    run(mid[0], 23), run(mid[0], 24), run(mid[1], 23)
    run(mid[2], 960, 7), run(mid[3], 961, 13), run(lo, 1100, 37), run(mid[4], 1500, 50)
    run(mid[5], 2500, 21)
    run(hi, 70), sep()
    return out


def round_robin_sums(width):
    """Every value once, then round-robins of period 2, 8 and 9 over distinct texts (both
    8-byte texts among them)."""
    V = value_sums(width)
    out = list(V)
    for period, count in ((2, 2000), (8, 2400), (9, 2700)):
        texts = [V[-1], V[1], V[0]] + V[2:period - 1] if period > 2 else [V[1], V[-1]]
        assert len(set(texts)) == period
        out += [texts[i % period] for i in range(count)]
    return out


# ---------------------------------------------------------------------------------------
# the cases

def _case(name, regions, n_ids=1, mult=1, path=None, blocks=(), prop=None, min_maf=0):
    n = len(regions[0]["pairs"])
    assert all(len(r["pairs"]) == n for r in regions)
    return {"name": name, "regions": regions, "n_samples": n, "n_ids": n_ids, "mult": mult, "path": path,
            "blocks": tuple(blocks), "prop": prop or {}, "min_maf": min_maf}


def width_of(nv):
    return "w2" if nv <= 4 else "w4" if nv <= 16 else "w8" if nv <= 255 else "values"


VALUE_CASES = [  # (distinct totals, samples, range): n % 4 in {0, 1, 2, 3}, tiny n, n around 64 and 512
    (2, 2, 32), (2, 3, 33), (4, 5, 33), (4, 64, 33), (5, 5, 64), (5, 63, 65), (16, 18, 97), (16, 65, 100),
    (17, 63, 97), (17, 513, 100), (255, 256, 600), (255, 513, 599), (256, 258, 600), (256, 513, 601),
    (257, 259, 600), (257, 513, 640)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for i, (nv, n, R) in enumerate(VALUE_CASES):
        out.append(_case("vals_%d_n%d" % (nv, n), [region_spec(value_pairs(100 + i, nv, n, R), seed=10 + i)],
                         path=width_of(nv), prop={"n_vals": nv, "range": R, "n_mod4": n % 4,
                                                  "same_total": n >= nv + 2, "words": nv >= 4}))
    # range: hi - lo = 65 535 (the bitmap's last bit) and 65 536 (host path), a few samples more
    # with deletions spread over the bitmap's 2 048 words (key_encode_kernel's cross-thread rank prefix)
    spread = [257, 1031, 2049, 4099, 8191, 8193, 12000, 16385, 20000, 24001, 28000, 30011, 32001]
    for name, top, path, rng in (("range_65535", ((32767, 1), (32767, 0)), "w4", 65535),
                                 ("range_65536", ((32768, 0), (32768, 0)), "range", 65536)):
        pairs = [(snv(0), snv(0)), top]
        for j, d in enumerate(spread):
            pairs.append(((d, 0), (d, 1)) if j % 3 == 0 else ((d, 0), snv(j)) if j % 3 == 1 else (snv(0), (d, 2)))
        pairs += [top, ((spread[3], 0), (spread[5], 0))]
        out.append(_case(name, [region_spec(pairs, "at", 3, LONG_LEN)], path=path,
                         prop={"range": rng, "n_vals": len({reduction(a) + reduction(b) for a, b in pairs}),
                               "n_mod4": len(pairs) % 4, "spread_words": 256}))
    for n_pairs, path in ((8192, "w8"), (8193, "no_pairs")):
        for order in ("sorted", "shuffled"):
            blocks = ("wave",) + (("stored",) if order == "shuffled" and n_pairs == 8192 else ())
            out.append(_case("pairs_%d_%s" % (n_pairs, order), [region_spec(pair_list(n_pairs, order, n_pairs), seed=5)],
                             path=path, blocks=blocks,
                             prop={"n_pairs": n_pairs, "repeated": True, "order": order, "n_vals": 180}))
    for mult in (2, 3):  # the same bed range listed mult times: a 4-bit and an 8-bit key
        out.append(_case("mult_%d" % mult, [region_spec(value_pairs(300 + mult, 10, 50 + mult, 70), seed=31),
                                            region_spec(value_pairs(310 + mult, 30, 50 + mult, 90), seed=32)],
                         mult=mult, prop={"paths": ["w4", "w8"], "mult": mult}))
    out.append(_case("maf", [region_spec(value_pairs(320, 6, 41, 64), seed=33),
                             region_spec(value_pairs(321, 20, 41, 90), seed=34)], prop={"paths": ["w4", "w8"], "maf": True}))
    for width in (4, 8):
        out.append(_case("runs_w%d" % width, [region_spec(from_sums(run_sums(width)), seed=40)], path="w%d" % width,
                         blocks=("wave",), prop={"runs": True}))
        out.append(_case("round_robin_w%d" % width, [region_spec(from_sums(round_robin_sums(width)), seed=41)],
                         path="w%d" % width, blocks=("wave",), prop={"round_robin": True}))
    # block composition: what bgzf_plan_kernel cannot stage goes to bgzf_block_kernel
    out.append(_case("block_value_texts", [region_spec(value_pairs(400, 210, 1900, 500), seed=50)], n_ids=4, path="w8",
                     blocks=("block",), prop={"n_vals": 210, "row_bytes": (18000, 23000), "rows": 4}))
    out.append(_case("block_encoded_rows", [region_spec(with_runs(value_pairs(401, 20, 420, 90)), seed=51)],
                     n_ids=12, path="w8", blocks=("block",), prop={"row_bytes": (5000, 7200), "rows": 12}))
    tiny = [region_spec(value_pairs(410 + j, 17 if j == 4 else 2 + j % 3, 20, 40), seed=52 + j) for j in range(10)]
    out.append(_case("block_tiny_rows", tiny, n_ids=12, blocks=("block",),
                     prop={"paths": ["w8" if j == 4 else "w2" for j in range(10)], "rows": 120,
                           "row_bytes": (100, 400)}))
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def names():
    return [c["name"] for c in cases()]


def materialize(c, first=0, n_samples=None, n_ids=None):
    """(pattern set, n_samples, beds, regions) of a case as a batch of its own, or of its
    regions as regions first.. of a larger one."""
    regions = [build_region(r, 10000 + REGION_STEP * (first + j), n_samples) for j, r in enumerate(c["regions"])]
    beds = [("edges.bed", [r["merged"] for r in regions for _ in range(c["mult"])])]
    return pattern_set(n_ids or c["n_ids"]), n_samples or c["n_samples"], beds, regions


FALLBACK_PATHS = ("values", "range", "no_pairs")


@functools.lru_cache(maxsize=None)
def mixed_order():
    """Every case, the not-encoded ones (8 193 pairs, 257 values, range 65 536) each between
    encoded ones."""
    enc = [c["name"] for c in cases() if c["path"] not in FALLBACK_PATHS]
    fb = [c["name"] for c in cases() if c["path"] in FALLBACK_PATHS]
    out = []
    for i, name in enumerate(enc):
        out.append(name)
        if i < len(fb):
            out.append(fb[i])
    assert len(fb) < len(enc)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed():
    """All cases as regions of one batch of N_MIX samples under pattern_id 1 (each case's
    sample list padded with its last pair; bed multiplicity 1): (pattern set, n, beds,
    regions, [(case name, region of the case, region of the batch)])."""
    regions, where = [], []
    for name in mixed_order():
        c = case(name)
        _, _, _, regs = materialize(c, len(regions), N_MIX, 1)
        for j, r in enumerate(regs):
            where.append((name, j, len(regions)))
            regions.append(r)
    beds = [("edges.bed", [r["merged"] for r in regions])]
    return pattern_set(1), N_MIX, beds, regions, tuple(where)


def region_paths(c):
    """The declared path of each region's keys."""
    return c["prop"]["paths"] if c["path"] is None else [c["path"]] * len(c["regions"])


@functools.lru_cache(maxsize=None)
def oracle(name, min_maf=0):
    """(keys per region, rows) of a case as its own batch, or of the mixed batch (name
    'mixed'), from the oracle."""
    ps, n, beds, regions = mixed()[:4] if name == "mixed" else materialize(case(name))
    keys, rows, _ = run_oracle(ps, n, beds, regions, min_maf=min_maf)
    return keys, rows


def key_path(left, right, n_pairs):
    """The path the encoding's limits give a key with these per-sample counts."""
    tot = [(a + b) & 0xFFFFFFFF for a, b in zip(left, right)]
    if len(set(tot)) == 1:
        return None  # not a varying key
    if n_pairs > MAX_PAIRS:
        return "no_pairs"
    if max(tot) - min(tot) >= 65536:
        return "range"
    return width_of(len(set(tot)))


def expected_stats(keys, pair_counts):
    """tfbs_batch_encode_stats' counters for the oracle's keys of regions with these numbers
    of distinct ordered haplotype pairs."""
    out = {k: 0 for k in ("keys", "w2", "w4", "w8", "no_pairs", "range", "values")}
    for region_keys, n_pairs in zip(keys, pair_counts):
        for (left, right) in region_keys.values():
            p = key_path(left, right, n_pairs)
            if p:
                out["keys"] += 1
                out[p] += 1
    return out


def pair_count(spec):
    return len(set(spec["pairs"]))


def maf_of(row):
    """min_maf's quantity from a row's freqs= (counts_as_genotypes: the samples outside the
    most frequent genotype class, ties to 0|0, then 1|1)."""
    info = row.split("\t")[7]
    zero, one, two = (int(x) for x in info.split("freqs=")[1].split(";")[0].split("/"))
    if zero >= one and zero >= two:
        return one + two
    if two >= zero and two >= one:
        return zero + one
    return zero + two


def maf_threshold():
    """The larger maf of the 'maf' case's two rows: kept at min_maf = it, dropped at + 1."""
    _, rows = oracle("maf")
    return max(maf_of(r) for r in rows.split("\n") if r)
