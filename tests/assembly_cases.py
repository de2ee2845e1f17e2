"""The cases that pin the key assembly (key_kernels.hip: key_fast_kernel, key_asm_kernel) on
each of its limits, and the model that says which branch a case must take.

Every quantity the assembly branches on is chosen, not hoped for.  The PWMs are *literal
motifs*: weight 1 on the motif's base per column, 0 elsewhere, min_score L - 1, so only the
exact motif hits.  pattern_id 1 is the one-column motif 'A'; every other motif is made of C, G
and T with a G in its first, middle and last column; the background is C and T only.  So no
motif occurs in the background, none can overlap a plant partly, and the reference's hits are
exactly the plants (test_assembly_cases_cpu.py checks that by brute force).  Haplotypes are
distinct subsets of the region's variants (SNVs that break a planted motif or complete a
broken one, a deletion to the last base, an insertion), one haplotype id per subset and the
ids left over on the first subset, so the number of distinct haplotypes U is exact.

Columns count from the extended window's first base (merged start - 31).  A diff run [a, b]
of a haplotype makes window w of a strand of length L dirty iff a <= w + L - 1 and b >= w.

figures() derives, from the oracle's keys and the host batch accessors alone (no device),
what the assembly sees of a region: U, the reference hits nref, the dirty (haplotype,
reference hit, range) triples nD, the diff runs, the touched keys T, bounds of the listed
own hits.  predict() turns those into the TFBS_PATH_* word of tfbs_amd.h.
"""
import functools
import itertools
import random

from helpers import T, build_batch, run_oracle

LMAX = 32
MARGIN = LMAX - 1  # the "full" set's extension (its longest strand - 1)
LENGTHS = (1, 8, 9, 16, 17, 31, 32, 8, 16, 32)  # pattern_ids 1..10 of the "full" set
REVERSE = (8, 9)                                # ids with a reverse strand too (a motif of its own)
SHORT_IDS = 17                                  # the "short" set: 17 ids of length 8 (one depth class)
REGION_STEP = 40000
BASES = "ACGT"

# key_kernels.hip's limits, as tfbs_amd.h and DESIGN.md document them
SHAPES = {"small": dict(block=256, hap_lds=512, cor=3584, refs=256, cnt=3072, runs=1536, rows=256, lists=128),
          "big": dict(block=1024, hap_lds=2048, cor=8192, refs=256, cnt=24576, runs=12288, rows=1024, lists=256)}
BIG_U = 384
MAX_U, MAX_K, MAX_INNER, PAIR_LIMIT, REF_LIST = 2048, 16384, 32, 65536, 64
ASM = dict(haps=1024, runs=2048, hits=2048, refs=256, counters=6144)


def _motif(rnd, L):
    if L == 1:
        return "A"
    m = [rnd.choice("CGT") for _ in range(L)]
    m[0] = m[L // 2] = m[-1] = "G"
    return "".join(m)


@functools.lru_cache(maxsize=None)
def strands(kind="full"):
    """[(pattern_id, direction, L, motif)] of a pattern set."""
    rnd = random.Random(20240 + (0 if kind == "full" else 3))
    out = []
    if kind == "full":
        for pid, L in enumerate(LENGTHS, 1):
            out.append((pid, T.DIR_P, L, _motif(rnd, L)))
        for pid in REVERSE:
            out.append((pid, T.DIR_N, LENGTHS[pid - 1], _motif(rnd, LENGTHS[pid - 1])))
    elif kind == "short":
        for pid in range(1, SHORT_IDS + 1):
            out.append((pid, T.DIR_P, 8, _motif(rnd, 8)))
    else:  # "ids<n>": n ids of length 16 (the key count's edge)
        seen = set()
        while len(out) < int(kind[3:]):
            m = _motif(rnd, 16)
            if m not in seen:
                seen.add(m)
                out.append((len(out) + 1, T.DIR_P, 16, m))
    assert len({s[3] for s in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pattern_set(kind="full"):
    pats = []
    for pid, direction, L, motif in strands(kind):
        w = [T.Weight(*[1 if BASES[c] == ch else 0 for c in range(4)]) for ch in motif]
        pats.append(T.Pattern.PWM(w, "M%d" % pid, pid, L - 1, direction))
    return T.PatternSet.from_patterns(pats)


def margin(kind):
    """Columns before the merged range: the set's longest strand - 1."""
    return max(s[2] for s in strands(kind)) - 1


def n_ids(kind):
    return len({s[0] for s in strands(kind)})


def strand_of(kind, pid, direction=None):
    for i, s in enumerate(strands(kind)):
        if s[0] == pid and (direction is None or s[1] == direction):
            return i
    raise KeyError(pid)


# ---------------------------------------------------------------------------------------
# a region under construction

class Layout:
    """The reference window of one region: a C/T background of n columns with plants, the
    variants (column, reference bases, alternative) and the inner ranges (columns)."""

    def __init__(self, kind, merged_len, seed):
        self.kind = kind
        self.m = margin(kind)
        self.n = merged_len + 2 * self.m
        rnd = random.Random(seed)
        self.ref = [rnd.choice("CT") for _ in range(self.n)]
        self.plants = []    # (strand, window)
        self.variants = []  # (column, reference length, alternative)
        self.ranges = []
        self.used = [False] * self.n

    def plant(self, strand, w, broken_at=None):
        """The strand's motif at window w; broken_at: that column of it holds another base (no
        hit in the reference; an SNV can complete it)."""
        motif = strands(self.kind)[strand][3]
        assert 0 <= w and w + len(motif) <= self.n and not any(self.used[w:w + len(motif)]), (strand, w)
        for k, ch in enumerate(motif):
            self.ref[w + k] = ch
            self.used[w + k] = True
        if broken_at is None:
            self.plants.append((strand, w))
        else:
            assert motif[broken_at] != "G" and len(motif) > 1
            self.ref[w + broken_at] = "C" if motif[broken_at] == "T" else "T"

    def snv(self, col, alt=None):
        """An SNV at col: to another background base (never A or G), or to alt."""
        rb = self.ref[col]
        alt = alt or ("T" if rb != "T" else "C")
        assert alt != rb
        self.variants.append((col, 1, alt))
        return len(self.variants) - 1

    def deletion_to_end(self, col):
        self.variants.append((col, self.n - col, self.ref[col]))
        return len(self.variants) - 1

    def insertion(self, col, ins="CT"):
        self.variants.append((col, 1, self.ref[col] + ins))
        return len(self.variants) - 1

    def free(self, col, span=1):
        """The first column >= col with span unused columns."""
        while any(self.used[col:col + span]):
            col += 1
        assert col + span <= self.n
        return col


def subsets(sites, count, sizes, base=()):
    """The first count subsets of the variants `sites` with sizes in `sizes`, by size then
    order, each with the variants of base."""
    out = []
    for k in sizes:
        for c in itertools.combinations(sites, k):
            out.append(tuple(base) + c)
            if len(out) == count:
                return out
    raise AssertionError("not enough subsets")


def _spec(name, lay, haps, **kw):
    assert len(set(haps)) == len(haps)
    d = dict(name=name, kind=lay.kind, ref="".join(lay.ref), plants=tuple(lay.plants), variants=tuple(lay.variants),
             ranges=tuple(lay.ranges), haps=tuple(tuple(sorted(h)) for h in haps), edge=None, side=None,
             behind=None, env={})
    d.update(kw)
    return d


def build_region(spec, index, n_samples=None):
    """helpers.build_batch's region dict at merged start 10000 + REGION_STEP * index."""
    ref = spec["ref"]
    s = 10000 + REGION_STEP * index
    m = margin(spec["kind"])
    es = s - m
    H = 2 * (n_samples or samples_of(spec))
    U = len(spec["haps"])
    assert H >= U
    own = [spec["haps"][h] if h < U else spec["haps"][0] for h in range(H)]
    recs = []
    for v, (col, rlen, alt) in enumerate(spec["variants"]):
        car = [h for h in range(H) if v in own[h]]
        if car:
            recs.append(("car", es + col, ref[col:col + rlen], alt, car))
    recs.sort(key=lambda r: r[1])
    return {"merged": (s, s + len(ref) - 2 * m - 1), "ref": ref, "records": recs}


def samples_of(spec):
    return (len(spec["haps"]) + 1) // 2


def bed_ranges(spec, index):
    es = 10000 + REGION_STEP * index - margin(spec["kind"])
    return [(es + a, es + b) for a, b in spec["ranges"]]


def materialize(specs, n_samples=None):
    """(pattern set, n_samples, beds, regions) of specs as one batch."""
    kind = specs[0]["kind"]
    assert all(s["kind"] == kind for s in specs)
    n = n_samples or max(samples_of(s) for s in specs)
    regions = [build_region(s, i, n) for i, s in enumerate(specs)]
    beds = [("cases.bed", [r for i, s in enumerate(specs) for r in bed_ranges(s, i)])]
    return pattern_set(kind), n, beds, regions


# ---------------------------------------------------------------------------------------
# the families

def _default_ranges(lay, lo, hi):
    """Two nested ranges in a third and a disjoint one over the merged columns [lo, hi] (an
    inner range holds the merged range's first or last base, main.rs:62-72): a hit lies under 0
    (the gap, the margins), 1, 2 or 3 of them."""
    span = hi - lo
    lay.ranges = [(lo, lo + span * 5 // 10), (lo, lo + span * 3 // 10), (lo, lo + span * 15 // 100),
                  (lo + span * 7 // 10, hi)]


def _quad(lay, strand, col):
    """The four relations of a reference hit to a run [a, b], for one strand of length L, as
    two pairs of back-to-back plants: an SNV on the last column of the first plant (window
    a - L + 1: dirty) which is the column before the second (window b + 1: clean), and an SNV on
    the first column of the fourth plant (window b: dirty), the column after the third (window
    a - L: clean).  Returns (the two SNVs, the next free column)."""
    L = strands(lay.kind)[strand][2]
    if L == 1:  # AAAA with SNVs on its middle columns: one run [a, a + 1], hits at a - 1, a, a + 1, a + 2
        for k in range(4):
            lay.plant(strand, col + k)
        return [lay.snv(col + 1, "C"), lay.snv(col + 2, "C")], col + 5
    lay.plant(strand, col)
    lay.plant(strand, col + L)
    s1 = lay.snv(col + L - 1)
    lay.plant(strand, col + 2 * L + 1)
    lay.plant(strand, col + 3 * L + 1)
    s2 = lay.snv(col + 3 * L + 1)
    return [s1, s2], col + 4 * L + 2


def core():
    """Every strand length's four hit / run relations, an SNV every haplotype carries (no
    reference group: the helper copy of the reference), a deletion to the last base, an
    insertion, an SNV that completes a broken motif (an own hit), ranges with 0 to 3 bits."""
    lay = Layout("full", 640, 11)
    col, sites = 2, []
    for pid in (1, 2, 3, 4, 5, 8, 9):  # L = 1, 8, 9, 16, 17 forward, then the reverse strands' 8 and 16
        st = strand_of("full", pid, T.DIR_N if pid in REVERSE else T.DIR_P)
        v, col = _quad(lay, st, col)
        sites += v
    for pid in (6, 7):  # L = 31, 32
        v, col = _quad(lay, strand_of("full", pid), col)
        sites += v
    st8 = strand_of("full", 2)
    lay.plant(st8, col)  # the all-carrier SNV on its first column
    every = lay.snv(col)
    m8 = strands("full")[st8][3]
    k8 = next(k for k in range(1, 8) if m8[k] != "G")
    lay.plant(st8, col + 10, broken_at=k8)
    make = lay.snv(col + 10 + k8, m8[k8])
    lay.plant(strand_of("full", 10), col + 20)
    ins = lay.insertion(col + 19)  # the boundary run (a, a - 1) just before a plant
    lay.plant(st8, lay.n - 12)
    dele = lay.deletion_to_end(lay.n - 3)
    _default_ranges(lay, MARGIN, lay.n - 1 - MARGIN)
    haps = [(every,)] + [(every, v) for v in sites] + [(every, sites[i], sites[i + 3]) for i in range(0, 12, 2)]
    haps += [(every, make), (every, make, sites[2]), (every, ins), (every, ins, sites[5]), (every, dele),
             (every, dele, sites[0])]
    return _spec("core", lay, haps, edge="core")


def family(name, U, kind="full", n_a=0, n_plants=6, m_sites=None, sizes=(0, 1, 2, 3), every=False, merged_len=200,
           seed=1, ranges="default", extra=None, **kw):
    """U haplotypes over a region with n_a one-column 'A' hits and n_plants longer plants:
    SNV sites alternate between the last column of a plant (the hit at a - L + 1 dirty, the
    back-to-back plant after it clean), an 'A' (dirty for L = 1) and a blank column."""
    lay = Layout(kind, merged_len, seed)
    st = strands(kind)
    longer = [i for i, s in enumerate(st) if 1 < s[2] <= 9] or list(range(6))
    col, plant_sites = 1, []
    for k in range(n_plants):
        i = longer[k % len(longer)]
        L = st[i][2]
        col = lay.free(col, L)
        lay.plant(i, col)
        if k % 2 == 0:
            plant_sites.append(col + L - 1)
            col += L
        else:
            col += L + 2
    a_cols = []
    if n_a:
        one = strand_of(kind, 1)
        col = lay.free(col + 1, n_a)
        for k in range(n_a):
            lay.plant(one, col + k)
            a_cols.append(col + k)
        col += n_a + 1
    if m_sites is None:
        m_sites = 1
        while sum(len(list(itertools.combinations(range(m_sites), k))) for k in sizes) < U:
            m_sites += 1
    sites = []
    blank = col + 2
    for k in range(m_sites):
        if k % 3 == 0 and k // 3 < len(plant_sites):
            sites.append(lay.snv(plant_sites[k // 3]))
        elif k % 3 == 1 and 2 * (k // 3) + 1 < len(a_cols):
            sites.append(lay.snv(a_cols[2 * (k // 3) + 1], "C"))
        else:
            blank = lay.free(blank, 1)
            sites.append(lay.snv(blank))
            lay.used[blank] = True
            blank += 2  # (not adjacent: one run each)
    base = ()
    if every:
        c = lay.free(blank, 1)
        base = (lay.snv(c),)
    if ranges == "default":
        _default_ranges(lay, lay.m, lay.n - 1 - lay.m)
    else:
        lay.ranges = ranges(lay)
    haps = subsets(sites, U, sizes, base)
    if extra:
        haps = extra(lay, haps, sites)
    return _spec(name, lay, haps, **kw)


def nested(count, lo_pad=0):
    """count nested ranges sharing the merged start, each one column longer than the last."""
    def make(lay):
        hi = lay.n - 1 - lay.m
        return [(lay.m + lo_pad, hi - (count - 1) + k) for k in range(count)]
    return make


def _listed(name, plus):
    """An SNV every haplotype carries on a plant under 28 nested ranges, 128 haplotypes over 7
    sites that dirty nothing: nD = 128 x 28 = 3 584 = the small shape's list; plus: one
    haplotype's own site dirties a hit under one range more."""
    lay = Layout("full", 200, 31)
    st8 = strand_of("full", 2)
    lay.plant(st8, 60)
    every = lay.snv(60)
    lay.plant(st8, lay.n - MARGIN - 3)  # under the longest range only (its first base is that range's last)
    lone = lay.snv(lay.n - MARGIN - 3 if plus else 5)
    hi = lay.n - 1 - MARGIN
    lay.ranges = [(MARGIN, hi - 28 - 1 + k) for k in range(27)] + [(MARGIN, hi - 2)]
    sites = [lay.snv(8 + 2 * k) for k in range(7)]
    haps = [(every,) + tuple(sites[i] for i in c) for k in range(8) for c in itertools.combinations(range(7), k)][:127]
    haps.append((every, lone))
    return _spec(name, lay, haps, edge="dirty_listed", side=plus)


def _runs(name, plus):
    """384 haplotypes of 4 one-column runs each (1 536 runs: the small shape's LDS), or one of
    them with 5."""
    def extra(lay, haps, sites):
        if plus:
            haps[-1] = tuple(sites[:5])
        return haps
    return family(name, 384, m_sites=12, sizes=(4,), n_plants=4, n_a=6, seed=41, extra=extra, edge="runs", side=plus)


def _chunks(name, plus):
    """U = 384 (16 packed rows per chunk), 16 ids with a hit under all 32 nested ranges: T = 512
    touched keys = 32 chunks; plus: a 17th id's hit under the longest range only, 33 chunks."""
    lay = Layout("short", 230, 51)
    M = lay.m
    col = M + 4
    for pid in range(1, 17):
        lay.plant(strand_of("short", pid), col)
        col += 9
    hi = lay.n - 1 - M
    assert col < hi - 45
    lay.ranges = [(M, hi - 31 + k) for k in range(32)]
    if plus:
        lay.plant(strand_of("short", 17), hi)  # its first column is the longest range's last
    sites = [lay.snv(hi - 29 + 2 * k) for k in range(10)]
    lone = lay.snv(M + 4 + 7)  # the first plant's last column, one haplotype's
    haps = subsets(sites, 383, range(5)) + [(lone,)]
    return _spec(name, lay, haps, edge="chunks", side=plus)


def _lmax(name, length, U, n_a=300, edge="lmax", **kw):
    """A region whose haplotypes are `length` bases long (no reuse past 1 024 windows: every hit
    is an own hit), a poly-A stretch of n_a bases under the one-column motif and two ranges,
    U haplotypes."""
    lay = Layout("full", length - 2 * MARGIN, 61)
    one = strand_of("full", 1)
    for k in range(n_a):
        lay.plant(one, 1000 + k)
    far = 1000 + n_a + 700
    lay.plant(strand_of("full", 4), far)
    lay.plant(strand_of("full", 7), length - 40)
    lay.ranges = [(MARGIN, lay.n - 1 - MARGIN), (MARGIN, 1000 + n_a + 200)]
    sites = [lay.snv(1000 + 7, "C"), lay.snv(far + 15), lay.snv(far + 2000), lay.snv(length - 9)]
    haps = [tuple(sites[i] for i in c) for k in range(3) for c in itertools.combinations(range(4), k)][:U]
    return _spec(name, lay, haps, edge=edge, side=length if edge == "lmax" else n_a, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    out = [core()]
    for U in (384, 385):
        out.append(family("shape_%d" % U, U, n_a=8, seed=2, edge="shape", side=U))
    for U in (512, 513):  # hap_info's global read (on the small shape under TFBS_KF_BIGU=0)
        out.append(family("haps_%d" % U, U, n_a=8, seed=3, every=True, edge="hap_lds", side=U))
    for U in (256, 257):  # U x nref = 65 536 | 65 792: pairwise | the sorted walk
        out.append(family("walk_%d" % U, U, n_a=250, n_plants=6, merged_len=280, seed=4, edge="walk", side=U))
    out.append(family("walk_big_400_163", 400, n_a=157, n_plants=6, merged_len=280, seed=5, edge="walk", side=163))
    out.append(family("walk_big_400_164", 400, n_a=158, n_plants=6, merged_len=280, seed=5, edge="walk", side=164))
    for U in (256, 257):  # wave 0: 64 | 65 steps
        out.append(family("steps64_%d" % U, U, n_a=58, n_plants=6, seed=6, edge="stepbits", side=U))
    for U in (128, 129):
        out.append(family("steps128_%d" % U, U, n_a=122, n_plants=6, seed=7, every=True, edge="stepbits", side=U))
    for n_a in (250, 251):  # 256 | 257 reference hits: the latter key_fast_kernel's give-up 3
        out.append(family("refs_%d" % (n_a + 6), 9, n_a=n_a, n_plants=6, merged_len=280, seed=8, edge="refs",
                          side=n_a + 6))
    out += [_listed("listed_3584", 0), _listed("listed_3585", 1)]
    out += [_runs("runs_1536", 0), _runs("runs_1537", 1)]
    out += [_chunks("chunks_32", 0), _chunks("chunks_33", 1)]
    for U in (2048, 2049):  # give-up 0
        out.append(family("maxu_%d" % U, U, n_a=8, m_sites=12, sizes=tuple(range(13)), seed=9, edge="max_u", side=U))
    for k in (32, 33):
        out.append(family("inner_%d" % k, 12, n_a=8, seed=10, ranges=nested(k), edge="n_inner", side=k))
    for length, U in ((16319, 3), (16320, 4)):
        out.append(_lmax("lmax_%d" % length, length, U))
    # spill records well below and well above the 8 192 that post_scan_kernel buckets itself: hit
    # lists of 8 entries per wave (TFBS_CAND_CAP=64) under 2 400 and 48 000 own hits
    for n_a in (300, 6000):
        out.append(_lmax("spill_%d" % n_a, 16000, 4, n_a, edge="spill", env={"TFBS_CAND_CAP": "64"}))
    for k in (512, 513):  # K = 16 384 | 16 416 keys: 512 | 513 ids under 32 ranges
        out.append(family("keys_%d" % k, 6, kind="ids%d" % k, n_plants=4, seed=14, ranges=nested(32), edge="keys",
                          side=32 * k))
    # 128 | 136 scan hit lists under TFBS_MFMA_HAPS_PER_BLOCK=4 (16 | 17 groups of 4 haplotypes, 8 lists
    # each: one depth class), behind a region of 3 haplotypes: hap_begin is not group-aligned
    out.append(family("sliced_pad", 2, kind="short", n_plants=2, seed=12, every=True, edge="pad"))
    for U in (61, 62):
        out.append(family("sliced_%d" % U, U, kind="short", n_plants=6, seed=13, edge="lists", side=U,
                          behind="sliced_pad", env={"TFBS_MFMA_HAPS_PER_BLOCK": "4"}))
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def names():
    return [c["name"] for c in cases()]


# The "full" batch's order.  A scan hit list belongs to a group of 64 haplotypes, so regions that
# share a group count each other's listed hits toward the in-LDS | arena decision: the case
# on the list's very limit comes first (128 haplotypes: two whole groups of its own), the small
# regions lie between large ones, and the region with 48 000 own hits between two that take the
# arena by themselves (test_assembly_cases_cpu.py checks that no decision is left open).
FULL_ORDER = ("listed_3584", "shape_384", "lmax_16319", "shape_385", "lmax_16320", "haps_512", "spill_300",
              "haps_513", "inner_32", "walk_256", "inner_33", "walk_257", "core", "walk_big_400_163", "refs_256",
              "walk_big_400_164", "refs_257", "steps64_256", "steps64_257", "steps128_128", "steps128_129",
              "runs_1536", "runs_1537", "listed_3585", "spill_6000", "maxu_2048", "maxu_2049")


def mixed_names(kind="full"):
    """The cases of a pattern set that share one batch: all of them (the "ids" sets have one
    case each: no batch of their own)."""
    names = [c["name"] for c in cases() if c["kind"] == kind]
    if kind == "full":
        assert sorted(names) == sorted(FULL_ORDER)
        return list(FULL_ORDER)
    return names


@functools.lru_cache(maxsize=None)
def oracle(names_key):
    """(keys per region, rows) of the cases named (a tuple) as one batch."""
    specs = [case(n) for n in names_key]
    ps, n, beds, regions = materialize(specs)
    keys, rows, _ = run_oracle(ps, n, beds, regions)
    return keys, rows


# ---------------------------------------------------------------------------------------
# the model: what the assembly sees of a region

def reference_hits(spec):
    """Every (strand, window) whose columns of the reference are the strand's motif."""
    ref, out = spec["ref"], []
    for i, (_, _, L, motif) in enumerate(strands(spec["kind"])):
        at = ref.find(motif)
        while at >= 0:
            out.append((i, at))
            at = ref.find(motif, at + 1)
    return out


def range_bits(spec, w, L, first=0, count=32):
    """The inner ranges [first, first + count) a hit at window w overlaps (its first or its
    last base inside)."""
    return sum(1 for a, b in spec["ranges"][first:first + count] if a <= w <= b or a <= w + L - 1 <= b)


def run_meets(a, b, w, L):
    return a <= w + L - 1 and b >= w


@functools.lru_cache(maxsize=None)
def host_batch(names_key, dedup=True):
    """The host batch of the cases named (no device)."""
    import os
    specs = [case(n) for n in names_key]
    old = os.environ.get("TFBS_DEDUP")
    os.environ["TFBS_DEDUP"] = "1" if dedup else "0"
    try:
        return build_batch(*materialize(specs))
    finally:
        if old is None:
            del os.environ["TFBS_DEDUP"]
        else:
            os.environ["TFBS_DEDUP"] = old


def figures(names_key, r, dedup=True, hpb=64):
    """What the assembly branches on for region r of the batch of the cases named."""
    spec = case(names_key[r])
    st = strands(spec["kind"])
    b = host_batch(names_key, dedup)
    okeys = oracle(names_key)[0][r]
    hb, U, ref_hap, n_inner = b.layout(r)
    assert n_inner == len(spec["ranges"]) and U == len(spec["haps"])
    refs_on = ref_hap is not None
    hits = reference_hits(spec) if refs_on else []
    runs = [b.hap_runs(r, l) for l in range(U)]
    nD = 0
    for reuses, _, rr in runs:
        if not reuses:
            continue
        for i, w in hits:
            L = st[i][2]
            if any(run_meets(a, e, w, L) for a, e in rr):
                nD += range_bits(spec, w, L)
    offs = [(off, off + len(rr)) for reuses, off, rr in runs if reuses]
    nruns = max(e for _, e in offs) - min(o for o, _ in offs) if offs else 0
    # touched keys: the oracle's keys (some haplotype matched) and the reference hits' keys
    es = 10000 + REGION_STEP * r - margin(spec["kind"])
    touched = {(rng, pid) for (_, rng, pid) in okeys}
    for i, w in hits:
        for a, e in spec["ranges"][:32]:
            if a <= w <= e or a <= w + st[i][2] - 1 <= e:
                touched.add(((es + a, es + e), st[i][0]))
    # listed own hits: one entry per (hit, range) of a haplotype's dirty windows -- at most its
    # total count; exactly that without reuse; at least the hits of its dirty windows when it
    # has the reference's columns (SNVs only)
    memb = b.membership(r)
    total = [0] * U
    for (left, right) in okeys.values():
        seen = {}
        for s in range(b.n_samples):
            seen[memb[2 * s]] = left[s]
            seen[memb[2 * s + 1]] = right[s]
        for l, c in seen.items():
            total[l] += c
    lo = hi = 0
    lmax = len(spec["ref"])
    for l in range(U):
        reuses, _, rr = runs[l]
        nucs, pos, _ = b.haplotype(r, l)
        lmax = max(lmax, len(nucs))
        if not reuses:
            lo += total[l]
            hi += total[l]
        elif len(nucs) == len(spec["ref"]) and all(p == es + k for k, p in enumerate(pos)):
            seq, own = "".join(BASES[x] for x in nucs), 0
            for i, (_, _, L, motif) in enumerate(st):
                at = seq.find(motif)
                while at >= 0:
                    if any(run_meets(a, e, at, L) for a, e in rr):
                        own += range_bits(spec, at, L)
                    at = seq.find(motif, at + 1)
            lo += own
            hi += own
        else:  # an indel haplotype: its own columns' runs are not the reference's
            hi += total[l]
    g_lo, g_hi = hb // hpb, (hb + U - 1) // hpb
    return dict(U=U, nref=len(hits), nD=nD, nruns=nruns, T=len(touched), K=n_ids(spec["kind"]) * n_inner,
                n_inner=n_inner, lmax=lmax, ent_lo=lo, ent_hi=hi, groups=g_hi - g_lo + 1, hap_begin=hb,
                refs_on=refs_on)


# TFBS_KEY_COR_LDS / TFBS_KEY_COR_CAP runs: (corrections kept in LDS at most, arena words, the
# give-up they must end in or None) -- the arena full for the corrections (4) and for the
# counters (5), and dirty corrections listed in LDS, then copied from the top of the list to
# an arena with room
CAP_CASES = {"shape_384": (16, 200, 4), "inner_32": (16, 300, 4), "chunks_33": (16, 20000, 5),
             "listed_3584": (16, 100000, None), "walk_257": (16, 100000, None)}


def batch_key(name):
    """The cases of the batch a case is run in (the case last)."""
    c = case(name)
    return ((c["behind"],) if c["behind"] else ()) + (name,)


def predict(f, big_u=BIG_U, fast_max_u=1 << 30, cor_lds=1 << 30, cor_cap=1 << 22, lists_per_group=None,
            others_ent=0):
    """The TFBS_PATH_* word of a region with figures f (tfbs_amd.h), as a dict of bit names
    with None where the figures' bounds leave a bit open, plus "why" (the give-up reason or
    None).  others_ent: listed hits of neighbouring regions' haplotypes in the groups shared
    with them (an upper bound)."""
    P = {k: False for k in T.PATH_BITS}
    why = None
    big = big_u > 0 and f["U"] > big_u
    S = SHAPES["big" if big else "small"]
    P["FAST"], P["BIG"] = True, big
    U, nref = f["U"], f["nref"]

    def finish():
        if why is not None:
            P["GIVEUP"] = True
            P["ASM"] = True
            P["ASM_HAPS"] = U > ASM["haps"]
            P["ASM_RUNS"] = f["nruns"] > ASM["runs"]
            P["ASM_HITS"] = False if f["ent_hi"] <= ASM["hits"] else True if f["ent_lo"] > ASM["hits"] else None
            P["ASM_REFS"] = nref > ASM["refs"]
            P["ASM_SCRATCH"] = U > ASM["counters"]
        P["TICKET"] = None  # (the launch's business: asserted by the ticket tests)
        return P, why

    if U == 0 or f["K"] == 0:
        return finish()
    if U > min(MAX_U, fast_max_u) or f["K"] > MAX_K or f["n_inner"] > MAX_INNER:
        why = 0
        return finish()
    if lists_per_group is not None:
        P["LISTS_SLICED"] = f["groups"] * lists_per_group > S["lists"]
    else:
        P["LISTS_SLICED"] = None
    if f["nruns"] >= 65536:
        why = 2
        return finish()
    P["RUNS_L2"] = f["nruns"] > S["runs"]
    if nref > S["refs"]:
        why = 3
        return finish()
    pairwise = U * nref <= PAIR_LIMIT
    P["WALK"] = not pairwise
    rpl = 1 if nref <= 1 else 64 if nref >= 64 else 1 << (nref - 1).bit_length()
    hpw = 64 // rpl
    n_p = (nref + rpl - 1) // rpl
    waves = S["block"] // 64
    n_l0 = (U + waves * hpw - 1) // (waves * hpw)
    P["STEPBITS"] = pairwise and n_l0 * n_p <= 64
    P["DIRTY_LISTED"] = pairwise and f["nD"] <= S["cor"]
    extra = max(0, nref - REF_LIST) + f["nD"]  # the reference hits past the region's list are spill records
    need_lo, need_hi = f["ent_lo"] + extra, f["ent_hi"] + others_ent + extra
    lim = min(S["cor"], cor_lds)
    P["COR_ARENA"] = False if need_hi <= lim else True if need_lo > lim else None
    used = 0
    if P["COR_ARENA"] is None:
        return finish()  # (a case off its margin: the CPU test refuses it)
    if P["COR_ARENA"]:
        if need_lo > cor_cap:
            why = 4
            return finish()
        if need_hi > cor_cap:
            P["COR_ARENA"] = None
            return finish()
        used = need_hi
    half = 4 * (f["lmax"] + 64) < 65536 and cor_lds != 0
    rows_per = min((2 if half else 1) * S["cnt"] // U, S["rows"])
    if (f["T"] + rows_per - 1) // rows_per > 32 or cor_lds == 0:
        half = False
        P["CNT_ARENA"] = True
        if min(f["T"], S["rows"]) * U > cor_cap - used:
            why = 5
            return finish()
    P["U32"] = not half
    P["HAP_GLOBAL"] = U > S["hap_lds"]
    return finish()


def mixed_predictions(key, lists_per_group, hpb=64, **kw):
    """(figures, predictions) of every region of the batch of the cases `key`.  A region's
    listed own hits are bounded above with those of every other region that has a haplotype in
    one of the haplotype groups (hpb haplotypes, from the batch's first) the region touches:
    the groups' lists are shared."""
    figs = [figures(key, r, hpb=hpb) for r in range(len(key))]
    out = []
    for r, f in enumerate(figs):
        lo = f["hap_begin"] // hpb * hpb
        hi = (f["hap_begin"] + f["U"] - 1) // hpb * hpb + hpb - 1
        others = sum(g["ent_hi"] for q, g in enumerate(figs)
                     if q != r and g["hap_begin"] <= hi and g["hap_begin"] + g["U"] - 1 >= lo)
        out.append(predict(f, lists_per_group=lists_per_group, others_ent=others, **kw))
    return figs, out
