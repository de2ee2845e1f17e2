"""Regions that put key_fast_kernel's region body (key_kernels.hip) on the edges of its dirty
test and of its counter chunks, built with assembly_cases' Layout / family and read back with
its figures() / predict().

The dirty test is hit-major: a wave takes 64 haplotypes and a slice of at most 64 reference
hits, a group of GROUP hits at a time; a region whose haplotype blocks fill at most half of the
workgroup's waves (U <= 128 of 256 threads, U <= 512 of 1 024) splits the hits into shares.
The chunks hold rows_per = min(2 x 3 072 / U, 256) rows of packed counters on the common
shape; a wave's rows sit in its lanes, a varying row's slot is a prefix over 64 rows a ballot,
and the rows' keys are built once per region when T <= 256.

Slots stand in id order within one strand length (by longest strand, then id), and a
row is a touched key in key order (slot x ranges + range): in the two-range "ids40" regions rows
2 i and 2 i + 1 are pattern id i + 1."""
import functools

import assembly_cases as A
from helpers import T

GROUP = 8        # hits whose columns a wave holds in scalar registers at a time
ROWS = 256       # s_rkey: the rows whose keys are built once per region
CNT = 3072       # counter words of the common shape

REGISTRY = {}
_case = A.case


def _lookup(name):
    """assembly_cases.case for this module's regions too (figures(), oracle() and host_batch()
    find a region by name)."""
    return REGISTRY[name]() if name in REGISTRY else _case(name)


A.case = _lookup


def _reg(name, fn, *a, **kw):
    REGISTRY[name] = functools.lru_cache(maxsize=None)(functools.partial(fn, name, *a, **kw))


# ------------------------------------------------------------------------------ the dirty test
def _hits(name, n, fill=0):
    """n reference hits of the one-column motif side by side, every one of them dirty for exactly
    one haplotype: min(n, 16) haplotypes carry the SNVs of a block of neighbouring hits each (one
    run), beside the reference.  A hit that is left out of the test shows in a key.  fill: that
    many haplotypes more, over SNVs that dirty nothing (one wave then meets more than 64 hits)."""
    lay = A.Layout("full", max(200, n + 80), 300 + n)
    one = A.strand_of("full", 1)
    c0 = lay.free(A.MARGIN + 4, n + 1)
    for k in range(n):
        lay.plant(one, c0 + k)
    sites = [lay.snv(c0 + k, "C") for k in range(n)]
    blank = lay.snv(c0 + n + 8)  # (n = 0: a haplotype that dirties nothing)
    nh = max(1, min(n, 16))
    per = (n + nh - 1) // nh if n else 0
    haps = [()] + [tuple(sites[i * per:(i + 1) * per]) or (blank,) for i in range(nh) if n == 0 or sites[i * per:(i + 1) * per]]
    if fill:
        blanks = [lay.snv(c0 + n + 12 + 2 * k) for k in range(10)]
        haps += A.subsets(blanks, fill, range(1, 7))
    lay.ranges = [(lay.m, lay.n - 1 - lay.m), (lay.m, c0 + n // 2)]  # a hit under 2 ranges or 1
    return A._spec(name, lay, haps)


HIT_COUNTS = (0, 1, GROUP - 1, GROUP, GROUP + 1, 63, 64, 65, 128, 256)
for _n in HIT_COUNTS:
    _reg("hits%d" % _n, _hits, _n)
# 70 hits and 3 | 9 haplotype blocks: no hit shares on 4 | 16 waves, a second slice of 6 hits
WIDE = {"hits70_u140": 125, "hits70_u520": 505}
for _name, _fill in WIDE.items():
    _reg(_name, _hits, 70, _fill)

U_COUNTS = (1, 63, 64, 65, 128, 129, 257, 512, 513)  # 128 | 129 and 512 | 513: the hit shares' edge
for _u in U_COUNTS:
    _reg("u%d" % _u, A.family, _u, n_a=8, n_plants=6, seed=2)

RUN_COUNTS = (1, GROUP - 1, GROUP + 1, 16)  # (0 runs: the reference haplotype of every region)
for _k in RUN_COUNTS:
    _reg("runs%d" % _k, A.family, 7, m_sites=18, sizes=(_k,), n_a=8, n_plants=4, seed=41)


def _between(lay, haps, sites):
    haps[2] = tuple(sites[:17])  # 17 runs: no reuse
    return haps


_reg("between", A.family, 5, m_sites=18, sizes=(1,), n_a=8, n_plants=4, seed=42, extra=_between)
for _k in (1, 2, 32):
    _reg("inner%d" % _k, A.family, 12, n_a=8, seed=10, ranges=A.nested(_k))

DIRTY_BATCHES = {
    "hits": tuple("hits%d" % n for n in HIT_COUNTS) + tuple(WIDE),
    "haps": tuple("u%d" % u for u in U_COUNTS),
    # core: a run on a window's first column only and on its last only, for every strand length;
    # listed_3585: one dirty correction more than the top of the list holds (the second pass)
    "misc": tuple("runs%d" % k for k in RUN_COUNTS) + ("between", "inner1", "inner2", "inner32", "core", "listed_3585"),
}


# --------------------------------------------------------------------------------- the chunks
def _rows(name, U, full_ids, last_bits):
    """T = 32 x full_ids + last_bits rows: full_ids ids with a hit under all 32 nested ranges, one
    more id's hit under the last_bits longest ranges; U haplotypes, one of which breaks the first
    plant (its 32 rows vary)."""
    lay = A.Layout("short", 230, 51 + U)
    M = lay.m
    hi = lay.n - 1 - M
    col = M + 4
    for pid in range(1, full_ids + 1):
        lay.plant(A.strand_of("short", pid), col)
        col += 10
    assert col < hi - 45
    lay.ranges = [(M, hi - 31 + k) for k in range(32)]
    if last_bits:  # window hi - 31 + j lies under the 32 - j ranges that end at or behind it
        lay.plant(A.strand_of("short", full_ids + 1), hi - 31 + (32 - last_bits))
    lone = lay.snv(M + 4 + 7)
    sites = [lay.snv(col + 2 + 2 * k) for k in range(8)]
    haps = A.subsets(sites, U - 1, range(5)) + [(lone,)]
    return A._spec(name, lay, haps)


# rows_per = 2 x 3 072 / 48 = 128: one row less, as many, one more; 256 | 257 rows: the keys once | per chunk
for _t, (_u, _f, _b) in {127: (48, 3, 31), 128: (48, 4, 0), 129: (48, 4, 1), 256: (24, 8, 0), 257: (24, 8, 1)}.items():
    _reg("rows%d" % _t, _rows, _u, _f, _b)
for _u in (1, 2, 3):
    _reg("few%d" % _u, A.family, _u, kind="short", n_plants=6, seed=13 + _u)

N_IDS = 40  # (x 17 columns: the region stays below the 1 024 columns of reference-window reuse)
KIND_IDS = "ids%d" % N_IDS


def _special(name, U, breakers, every_on=()):
    """Two nested ranges over every id's one plant: rows 2 i and 2 i + 1 are id i + 1.  breakers:
    {id: the haplotypes (indices of the region's list; -1: the last) that break its hit}; "rest":
    all but the reference haplotype.
    every_on: ids whose hit every haplotype breaks (an SNV all carry: no reference haplotype, the
    hit's row cancels to 0)."""
    lay = A.Layout(KIND_IDS, 17 * N_IDS + 40, 70 + U)
    M = lay.m
    col, first = M + 2, {}
    for pid in range(1, N_IDS + 1):
        lay.plant(A.strand_of(KIND_IDS, pid), col)
        first[pid] = col
        col += 17
    lay.ranges = [(M, lay.n - 1 - M), (M, lay.n - 2 - M)]
    base = tuple(lay.snv(first[pid] + 15) for pid in every_on)
    filler = [lay.snv(col + 2 + 2 * k) for k in range(8)]  # (they dirty nothing: distinct haplotypes)
    haps = [set(h) for h in A.subsets(filler, U, range(5))]
    for pid, who in breakers.items():
        v = lay.snv(first[pid] + 15)
        for l in (range(1, U) if who == "rest" else [w % U for w in who]):
            haps[l].add(v)
    return A._spec(name, lay, [base + tuple(sorted(h)) for h in haps])


# a hit that only the reference haplotype keeps (the last distinct haplotype: they stand in the order
# of their first record) | that one other haplotype breaks, in the first and the last rows of the
# chunk, the other way round in edge_b; the ids between: equal and not 0
_reg("edge_a", _special, 9, {1: "rest", 2: [-1], N_IDS - 1: "rest", N_IDS: [-1]})
_reg("edge_b", _special, 10, {1: [-1], 2: "rest", N_IDS - 1: [-1], N_IDS: "rest"})
# the first and the last id's rows cancel to 0 on every haplotype, id 20's vary, the rest equal and not 0
_reg("cancel", _special, 6, {20: [2]}, every_on=(1, N_IDS))
# varying rows 63 | 64 | 65 (ids 32, 33, 33): every id varies, the odd ones (33), the even ones (32)
_reg("vary_all", _special, 5, {pid: [1 + pid % 3] for pid in range(1, N_IDS + 1)})
_reg("vary_ids_odd", _special, 5, {pid: [1 + pid % 3] for pid in range(1, N_IDS + 1, 2)})
_reg("vary_ids_even", _special, 4, {pid: [1 + pid % 2] for pid in range(2, N_IDS + 1, 2)})

CHUNK_BATCHES = {
    "rows": ("rows127", "rows128", "rows129", "rows256", "rows257", "few1", "few2", "few3"),
    "special": ("edge_a", "edge_b", "cancel", "vary_all", "vary_ids_odd", "vary_ids_even"),
}
BATCHES = dict(DIRTY_BATCHES, **CHUNK_BATCHES)


def hap_counts(key, r):
    """{oracle key: [count of each distinct haplotype]} of region r of the batch `key`."""
    b = A.host_batch(key)
    memb = b.membership(r)
    U = b.layout(r)[1]
    out = {}
    for k, (left, right) in A.oracle(key)[0][r].items():
        c = [None] * U
        for s in range(b.n_samples):
            c[memb[2 * s]] = left[s]
            c[memb[2 * s + 1]] = right[s]
        out[k] = c
    return out


def rows_per(U):
    return min(2 * CNT // U, ROWS)
