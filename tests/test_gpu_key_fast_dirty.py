"""key_fast_kernel's dirty test and its region body by placement (key_kernels.hip), at the sizes
where they can go wrong.

The pairwise dirty test gives every haplotype a lane: the lane walks its diff runs once over 64
reference hits at a time and keeps the dirty ones as a 64-bit mask, from which it counts and
lists its corrections.  So the edges are lanes (U = 1, 63, 64, 65 haplotypes: a wave's last lane
and the first of the next; 256, 257: the workgroup's last thread and a second round) and mask
bits (0, 1, 63, 64, 65 reference hits: bit 63, and a second slice of one hit, which reaches the
region through a spill record: its list holds 64).  Every plant of these regions has an SNV on
its first column (a run [a, a] with w == b: dirty) and one on its last (w + L - 1 == a: dirty),
each carried by a haplotype of its own, and plants stand back to back in pairs, so the same
runs miss the neighbour by one column (clean); whatever order the kernel keeps the reference
hits in, a planted hit at bit 63 or bit 62 is dirty for a haplotype for which every other hit is
clean (two of the 63 to 65 hits lie across the seam of a pair: no SNV of their own).

The region body is compiled twice -- corrections, runs and packed u16 counters in LDS, and any
other placement -- and a persistent workgroup passes from one region to the next, so one batch
under TFBS_KF_GRID=3 holds regions of every placement behind one another.

The cases are assembly_cases.family() regions; their figures and the path word they must
report come from assembly_cases.figures / predict, which look a case up by name: the module's
own cases are served to them through assembly_cases.case for the module's duration."""
import contextlib
import itertools
import os

import pytest

import assembly_cases as A
from helpers import T, build_batch

pytestmark = pytest.mark.gpu

CHROM = "chr1"
OWN = {}
_case_before = A.case


def _case(name):
    return OWN[name] if name in OWN else _case_before(name)


@pytest.fixture(scope="module", autouse=True)
def own_cases():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")
    A.case = _case
    yield
    A.case = _case_before


def _blank_sites(lay, n):
    col = max([w for _, w in lay.plants] + [lay.m]) + 12
    out = []
    for _ in range(n):
        col = lay.free(col, 1)
        out.append(lay.snv(col))
        lay.used[col] = True
        col += 2  # (not adjacent: one run each)
    return out


def _edge_haps(U, how="mixed"):
    """family()'s `extra`: an SNV on the first and on the last column of every plant, 10 blank
    sites, and U haplotypes: the reference, one per plant SNV (one run, one dirty hit), then
    distinct subsets of the blank sites, every second one with a plant SNV too.
    how = "all": every haplotype carries every plant's first-column SNV; "none": no haplotype
    carries a plant SNV; "runs16": the second haplotype carries the first 16 plants' SNVs."""
    def extra(lay, haps, sites):
        L = A.strands(lay.kind)[0][2]
        first = [lay.snv(w) for _, w in lay.plants]
        last = [lay.snv(w + L - 1) for _, w in lay.plants]
        blank = _blank_sites(lay, 10)
        combos = [c for k in range(1, 11) for c in itertools.combinations(blank, k)]
        if how == "all":
            return ([tuple(first)] + [tuple(first) + c for c in combos])[:U]
        if how == "none":
            return ([()] + combos)[:U]
        out = [()]
        if how == "runs16":
            out.append(tuple(first[:16]))
        out += [(s,) for s in first + last]  # (the first-column SNVs first: with U > plants every hit has one)
        plant = first + last
        for i, c in enumerate(combos):
            out.append(c + ((plant[i % len(plant)],) if plant and i % 2 else ()))
        return out[:U]
    return extra


def _short(name, U, n_plants, how="mixed", seed=170, **kw):
    OWN[name] = A.family(name, 1, kind="short", n_plants=n_plants, m_sites=1, sizes=(0,), seed=seed,
                         merged_len=10 * n_plants + 60, ranges=A.nested(2), extra=_edge_haps(U, how), **kw)
    return name


def _full_1_32(name):
    """The "full" set: four one-column hits (AAAA, SNVs on its middle columns) and a plant of 32
    columns with an SNV on its first and one on its last column."""
    def extra(lay, haps, sites):
        st = A.strand_of("full", 7)
        w = lay.free(160, 36) + 2
        lay.plant(st, w)
        return haps + [(lay.snv(w),), (lay.snv(w + 31),)]
    OWN[name] = A.family(name, 20, kind="full", n_a=4, n_plants=4, m_sites=6, sizes=(0, 1, 2), seed=91,
                         merged_len=260, ranges=A.nested(2), extra=extra)
    return name


# lanes: U at 6 reference hits; mask bits: reference hits at 65 haplotypes (a full wave and one lane).
# Back-to-back plants of the "short" set make two more hits across their seam: 61, 62 and 63 plants
# are 63, 64 and 65 reference hits (the test asserts the count)
LANES = [_short("kfd_u%d" % U, U, 6) for U in (1, 63, 64, 65, 256)]
BITS = [_short("kfd_ref%d" % n, 65, p) for n, p in ((0, 0), (1, 1), (63, 61), (64, 62), (65, 63))]
OTHERS = [_short("kfd_all_dirty", 64, 3, "all"), _short("kfd_none_dirty", 64, 6, "none"),
          _short("kfd_runs16", 40, 16, "runs16"), _full_1_32("kfd_full_1_32")]
U257 = _short("kfd_u257", 257, 6)
# the hand-over batch ("full" set), in the launch's order (most haplotypes first): diff runs in
# global memory; two regions whose corrections exceed TFBS_KEY_COR_LDS; three small ones (the last
# shares a haplotype group, and so its hit lists, with lmax_16320's 2 405 own hits); u32 counters
_full = dict(kind="full", ranges=A.nested(2))
for _name, _U, _kw in (("kfd_arena_a", 150, dict(n_a=40, n_plants=6, merged_len=260)),
                       ("kfd_arena_b", 90, dict(n_a=40, n_plants=6, merged_len=260)),
                       ("kfd_lds_a", 30, dict(n_a=6, n_plants=4)), ("kfd_lds_b", 26, dict(n_a=6, n_plants=4)),
                       ("kfd_lds_c", 24, dict(n_a=6, n_plants=4))):
    OWN[_name] = A.family(_name, _U, seed=92, **_kw, **_full)
HANDOVER = ("runs_1537", "kfd_arena_a", "kfd_arena_b", "kfd_lds_a", "kfd_lds_b", "kfd_lds_c", "lmax_16320")
HANDOVER_COR_LDS = 250


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def scanner():
    """One tracing Scanner per (pattern set, environment)."""
    made = {}

    def get(kind, env):
        key = (kind, tuple(sorted(env.items())))
        if key not in made:
            with _env(dict(env, TFBS_MFMA="1")):
                made[key] = T.Scanner(A.pattern_set(kind))
            made[key].assembly_trace(True)
        return made[key]

    yield get
    for sc in made.values():
        sc.close()


def _lists_per_group(kind):
    return 8 * A.pattern_set(kind).plan_stats(mfma=True)["n_mfma_supers"]


def _assert_word(word, P, why, ctx):
    for name, want in P.items():
        if want is not None:
            assert bool(word & T.PATH_BITS[name]) == want, (name, hex(word), ctx)
    assert why is None and not word & T.PATH_BITS["GIVEUP"], (hex(word), ctx)


def _run(key, env, scanner, **kw):
    """The batch of the cases `key`: the reduction's keys, per-sample vectors and rows against
    the oracle's, each region's path word against predict; returns (figures, words)."""
    specs = [A.case(n) for n in key]
    okeys, orows = A.oracle(key)
    sc = scanner(specs[0]["kind"], env)
    with _env(env):
        b = build_batch(*A.materialize(specs))
        b.scan(sc, reduce=True)
    assert b.num_regions == len(okeys)
    for i, want in enumerate(okeys):
        got = b.keys(i)
        assert got.keys() == want.keys(), (key[i], i)
        for k in want:
            assert got[k] == want[k], (key[i], i, k)
    assert b.rows(CHROM)[0] == orows
    words = b.assembly_paths(sc)
    figs, preds = A.mixed_predictions(key, _lists_per_group(specs[0]["kind"]), **kw)
    for r, (P, why) in enumerate(preds):
        print(key[r], hex(words[r]), figs[r])
        _assert_word(words[r], P, why, (key[r], figs[r]))
    assert sc.assembly_figures()["left"] == 0
    return figs, words


@pytest.mark.parametrize("name", LANES + BITS + OTHERS)
def test_lanes_and_mask_bits(name, scanner):
    (f,), (word,) = _run((name,), {}, scanner)
    assert f["U"] * f["nref"] <= A.PAIR_LIMIT and not word & T.PATH_BITS["WALK"]
    assert f["refs_on"] == (name != "kfd_u1")  # (one haplotype: the reference itself, nothing to reuse)
    want = dict(kfd_ref0=0, kfd_ref1=1, kfd_ref63=63, kfd_ref64=64, kfd_ref65=65).get(name)
    assert want is None or f["nref"] == want, f
    if name.startswith("kfd_u"):
        assert f["U"] == int(name[5:]), f
    if name == "kfd_all_dirty":  # every (haplotype, hit, range) triple
        assert f["nD"] == f["U"] * sum(A.range_bits(A.case(name), w, 8) for _, w in A.reference_hits(A.case(name)))
    if name == "kfd_none_dirty":
        assert f["nD"] == 0 and f["nref"] == 6, f
    if name == "kfd_runs16":  # the longest run list a reusing haplotype has, beside lists of one run
        b = A.host_batch((name,))
        assert sorted({len(b.hap_runs(0, l)[2]) for l in range(f["U"]) if b.hap_runs(0, l)[0]})[-1] == 16


@pytest.mark.parametrize("big_u", ["1024", "1"])
def test_second_round_of_lanes(big_u, scanner):
    """257 haplotypes: thread 0's second haplotype on the common shape (which takes the region
    whatever TFBS_KF_BIGU says above 257), and the same body as the big shape's under 1."""
    (f,), (word,) = _run((U257,), {"TFBS_KF_BIGU": big_u}, scanner, big_u=int(big_u))
    assert f["U"] == 257 and bool(word & T.PATH_BITS["BIG"]) == (big_u == "1")


def test_three_in_one_batch(scanner):
    """Regions of 65, 64 and 1 haplotypes side by side (their lists in shared haplotype groups)."""
    _run(("kfd_ref65", "kfd_u64", "kfd_u1"), {}, scanner)


def test_placement_hand_over(scanner):
    """TFBS_KF_GRID=3: three persistent workgroups over seven regions of the common shape.  The
    first three (runs from global memory, corrections in the arena twice) take the general body;
    whichever workgroup takes the first ticket passes from there to a region with everything in
    LDS and packed counters, and one passes on to u32 counters: s_ncor, s_arena and the top of
    s_cor of the region before must not reach the next."""
    env = {"TFBS_KF_GRID": "3", "TFBS_KEY_COR_LDS": str(HANDOVER_COR_LDS)}
    figs, words = _run(HANDOVER, env, scanner, cor_lds=HANDOVER_COR_LDS)
    bit = T.PATH_BITS
    assert sorted(range(len(figs)), key=lambda r: -figs[r]["U"]) == list(range(len(figs)))  # (the launch's order)
    seen = [tuple(bool(w & bit[k]) for k in ("RUNS_L2", "COR_ARENA", "U32", "CNT_ARENA")) for w in words]
    assert seen[0][0] and not any(s[0] for s in seen[1:]), seen
    assert seen[1][1:] == seen[2][1:] == (True, False, False), seen
    assert seen[3] == seen[4] == (False, False, False, False), seen
    assert seen[6][2], seen
    assert not any(w & bit["BIG"] for w in words)
    assert sum(1 for w in words if w & bit["TICKET"]) == len(words) - 3
