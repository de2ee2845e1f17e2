"""The count path of scan_fast_kernel (octet and quad lookup units) and scan_generic_kernel --
several tiles of both unit kinds, the window and haplotype geometry, N and indels, the reduction
paths, the arithmetic edges, the generic kernel, LUT groups between matrix-core groups and a
single-group tile above 64 KiB -- through RegionBatch and tfbs_matches against the plain Python
restatement (lut_ref.py) applied per haplotype id.  The cases and their expected keys are built in
mono_cases.py from the model alone; test_lut_cpu.py checks the model against the oracle and what
makes the cases bite.  Every test asserts from the plan that the path it names is taken.  Integer
work: every comparison is exact."""
import contextlib
import os

import pytest

import dinuc_cases as K
import lut_ref as R
import mono_cases as M
from helpers import T, build_batch

pytestmark = pytest.mark.gpu

MODES = ((False, False), (True, False), (True, True))  # dense download, device reduction, + device encoding
TFBS_E_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@contextlib.contextmanager
def scanner(ps, **env):
    """A Scanner created with the environment variables `env` set (a context reads its settings
    when it is made); they are restored before the scan."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        sc = T.Scanner(ps)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    try:
        yield sc
    finally:
        sc.close()


def check_keys(sc, ps, case, reduce=False, encode=False):
    b = build_batch(ps, case["n"], case["beds"], case["regions"])
    b.scan(sc, reduce=reduce, encode=encode)
    for i, want in enumerate(case["want"]):
        assert b.keys(i) == want, (i, reduce, encode)
    return b


def two_haplotypes(case, region=0):
    """Two distinct haplotypes of a region, those with an indel first."""
    def has_break(sq):
        return any(b != a + 1 for a, b in zip(sq[1], sq[1][1:]))
    return sorted(set(case["seqs"][region]), key=lambda sq: (not has_break(sq), sq))[:2]


def check_matches(sc, case, region=0):
    """tfbs_matches window by window: a failure names a strand and its windows, not a count."""
    for codes, pos in two_haplotypes(case, region):
        got = sc.matches_all([(K.NUC[c], p) for c, p in zip(codes, pos)])
        for i, p in enumerate(case["pats"]):
            assert got[i] == R.matches(p, codes, pos), (i, p)


def all_on_the_lut_path(ps, tile_blocks=20):
    st = ps.plan_stats(tile_blocks, mfma=False)
    assert st["n_mfma_strands"] == 0
    assert st["n_octet_strands"] + st["n_quad_strands"] + st["n_generic_strands"] == len(ps)
    return st


@pytest.mark.parametrize("tile_blocks", [8, 20, 36])
def test_counts_across_tiles_of_both_kinds(tile_blocks):
    """122 strands, a third of them quad: more than 64 slots, tiles holding octet and quad units,
    padded units of both kinds, units of mixed lengths, a five-strand id; keys and rows."""
    case = M.case_tiles()
    ps = T.PatternSet.from_patterns(case["pats"])
    st = all_on_the_lut_path(ps, tile_blocks)
    plan = ps.lut_plan(tile_blocks)
    kinds = [{plan["units"][u]["kind"] for u in range(t["first"], t["last"])} for t in plan["tiles"]]
    assert {R.OCTET, R.QUAD} in kinds and st["n_quad_strands"] >= 30 and st["n_octet_strands"] >= 60
    # (the five-strand id alone needs 16 blocks: under 8 it is a tile of its own, above its share)
    assert st["max_tile_blocks"] <= max(16, tile_blocks) and (tile_blocks != 8 or st["n_fast_tiles"] >= 3)
    want_rows = K.rebuild_rows(case["want"], case["beds"], ps.name_of)
    with scanner(ps, TFBS_MFMA=0, TFBS_TILE_BLOCKS=tile_blocks) as sc:
        for reduce, encode in MODES:
            b = check_keys(sc, ps, case, reduce, encode)
            assert b.rows("chr1", 0)[0] == want_rows, (reduce, encode)


@pytest.mark.parametrize("haps_per_block", [8, None])
def test_counts_window_and_haplotype_geometry(haps_per_block):
    """1 to 513 windows per haplotype for the tile's 1-column strands (chunk and pass edges, the
    three-chunk tail) with strands of 4, 5, 9 and 32 columns in the same tile, haplotypes shorter
    than a strand, and a region of more than 128 distinct haplotypes."""
    case = M.case_geometry()
    ps = T.PatternSet.from_patterns(case["pats"])
    all_on_the_lut_path(ps)
    plan = ps.lut_plan()
    assert len(plan["tiles"]) == 1 and plan["tiles"][0]["lmin"] == 1
    env = {} if haps_per_block is None else {"TFBS_HAPS_PER_BLOCK": haps_per_block}
    with scanner(ps, TFBS_MFMA=0, **env) as sc:
        b = check_keys(sc, ps, case)
        assert b.region_stats(b.num_regions - 1)[0] > 128
        check_keys(sc, ps, case, reduce=True)


def test_counts_n_and_indels():
    """N first and last in a window, at column 31 of a 32-column strand, just past a strand's end, in
    a run and at both ends of the reference, with insertions and deletions, on strands where the
    table (N held as A) and the exact score decide differently in either direction."""
    case = M.case_n_and_indels()
    ps = T.PatternSet.from_patterns(case["pats"])
    all_on_the_lut_path(ps)
    assert case["stats"]["differ_32"] >= 5
    with scanner(ps, TFBS_MFMA=0) as sc:
        for region in range(3):
            check_matches(sc, case, region)
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce, encode)


@pytest.mark.parametrize("key_fast_max_u", [None, 0])
def test_counts_reduction_paths(key_fast_max_u):
    """40, 8 and 9 nested inner ranges (counting passes of 8) and a bed range listed twice, through
    the dense download, the device reduction and the device encoding, with key_fast_kernel and
    (TFBS_KEY_FAST_MAXU=0) without it; keys and rows."""
    case = M.case_reduction()
    ps = T.PatternSet.from_patterns(case["pats"])
    all_on_the_lut_path(ps)
    want_rows = K.rebuild_rows(case["want"], case["beds"], ps.name_of)
    assert want_rows.count("\n") >= 20
    env = {} if key_fast_max_u is None else {"TFBS_KEY_FAST_MAXU": key_fast_max_u}
    with scanner(ps, TFBS_MFMA=0, **env) as sc:
        for reduce, encode in MODES:
            b = check_keys(sc, ps, case, reduce, encode)
            assert b.rows("chr1", 0)[0] == want_rows, (reduce, encode)


def test_arithmetic_edges():
    """Quad sums that wrap int32 under thresholds INT32_MIN, INT32_MAX, an attained score and that
    score minus 1; the octet rule's edges from both sides; the all-lowest (saturating) and
    all-highest window of an octet strand; through tfbs_matches and through a batch."""
    case = M.case_arithmetic()
    ps = T.PatternSet.from_patterns(case["pats"])
    st = all_on_the_lut_path(ps)
    assert st["n_octet_strands"] == 3 and st["n_quad_strands"] == len(ps) - 3
    assert case["stats"]["outside_int32"] >= 5
    with scanner(ps, TFBS_MFMA=0) as sc:
        check_matches(sc, case)
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce, encode)


def test_generic_kernel_counts():
    """Strands of 33 to 100 columns and a pattern_id of 5 and 36 columns in six generic tiles: more
    than 256 windows, 9 inner ranges, N inside long windows, indels, a haplotype shorter than
    most strands."""
    case = M.case_generic()
    ps = T.PatternSet.from_patterns(case["pats"])
    st = ps.plan_stats(mfma=True)
    assert st["n_generic_tiles"] >= 3 and st["n_generic_strands"] == len(ps) and st["n_fast_tiles"] == 0
    assert case["stats"]["differ_long"] >= 5
    with scanner(ps) as sc:
        for region in range(3):
            check_matches(sc, case, region)
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce, encode)


@pytest.mark.parametrize("mfma", [1, 0])
def test_lut_groups_between_matrix_core_groups(mfma):
    """Ids alternately on the matrix cores and on the LUT path (TFBS_MFMA=1): the LUT tile writes its
    dense counts across a slot span that holds matrix-core slots; both kinds of id, and an id with
    a strand of each, give the model's keys, as they do with TFBS_MFMA=0."""
    case = M.case_interleaved()
    ps = T.PatternSet.from_patterns(case["pats"])
    st = ps.plan_stats(mfma=bool(mfma))
    plan = ps.lut_plan(20, bool(mfma))
    if mfma:
        assert st["n_mfma_strands"] == 12 and st["n_octet_strands"] == 1 and st["n_quad_strands"] == 13
        assert plan["slot_mfma"] == [1, 0] * 6 + [0]
        assert any(any(plan["slot_mfma"][t["slot_begin"]:t["slot_begin"] + t["nslots"]]) for t in plan["tiles"])
    else:
        assert st["n_mfma_strands"] == 0 and not any(plan["slot_mfma"])
    with scanner(ps, TFBS_MFMA=mfma) as sc:
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce, encode)


@pytest.mark.parametrize("mfma", [0, 1])
def test_single_group_tile_above_64_kib(mfma):
    """One pattern_id of 32 blocks: a tile of 128 KiB, above a tile's usual share and above the
    64 KiB a kernel gets without the LDS attribute."""
    case = M.case_big_group()
    ps = T.PatternSet.from_patterns(case["pats"])
    st = ps.plan_stats(mfma=bool(mfma))
    assert st["max_tile_blocks"] == 32 and st["max_tile_blocks"] * 4096 > 64 * 1024
    with scanner(ps, TFBS_MFMA=mfma) as sc:
        check_matches(sc, case)
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce, encode)


def test_group_above_the_lds_is_refused():
    """One pattern_id of 48 blocks (192 KiB) is refused when the context is made; nothing is launched."""
    ps = T.PatternSet.from_patterns(M.refused_group())
    assert ps.plan_stats()["max_tile_blocks"] == 48
    with pytest.raises(T.TfbsError) as e:
        with scanner(ps, TFBS_MFMA=0):
            pass
    assert e.value.code == TFBS_E_ARG and "160 KiB" in str(e.value)


@pytest.mark.parametrize("name", ["tiles", "geometry", "n_and_indels", "reduction", "arithmetic", "generic"])
def test_cases_under_the_other_mfma_setting(name):
    """The cases above once more with the matrix cores on (the generic case: off): eligible strands
    leave the LUT path, the keys stay the model's."""
    case = M.CASES[name]()
    ps = T.PatternSet.from_patterns(case["pats"])
    mfma = 0 if name == "generic" else 1
    st = ps.plan_stats(mfma=bool(mfma))
    assert name in ("generic", "arithmetic") or st["n_mfma_strands"] > 0
    with scanner(ps, TFBS_MFMA=mfma) as sc:
        check_keys(sc, ps, case)
        check_keys(sc, ps, case, reduce=True, encode=True)
