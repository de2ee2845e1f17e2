"""The count path of scan_dinuc_kernel -- several tiles, the window and haplotype geometry, N
and indels with true pair weights, the reduction paths, the arithmetic edges and all four scan
kernels in one set -- through RegionBatch against the plain Python restatement (dinuc_ref.py)
applied per haplotype id.  The cases and their expected keys are built in dinuc_cases.py from
the reference alone; test_dinuc_cpu.py checks what makes them bite.  Integer work: every
comparison is exact."""
import contextlib
import os

import pytest

import dinuc_cases as K
import dinuc_ref as D
from helpers import T, build_batch

pytestmark = pytest.mark.gpu

MODES = ((False, False), (True, False), (True, True))  # dense download, device reduction, + device encoding


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


def scan_keys(sc, ps, case, reduce=False, encode=False):
    b = build_batch(ps, case["n"], case["beds"], case["regions"])
    b.scan(sc, reduce=reduce, encode=encode)
    return b, [b.keys(i) for i in range(b.num_regions)]


def check_keys(sc, ps, case, **kw):
    b, got = scan_keys(sc, ps, case, **kw)
    for i, want in enumerate(case["want"]):
        assert got[i] == want, (i, kw)
    return b


def test_counts_across_tiles():
    """122 strands in three or more tiles: ids of 2-3 bases with one and two strands filling more
    than a tile's 64 slots, two-strand ids of 32 bases, and a five-strand id of 4, 4, 7, 31 and
    32 bases; the slot order (longest strand, then id) is not the id order, which the rows keep."""
    case = K.case_tiles()
    ps = T.PatternSet.from_patterns(case["pats"])
    assert ps.dinuc_stats()["n_tiles"] >= 3
    with scanner(ps) as sc:
        b = check_keys(sc, ps, case)
        rows, _ = b.rows("chr1", 0)
        assert rows == K.rebuild_rows(case["want"], case["beds"], ps.name_of)
        check_keys(sc, ps, case, reduce=True)


@pytest.mark.parametrize("haps_per_block", [8, None])
def test_counts_window_and_haplotype_geometry(haps_per_block):
    """1, 63, 64, 65, 128, 129, 191, 192, 193, 256 and 257 windows per haplotype (chunk and pass
    edges, the three-chunk tail) with several distinct haplotypes per region, and a region with
    more than 128 distinct haplotypes; a workgroup takes 8 haplotypes, then the default 128."""
    env = {} if haps_per_block is None else {"TFBS_HAPS_PER_BLOCK": haps_per_block}
    for case in (K.case_geometry(), K.case_many_haplotypes()):
        ps = T.PatternSet.from_patterns(case["pats"])
        with scanner(ps, **env) as sc:
            b = check_keys(sc, ps, case)
            assert b.num_haplotypes > 128
            check_keys(sc, ps, case, reduce=True)


def test_counts_n_and_indels_with_pair_weights():
    """N (a run of 3, single, at both ends of the reference) together with insertions of 3 and
    deletions of 5 bases, one running to the last base of the extended range, under weights
    that depend on both bases of every pair."""
    case = K.case_n_and_indels()
    ps = T.PatternSet.from_patterns(case["pats"])
    with scanner(ps) as sc:
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce=reduce, encode=encode)


@pytest.mark.parametrize("key_fast_max_u", [None, 0])
@pytest.mark.parametrize("with_mono", [False, True])
def test_counts_reduction_paths(with_mono, key_fast_max_u):
    """40 nested inner ranges (five counting passes) and a bed range listed twice, through the
    dense download, the device reduction and the device encoding, with key_fast_kernel and
    (TFBS_KEY_FAST_MAXU=0) key_asm_kernel; keys and rows, the rows rebuilt from the reference's
    keys (test_dinuc_cpu.py shows the rebuilding gives the oracle's rows on a mono set)."""
    case = K.case_reduction()
    pats = (case["mono"] if with_mono else []) + case["pats"]
    ps = T.PatternSet.from_patterns(pats)
    want = [dict(w) for w in case["want"]]
    if with_mono:
        for w, m in zip(want, case["mono_keys"]):
            w.update(m)
    want_rows = K.rebuild_rows(want, case["beds"], ps.name_of)
    assert want_rows.count("\n") >= 20
    env = {} if key_fast_max_u is None else {"TFBS_KEY_FAST_MAXU": key_fast_max_u}
    with scanner(ps, **env) as sc:
        for reduce, encode in MODES:
            b, got = scan_keys(sc, ps, case, reduce=reduce, encode=encode)
            assert got == want, (reduce, encode)
            assert b.rows("chr1", 0)[0] == want_rows, (reduce, encode)


def test_arithmetic_edges():
    """Sums that wrap in int32 under thresholds INT32_MIN (every score but INT32_MIN hits),
    INT32_MAX (nothing hits, as for a padding strand), an attained score and that score minus 1,
    through tfbs_matches and through a batch."""
    case = K.case_wrap()
    ps = T.PatternSet.from_patterns(case["pats"])
    reg = case["regions"][0]
    with scanner(ps) as sc:
        for codes, pos in sorted(set(case["seqs"][0]))[:2]:
            got = sc.matches_all([(K.NUC[c], p) for c, p in zip(codes, pos)])
            for i, p in enumerate(case["pats"]):
                assert got[i] == D.matches(p.weights, p.min_score, codes, pos), (i, len(p), p.min_score)
        assert len(reg["ref"]) > 64
        for reduce, encode in MODES:
            check_keys(sc, ps, case, reduce=reduce, encode=encode)


@pytest.mark.parametrize("mfma", [0, 1])
def test_all_four_kernels_in_one_set(mfma):
    """Matrix-core, quad-LUT and generic (36 columns) mono PWMs with dinucleotide PWMs whose ids
    lie below, between and above the mono ids, on regions with indels: the mono keys are the
    oracle's, the dinucleotide keys the reference's, the rows ascend by pattern_id within
    every inner range although the dinucleotide slots come last."""
    case = K.case_all_kernels()
    pats = sorted(case["mono"] + case["pats"], key=lambda p: p.pattern_id)
    ps = T.PatternSet.from_patterns(pats)
    st = ps.plan_stats(mfma=bool(mfma))
    assert (st["n_mfma_strands"] > 0) == bool(mfma) and st["n_quad_strands"] > 0 and st["n_generic_strands"] > 0
    assert mfma or st["n_octet_strands"] > 0
    assert ps.dinuc_stats()["n_strands"] == len(case["pats"])
    di_ids = {p.pattern_id for p in case["pats"]}
    both = [dict(w) for w in case["want"]]
    for w, m in zip(both, case["mono_keys"]):
        w.update(m)
    want_rows = K.rebuild_rows(both, case["beds"], ps.name_of)
    pid_of = {p.name: p.pattern_id for p in pats}
    with scanner(ps, TFBS_MFMA=mfma) as sc:
        for reduce, encode in MODES:
            b, got = scan_keys(sc, ps, case, reduce=reduce, encode=encode)
            assert [{k: v for k, v in g.items() if k[2] not in di_ids} for g in got] == case["mono_keys"]
            assert [{k: v for k, v in g.items() if k[2] in di_ids} for g in got] == case["want"]
            rows = b.rows("chr1", 0)[0]
            assert rows == want_rows, (reduce, encode)
            prev, seen_di = None, 0
            for line in rows.splitlines():
                bed, name, rng = line.split("\t")[2].split(",")
                cur = (rng, bed, pid_of[name])
                assert prev is None or prev[:2] != cur[:2] or prev[2] < cur[2], line
                seen_di += cur[2] in di_ids
                prev = cur
            assert seen_di >= 10
