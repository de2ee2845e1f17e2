"""Spill records read in place (AsmArgs::spill_inplace): a lean assembly leaves the post-scan
stage out after a checked assembly that saw no candidate past the waves' lists and at most
TFBS_SPILL_INPLACE records, and its kernels -- key_fast_kernel on both shapes, key_asm_kernel --
take the records from the scan's own list, every region's workgroup keeping those whose region
word (bit 31, the kind, masked) is its own.

The stage is left out only without an overflow candidate, and TFBS_CAND_CAP=64 (candidate lists of
8 entries per wave) overflows them on every batch here, records or not (929 candidates on three
clean regions): that capacity is the overflow case, where the stage must run.  The other cases
take the capacities at which the records appear without such a candidate: 8 192 for the reference
hits past a region's 64 (kind 1, whatever the capacity), and TFBS_SHARE=0 (hit lists as short as
the candidate lists) under 32 nested ranges, a hit of which is 32 pairs, for the own hits (kind
0).  Every case compares keys, per-sample vectors and rows with the oracle and reads the mode and
the reruns from tfbs_ctx_post_figures."""
import contextlib
import functools
import itertools
import os

import pytest

import assembly_cases as A
from helpers import T, build_batch, run_oracle

pytestmark = pytest.mark.gpu

CHROM = "chr1"
KIND1 = {"TFBS_CAND_CAP": "8192"}                       # reference hits past a region's 64 only
KIND0 = {"TFBS_CAND_CAP": "2048", "TFBS_SHARE": "0"}    # own hits past a wave's list, no candidate past its own
BOTH = {"TFBS_CAND_CAP": "8192", "TFBS_SHARE": "0"}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


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


def _many_insertions(count):
    """count more haplotypes that share an insertion before the first plant (every window behind
    it is dirty: their hits are their own) and differ in the sites behind it."""
    def extra(lay, haps, sites):
        ins = lay.insertion(0)
        more = [(ins,) + tuple(sites[i] for i in c) for k in range(len(sites) + 1)
                for c in itertools.combinations(range(len(sites)), k)]
        return haps + more[:count]
    return extra


@functools.lru_cache(maxsize=None)
def _cases():
    out = {}
    for k in range(3):
        out["clean_%d" % k] = A.family("clean_%d" % k, 4, n_a=8, seed=70 + k)
    for n in (65, 100):  # 1 | 36 reference hits past the region's list: kind-1 records, and no other
        out["refs_%d" % n] = A.family("refs_%d" % n, 9, n_a=n - 6, n_plants=6, merged_len=280, seed=8)
    # own hits under 32 nested ranges, 6 haplotypes behind an insertion: kind-0 records alone
    out["own"] = A.family("own", 4, n_a=8, m_sites=6, ranges=A.nested(32), extra=_many_insertions(6), seed=112)
    # refs_100's reference hits and 24 haplotypes behind an insertion under 32 ranges: both kinds in one region
    out["both"] = A.family("both", 9, n_a=94, n_plants=6, merged_len=280, seed=8, ranges=A.nested(32),
                           extra=_many_insertions(24))
    # the same with 48 and with 40 such haplotypes and other reference hits: about 1 000 records
    # each, so that the three together hold well over 2 048 (3 000; two alone gave 2 020 to 2 045)
    out["both_b"] = A.family("both_b", 9, n_a=90, n_plants=6, merged_len=280, seed=9, ranges=A.nested(32),
                             extra=_many_insertions(48))
    out["both_c"] = A.family("both_c", 9, n_a=92, n_plants=6, merged_len=280, seed=10, ranges=A.nested(32),
                             extra=_many_insertions(40))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(key):
    ps, n, beds, regions = A.materialize([_cases()[n] for n in key])
    keys, rows, _ = run_oracle(ps, n, beds, regions)
    return keys, rows


def _batch(key):
    return build_batch(*A.materialize([_cases()[n] for n in key]))


def _assert_batch(b, key, what):
    okeys, orows = _oracle(key)
    assert b.num_regions == len(okeys)
    for i, want in enumerate(okeys):
        got = b.keys(i)
        assert got.keys() == want.keys(), (what, key[i])
        for k in want:
            assert got[k] == want[k], (what, key[i], k)
    assert b.rows(CHROM)[0] == orows, what


HIP_ERROR = []  # a HIP error ends the module's GPU work: nothing more is launched after one


@contextlib.contextmanager
def _scanner(env):
    if HIP_ERROR:
        pytest.fail("not run: an earlier test met a HIP error (%s)" % HIP_ERROR[0])
    try:
        with _env(dict(env, TFBS_MFMA="1")):
            sc = T.Scanner(A.pattern_set("full"))
        try:
            with _env(env):
                yield sc
        finally:
            sc.close()
    except AssertionError:
        raise
    except Exception as e:
        if "hip" in str(e).lower():
            HIP_ERROR.append(str(e))
        raise


def _steps(sc, key, n, dense=False):
    """tfbs_step n times on the uploaded batch (the third alike is captured and replayed), the
    figures after each; then the dense download (key_asm_kernel over every region, the same
    records) and the reduction's download, each against the oracle."""
    b = _batch(key)
    T.check(T.lib().tfbs_batch_upload(sc.h, b.h))
    figs = []
    for _ in range(n):
        T.check(T.lib().tfbs_step(sc.h, b.h))
        figs.append(dict(sc.assembly_figures(), **sc.post_figures()))
    if dense:
        T.check(T.lib().tfbs_batch_download(sc.h, b.h))
        _assert_batch(b, key, "dense after the steps")
    T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
    _assert_batch(b, key, "steps")
    return figs


def _in_place_from_the_second(figs, records=None):
    """records: the exact count (reference hits past the lists: the same in every step), or None
    for own hits, whose split between the waves' lists and the records moves with the pool."""
    for k, fig in enumerate(figs):
        assert fig["cand"] == 0, (k, fig)
        assert fig["spill"] == records if records is not None else 0 < fig["spill"] <= 8192, (k, fig)
        # (after an assembly without a record none is read in place: a record then means a rerun)
        assert (fig["left_out"], fig["in_place"]) == ((1, 1 if records != 0 else 0) if k else (0, 0)), (k, fig)
        assert fig["reruns"] == 0 and fig["reruns_post"] == 0, (k, fig)


WHERE = {"none": (("clean_0", "clean_1", "clean_2"), KIND1, 0),
         "one_record": (("clean_0", "refs_65", "clean_1"), KIND1, 1),
         "first": (("refs_100", "clean_0", "clean_1"), KIND1, 36),
         "middle": (("clean_0", "refs_100", "clean_1"), KIND1, 36),
         "last": (("clean_0", "clean_1", "refs_100"), KIND1, 36),
         "two_regions": (("refs_100", "clean_0", "refs_65"), KIND1, 37)}


@pytest.mark.parametrize("where", sorted(WHERE))
def test_reference_hit_records_where_they_fall(where):
    """No record, one, and 36 in the first, a middle and the last region only -- regions whose only
    records are reference hits (bit 31 of the region word) -- over three steps: the first in full,
    the next two without the stage, the last a replayed graph."""
    key, env, records = WHERE[where]
    with _scanner(env) as sc:
        figs = _steps(sc, key, 3, dense=True)
    print(where, figs)
    _in_place_from_the_second(figs, records)


def test_own_hit_records():
    """Kind-0 records alone (own hits past a wave's hit list), beside clean regions."""
    key = ("clean_0", "own", "clean_1")
    with _scanner(KIND0) as sc:
        figs = _steps(sc, key, 3, dense=True)
    print(figs)
    _in_place_from_the_second(figs)


READERS = {"small_shape": {}, "big_shape": {"TFBS_KF_BIGU": "1"}, "key_asm": {"TFBS_KEY_FAST_MAXU": "0"}}


@pytest.mark.parametrize("reader", sorted(READERS))
def test_both_kinds_in_one_region_every_reader(reader):
    """A region with reference-hit records and own-hit records (more than 1 000 together), a
    kind-1 region and a clean one: key_fast_kernel's common shape, its 1 024-thread shape
    (TFBS_KF_BIGU=1) and key_asm_kernel's list pass (TFBS_KEY_FAST_MAXU=0: every region given up)."""
    key = ("both", "clean_0", "refs_100")
    with _scanner(dict(BOTH, **READERS[reader])) as sc:
        figs = _steps(sc, key, 3, dense=True)
    print(reader, figs)
    assert min(f["spill"] for f in figs) > 1000 + 36
    _in_place_from_the_second(figs)
    if reader == "key_asm":
        assert figs[-1]["left"] == 3, figs


@pytest.mark.parametrize("reader", sorted(READERS))
def test_more_records_than_the_front_round(reader):
    """More than 2 048 records: key_fast_kernel's threads take the first 2 048 with the front's
    loads and the others in rounds of their own; three regions with both kinds, so that either part
    holds records of several regions."""
    key = ("both", "both_c", "clean_0", "both_b")
    with _scanner(dict(BOTH, **READERS[reader])) as sc:
        figs = _steps(sc, key, 3, dense=True)
    print(reader, figs)
    assert min(f["spill"] for f in figs) > 2048, figs
    _in_place_from_the_second(figs)


@pytest.mark.parametrize("limit, reruns", [(36, 0), (35, 1)])
def test_exactly_the_limit_and_one_below(limit, reruns):
    """36 records.  TFBS_ASM_LEAN=2 leaves the stage out of a fresh ctx's first assembly: with
    TFBS_SPILL_INPLACE=36 it reads them in place and stands; with 35 it read one too few, its
    report shows 36, and it runs again in full -- once."""
    key = ("clean_0", "refs_100", "clean_1")
    with _scanner(dict(KIND1, TFBS_ASM_LEAN="2", TFBS_SPILL_INPLACE=str(limit))) as sc:
        b = _batch(key)
        b.scan(sc, reduce=True)
        _assert_batch(b, key, "reduce")
        fig = dict(sc.assembly_figures(), **sc.post_figures())
    print(limit, fig)
    assert fig["spill"] == 36 and fig["cand"] == 0, fig
    assert fig["reruns"] == reruns and fig["reruns_post"] == reruns, fig
    assert (fig["left_out"], fig["in_place"]) == ((0, 0) if reruns else (1, 1)), fig


def test_an_overflow_candidate_keeps_the_stage():
    """TFBS_CAND_CAP=64: candidates past the waves' 8-entry lists beside the records.  The stage
    rescores them, so it runs in every step."""
    key = ("both", "clean_0", "refs_100")
    with _scanner({"TFBS_CAND_CAP": "64"}) as sc:
        figs = _steps(sc, key, 3)
    print(figs)
    for fig in figs:
        assert fig["cand"] > 0 and fig["spill"] > 0 and fig["left_out"] == 0 and fig["in_place"] == 0, fig
        assert fig["reruns"] == 0, fig


def test_a_second_batch_with_fewer_records():
    """One ctx: 1 000 records in the first region, then a batch of as many regions with 36 in its
    last -- the scan's list still holds the first batch's records behind them, which a stale count
    would read --, and back."""
    x, y = ("both", "clean_0", "clean_1"), ("clean_0", "clean_1", "refs_100")
    with _scanner(BOTH) as sc:
        for key in (x, y, x):
            figs = _steps(sc, key, 3)
            print(key, figs)
            assert all(f["spill"] > 1000 for f in figs) if key is x else True
            _in_place_from_the_second(figs, 36 if key is y else None)


def test_the_parents_rule():
    """TFBS_SPILL_INPLACE=0: records keep the stage, in every step; no record leaves it out from
    the second step on and nothing is read in place."""
    with _scanner(dict(KIND1, TFBS_SPILL_INPLACE="0")) as sc:
        figs = _steps(sc, ("clean_0", "refs_100", "clean_1"), 3)
        clean = _steps(sc, ("clean_0", "clean_1", "clean_2"), 3)
    print(figs, clean)
    for fig in figs:
        assert fig["spill"] == 36 and (fig["left_out"], fig["in_place"], fig["reruns"]) == (0, 0, 0), fig
    for k, fig in enumerate(clean):
        assert fig["spill"] == 0 and (fig["left_out"], fig["in_place"], fig["reruns"]) == (1 if k else 0, 0, 0), fig
