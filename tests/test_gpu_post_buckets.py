"""The spill records' buckets (post_buckets in scan_mfma.hip, read through spill_range in
key_kernels.hip) and the assembly without the post-scan stage.

Region r's records are spill_cnt[r] entries at spill_off[r] of spill_sorted; spill_off[r] means
nothing where the count is 0, the buckets lie in no particular order, and neither array is read
when the scan spilled nothing.  The batches are a handful of regions of a few haplotypes with
TFBS_CAND_CAP=64 (hit lists of 8 entries per wave) forcing the spills; every one is compared
with the oracle's keys, per-sample vectors and rows, from the dense download (key_asm_kernel in
mode 1 after check_overflow's bucketing, whose counts live in an array of their own) and from the
device reduction (post_scan_kernel's buckets, or the wide kernels', read by key_fast_kernel and,
for a region it gives up, key_asm_kernel in mode 0).  Every spilling case asserts its record
count, from the assembly's report, on the intended side of the 8 192 that one workgroup buckets."""
import contextlib
import functools
import os

import pytest

import assembly_cases as A
from helpers import T, build_batch, run_oracle

pytestmark = pytest.mark.gpu

CHROM = "chr1"
SPILL = {"TFBS_CAND_CAP": "64"}
SERIAL = 8192  # kPostSerial


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


def _with_insertion(lay, haps, sites):
    """Six more haplotypes, with an insertion before the first plant: every window behind it is
    dirty, so each of their hits is an own hit (a kind-0 record once its wave's list is full)."""
    ins = lay.insertion(0)
    return haps + [(ins,)] + [(ins, s) for s in sites[:5]]


@functools.lru_cache(maxsize=None)
def _custom():
    """Cases of this file alone: clean regions of 4 haplotypes (a few own hits, nothing past the
    region's 64 reference hits), and refs_257's shape -- 257 reference hits, 193 of them kind-1
    records -- with six haplotypes whose ~250 hits each are their own: both kinds in one region."""
    out = {}
    for k in range(3):
        out["clean_%d" % k] = A.family("clean_%d" % k, 4, n_a=8, seed=70 + k)
    for n_a in (250, 251):  # (256 reference hits: key_fast_kernel's readers; 257: given up, key_asm_kernel's)
        name = "both_%d" % (n_a + 6)
        out[name] = A.family(name, 9, n_a=n_a, n_plants=6, merged_len=280, seed=8, extra=_with_insertion)
    return out


def _case(name):
    return _custom()[name] if name in _custom() else A.case(name)


@functools.lru_cache(maxsize=None)
def _oracle(key):
    """As assembly_cases.oracle, for this file's cases too."""
    specs = [_case(n) for n in key]
    ps, n, beds, regions = A.materialize(specs)
    keys, rows, _ = run_oracle(ps, n, beds, regions)
    return keys, rows


def _batch(key):
    return build_batch(*A.materialize([_case(n) for n in key]))


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
    """A fresh Scanner made and used under env (every test's GPU work runs inside)."""
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


def _dense_and_reduced(sc, key):
    """Both readers of the buckets against the oracle; the reduction's figures."""
    b = _batch(key)
    b.scan(sc)
    _assert_batch(b, key, "dense")
    b = _batch(key)
    b.scan(sc, reduce=True)
    _assert_batch(b, key, "reduce")
    return sc.assembly_figures()


def _steps(sc, key, n):
    """tfbs_step n times on the uploaded batch (the third alike is captured, the next ones replay
    the graph); the figures after each."""
    b = _batch(key)
    T.check(T.lib().tfbs_batch_upload(sc.h, b.h))
    figs = []
    for _ in range(n):
        T.check(T.lib().tfbs_step(sc.h, b.h))
        figs.append(dict(sc.assembly_figures(), **sc.post_figures()))
    T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
    _assert_batch(b, key, "steps")
    return figs


POSITIONS = {"first": ("spill_300", "clean_0", "clean_1"),
             "last": ("clean_0", "clean_1", "spill_300"),
             "two": ("spill_300", "clean_0", "clean_1", "refs_256"),
             "kinds_one_region": ("both_256", "clean_0", "both_257"),
             "kinds_two_regions": ("refs_257", "clean_0", "spill_300")}


@pytest.mark.parametrize("where", sorted(POSITIONS))
def test_records_where_they_fall(where):
    """Records in the first region only, in the last only, in two regions with clean ones
    between, and reference hits past a region's 64 (kind 1: refs_256 keeps them on
    key_fast_kernel, refs_257 -- given up -- on key_asm_kernel) beside own hits (kind 0) in the
    same region and in another.  (A clean region that shares a scan group's lists with a
    spilling one may have its few own hits spilled too.)"""
    key = POSITIONS[where]
    with _scanner(SPILL) as sc:
        fig = _dense_and_reduced(sc, key)
    print(where, fig)
    assert 0 < fig["spill"] <= SERIAL, fig
    if where == "kinds_one_region":  # 192 + 193 reference hits past the regions' lists, and own hits past the waves'
        assert fig["spill"] > 192 + 193 + 300 and fig["left"] == 1, fig
    if where == "kinds_two_regions":  # (spill_300 alone: more than 1 000, test_gpu_assembly_paths.py)
        assert fig["spill"] > 193 + 1000 and fig["left"] == 1, fig


def test_stale_buckets_are_not_read():
    """One ctx: a batch that spills in its first region, then one of as many regions that spills
    only in its last -- whose first region must see none of the earlier records -- and back."""
    x, y = POSITIONS["first"], POSITIONS["last"]
    with _scanner(SPILL) as sc:
        for key in (x, y, x):
            fig = _dense_and_reduced(sc, key)
            assert 0 < fig["spill"] <= SERIAL, fig
        bx, by = _batch(x), _batch(y)
        for b, key in ((bx, x), (by, y), (bx, x), (by, y)):  # the reduction alone, alternating
            b.scan(sc, reduce=True)
            _assert_batch(b, key, "alternating")
            assert 0 < sc.assembly_figures()["spill"] <= SERIAL


SIDES = {"below": (("spill_300",), False), "above": (("spill_6000",), True),
         "both": (("spill_300", "clean_0", "spill_6000"), True)}


@pytest.mark.parametrize("side", sorted(SIDES))
def test_either_side_of_one_workgroup(side):
    """2 400 records (post_scan_kernel's last workgroup), 48 000 (the wide kernels, which leave
    the counts the same way), and both regions in one batch."""
    key, high = SIDES[side]
    with _scanner(SPILL) as sc:
        fig = _dense_and_reduced(sc, key)
        assert (fig["spill"] > SERIAL) == high and fig["spill"] >= 2400 and fig["wide"] == 1, fig
        b = _batch(key)
        for k in range(2):  # the second step lean: post_scan_kernel alone below, the wide kernels above
            b.scan(sc, upload=k == 0, reduce=True)
            _assert_batch(b, key, "second")
        fig = sc.assembly_figures()
        assert (fig["spill"] > SERIAL) == high and fig["wide"] == (1 if high else 0) and fig["reruns"] == 0, fig
        assert sc.post_figures()["left_out"] == 0


TAIL = dict(SIDES, kind1=(("clean_0", "refs_256", "clean_1", "refs_257"), False))


@pytest.mark.parametrize("side", sorted(TAIL))
def test_the_scan_kernels_tail(side):
    """TFBS_POST_FUSE=1: tfbs_step's lean steps bucket in the scan kernel's last workgroup (512
    threads) when the batch's last checked assembly saw at most 8 192 records and no candidate
    past the waves' lists; else the launch.  The kind-1 batch (385 reference hits past the regions'
    lists, wave lists of 1 024 entries: no such candidate) must take the tail from the second step
    on; the others' candidates past their 8-entry lists keep them on the launch."""
    key, high = TAIL[side]
    with _scanner(dict({"TFBS_CAND_CAP": "8192"} if side == "kind1" else SPILL, TFBS_POST_FUSE="1")) as sc:
        figs = _steps(sc, key, 5)
    print(side, figs)
    for k, fig in enumerate(figs):
        assert (fig["spill"] > SERIAL) == high and fig["spill"] >= (385 if side == "kind1" else 1000), fig
        fused = k > 0 and figs[k - 1]["spill"] <= SERIAL and figs[k - 1]["cand"] == 0
        assert fig["fused"] == (1 if fused else 0), (k, fig)
        assert fig["left_out"] == 0, (k, fig)
    if side == "kind1":
        assert [f["fused"] for f in figs] == [0, 1, 1, 1, 1] and figs[-1]["reruns"] == 0, figs


def test_no_stage_after_a_clean_assembly():
    """A batch that spills nothing, five steps (plain, plain, captured, replayed twice): from the
    second on the post-scan stage is left out, nothing reruns, and the results are the oracle's.
    (Wave lists of 1 024 candidates: at the default 128 a wave that happens to take nearly all of
    this one group's pairs from the pool lists a candidate past its own -- seen once, 1 candidate --
    and the next step then rightly keeps the stage.)"""
    key = ("clean_0", "clean_1", "clean_2")
    with _scanner({"TFBS_CAND_CAP": "8192"}) as sc:
        figs = _steps(sc, key, 5)
        launches = T.lib().tfbs_ctx_last_scan_launches(sc.h)
    print(figs)
    assert launches == 1  # (the last step replayed the graph)
    for k, fig in enumerate(figs):
        assert fig["spill"] == 0 and fig["left_out"] == (1 if k > 0 else 0), (k, fig)
        assert fig["reruns"] == 0 and fig["reruns_post"] == 0, (k, fig)


def test_no_stage_every_assembly_in_full():
    """TFBS_ASM_LEAN=0: the stage in every assembly, clean or not."""
    key = ("clean_0", "clean_1", "clean_2")
    with _scanner({"TFBS_ASM_LEAN": "0"}) as sc:
        figs = _steps(sc, key, 3)
    assert [f["left_out"] for f in figs] == [0, 0, 0] and figs[-1]["reruns"] == 0, figs


@pytest.mark.parametrize("key", [("spill_300",), ("clean_0", "both_257", "spill_6000")])
def test_stage_left_out_with_records_reruns_once(key):
    """TFBS_ASM_LEAN=2 on a fresh ctx: the first assembly leaves the stage out, its report shows
    the records, and it runs again in full -- once; the results are the oracle's.  Then the same
    through tfbs_step, whose every step reruns once (a graph's flags are the captured step's, not
    the rerun's)."""
    with _scanner(dict(SPILL, TFBS_ASM_LEAN="2")) as sc:
        b = _batch(key)
        b.scan(sc, reduce=True)
        _assert_batch(b, key, "reduce")
        fig = dict(sc.assembly_figures(), **sc.post_figures())
        assert fig["spill"] > 0 and fig["reruns"] == 1 and fig["reruns_post"] == 1, fig
        assert fig["left_out"] == 0 and fig["wide"] == 1 and fig["leftover"] == 1, fig  # (the rerun's)
        figs = _steps(sc, key, 5)
    print(figs)
    assert [f["reruns_post"] for f in figs] == [2, 3, 4, 5, 6], figs
    assert [f["reruns"] for f in figs] == [2, 3, 4, 5, 6], figs
