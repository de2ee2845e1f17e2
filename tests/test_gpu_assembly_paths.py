"""The key assembly (key_fast_kernel, key_asm_kernel; key_kernels.hip) on each of its limits,
on assembly_cases.py's cases (test_assembly_cases_cpu.py shows with the oracle and the host
batch alone that each sits on its edge): the two workgroup shapes at 384 | 385 haplotypes, the
descriptors past LDS at 512 | 513, pairwise | walk at U x nref = 65 536, the step bits of wave 0
at 64 | 65 steps, the dirty corrections' list at 3 584 | 3 585, the diff runs at 1 536 | 1 537,
256 | 257 reference hits, 32 | 33 counter chunks, 128 | 136 scan hit lists, packed | u32
counters at 16 319 | 16 320 bases, the give-ups at 2 048 | 2 049 haplotypes, 32 | 33 inner
ranges and a full arena, tickets under TFBS_KF_GRID=3 and none under TFBS_KF_PERSIST=0.

For every case and mode the oracle's keys, per-sample vectors and rows equal the product's
from the dense download (key_asm_kernel, mode 1) and from the device reduction, and the
reduction's path word (tfbs_batch_assembly_paths) equals what assembly_cases.predict gives
the CPU-proven figures: no case passes on a branch it was not built for.  The last test
asserts that every bit of the report was seen both set and clear."""
import contextlib
import os

import pytest

import assembly_cases as A
from helpers import T, build_batch

pytestmark = pytest.mark.gpu

CHROM = "chr1"
MODES = {"default": ({}, {}),
         "bigu1": ({"TFBS_KF_BIGU": "1"}, dict(big_u=1)),
         "maxu0": ({"TFBS_KEY_FAST_MAXU": "0"}, dict(fast_max_u=0)),
         "corlds0": ({"TFBS_KEY_COR_LDS": "0"}, dict(cor_lds=0)),
         "share0": ({"TFBS_SHARE": "0"}, {}),
         "dedup0": ({"TFBS_DEDUP": "0"}, {})}
SEEN = {}  # bit name -> the values seen (and "why" -> the give-up reasons)
FED = set()  # the tests that fed SEEN (test_every_bit_was_seen_set_and_clear needs them all)
FEEDERS = {"test_case_vs_oracle", "test_one_shape_for_all", "test_arena_limits", "test_mixed_batch",
           "test_lean_assemblies"}
# never set: key_asm_kernel's scratch counters need more than 6 144 distinct haplotypes in one
# region (3 073 samples, past the suite's sizes); never clear: every region of a reduction
# passes key_fast_kernel first
ONE_VALUE = {"ASM_SCRATCH": {False}, "FAST": {True}}


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


@pytest.fixture(scope="module")
def scanner():
    """One tracing Scanner per (pattern set, environment), shared by the module's tests."""
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


def _assert_keys(b, okeys):
    assert b.num_regions == len(okeys)
    for i, want in enumerate(okeys):
        got = b.keys(i)
        assert got.keys() == want.keys(), i
        for k in want:
            assert got[k] == want[k], (i, k)


def _note(words):
    for w in words:
        for name, bit in T.PATH_BITS.items():
            SEEN.setdefault(name, set()).add(bool(w & bit))
        if w & T.PATH_BITS["GIVEUP"]:
            SEEN.setdefault("why", set()).add(T.path_why(w))


def _assert_word(word, P, why, ctx):
    for name, want in P.items():
        if want is not None:
            assert bool(word & T.PATH_BITS[name]) == want, (name, hex(word), ctx)
    if why is not None:
        assert T.path_why(word) == why, (hex(word), ctx)


HIP_ERROR = []  # a HIP error ends the module's GPU work: nothing more is launched after one


@contextlib.contextmanager
def _guard():
    """Every test's GPU work runs inside: not started after a HIP error, which it records."""
    if HIP_ERROR:
        pytest.fail("not run: an earlier test met a HIP error (%s)" % HIP_ERROR[0])
    try:
        yield
    except AssertionError:
        raise
    except Exception as e:
        if "hip" in str(e).lower():
            HIP_ERROR.append(str(e))
        raise


def _run(key, env, scanner, dense=True):
    """The batch of the cases `key` under env: keys and rows from the dense download and the
    reduction against the oracle; returns the reduced batch, its scanner and its path words."""
    with _guard():
        out = _run_checked(key, env, scanner, dense)
    FED.add(os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split("[")[0].split(" ")[0])
    return out


def _run_checked(key, env, scanner, dense):
    specs = [A.case(n) for n in key]
    okeys, orows = A.oracle(key)
    sc = scanner(specs[0]["kind"], env)
    with _env(env):
        if dense:
            b = build_batch(*A.materialize(specs))
            b.scan(sc)
            _assert_keys(b, okeys)
            assert b.rows(CHROM)[0] == orows, "dense"
        b = build_batch(*A.materialize(specs))
        b.scan(sc, reduce=True)
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows, "reduce"
    words = b.assembly_paths(sc)
    _note(words)
    return b, sc, words


def _lists_per_group(kind):
    return 8 * A.pattern_set(kind).plan_stats(mfma=True)["n_mfma_supers"]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [n for n in A.names() if A.case(n)["edge"] != "pad"])
def test_case_vs_oracle(name, mode, scanner):
    c = A.case(name)
    env, kw = MODES[mode]
    env = dict(env, **c["env"])
    key = A.batch_key(name)
    r = len(key) - 1
    b, sc, words = _run(key, env, scanner)
    f = A.figures(key, r, dedup=mode != "dedup0", hpb=int(env.get("TFBS_MFMA_HAPS_PER_BLOCK", 64)))
    P, why = A.predict(f, lists_per_group=_lists_per_group(c["kind"]), **kw)
    print(name, mode, hex(words[r]), f)
    _assert_word(words[r], P, why, (name, mode, f))
    assert not words[r] & T.PATH_BITS["TICKET"]  # one region: no ticket
    fig = sc.assembly_figures()
    hpb = int(env.get("TFBS_MFMA_HAPS_PER_BLOCK", 64))
    left = [A.predict(A.figures(key, q, dedup=mode != "dedup0", hpb=hpb), **kw)[1] for q in range(len(key))]
    assert fig["left"] == sum(1 for w in left if w is not None), fig
    if c["edge"] == "spill":  # the side of post_scan_kernel's 8 192 records, from the report
        assert (fig["spill"] > 8192) == (c["side"] == 6000) and fig["spill"] > 1000, fig
        assert fig["reruns_wide"] == 0  # (no lean assembly here: the wide kernels were never missed)


@pytest.mark.parametrize("name", ["haps_512", "haps_513"])
def test_one_shape_for_all(name, scanner):
    """TFBS_KF_BIGU=0: every region on the small shape, whose LDS holds 512 haplotypes'
    descriptors; the others' are read again."""
    key = (name,)
    b, sc, words = _run(key, {"TFBS_KF_BIGU": "0"}, scanner)
    f = A.figures(key, 0)
    P, why = A.predict(f, big_u=0, lists_per_group=_lists_per_group("full"))
    assert not P["BIG"] and P["HAP_GLOBAL"] == (name == "haps_513") and why is None
    _assert_word(words[0], P, why, (name, f))


@pytest.mark.parametrize("name", sorted(A.CAP_CASES))
def test_arena_limits(name, scanner):
    """TFBS_KEY_COR_LDS=16 sends the corrections to an arena of TFBS_KEY_COR_CAP words: full for
    the corrections (give-up 4) or for the counter chunks (5), or large enough (dirty
    corrections listed at the top of the LDS list are copied over)."""
    lds, cap, want = A.CAP_CASES[name]
    key = (name,)
    b, sc, words = _run(key, {"TFBS_KEY_COR_LDS": str(lds), "TFBS_KEY_COR_CAP": str(cap)}, scanner)
    f = A.figures(key, 0)
    P, why = A.predict(f, cor_lds=lds, cor_cap=cap, lists_per_group=_lists_per_group(A.case(name)["kind"]))
    assert why == want
    _assert_word(words[0], P, why, (name, f))
    fig = sc.assembly_figures()
    assert (fig["arena"] > cap) == (want is not None), fig


@pytest.fixture(scope="module")
def mixed_key():
    return tuple(A.mixed_names("full"))


@pytest.mark.parametrize("kind", ["full", "short"])
@pytest.mark.parametrize("mode", ["default", "grid3", "persist0"])
def test_mixed_batch(mode, kind, scanner):
    """Every case of a pattern set as a region of one batch (lists, runs and arena shares next to
    neighbours'; the "ids" sets have one case each), with the persistent grids capped at 3
    workgroups per shape (the regions past the first 3 of a shape take tickets) and with one
    workgroup per region."""
    mixed_key = tuple(A.mixed_names(kind))
    env = {"grid3": {"TFBS_KF_GRID": "3"}, "persist0": {"TFBS_KF_PERSIST": "0"}}.get(mode, {})
    b, sc, words = _run(mixed_key, env, scanner, dense=mode == "default")
    figs, preds = A.mixed_predictions(mixed_key, _lists_per_group(kind))
    n_big = sum(1 for f in figs if f["U"] > A.BIG_U)
    n_small = len(figs) - n_big
    for r, (P, why) in enumerate(preds):
        _assert_word(words[r], P, why, (mixed_key[r], mode, figs[r]))
    tickets = sum(1 for w in words if w & T.PATH_BITS["TICKET"])
    assert tickets == (max(0, n_big - 3) + max(0, n_small - 3) if mode == "grid3" else 0)
    assert sc.assembly_figures()["left"] == sum(1 for _, why in preds if why is not None)


def test_second_step_on_the_same_ctx(mixed_key, scanner):
    """A second scan + reduce of the resident batch (the predicted-lean step: the first one's
    leftover regions make it launch the leftover pass again) gives the same words."""
    specs = [A.case(n) for n in mixed_key]
    okeys, orows = A.oracle(mixed_key)
    with _guard():
        sc = scanner("full", {})
        b = build_batch(*A.materialize(specs))
        b.scan(sc, reduce=True)
        first = b.assembly_paths(sc)
        b.scan(sc, upload=False, reduce=True)
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows
    assert b.assembly_paths(sc) == first
    assert sc.assembly_figures()["reruns"] == 0


@pytest.mark.parametrize("lean", ["0", "1", "2"])
@pytest.mark.parametrize("key", [("spill_300", "inner_33"), ("spill_6000",)])
def test_lean_assemblies(key, lean, scanner):
    """TFBS_ASM_LEAN: 0 every assembly in full; 1 the second step of a batch leaves out what the
    first did not need; 2 every assembly lean -- one that then needed the wide spill kernels
    (more than 8 192 records) or the leftover pass (a region key_fast_kernel gave up) must be
    seen to run again in full."""
    env = {"TFBS_ASM_LEAN": lean, "TFBS_CAND_CAP": "64"}
    okeys, orows = A.oracle(key)
    b, sc, words = _run(key, env, scanner, dense=False)
    high = key == ("spill_6000",)
    fig = sc.assembly_figures()
    assert (fig["spill"] > 8192) == high and fig["left"] == (0 if high else 1), fig
    # the first assembly of a batch under 0 / 1, the full rerun under 2: nothing left out
    assert fig["wide"] == 1 and fig["leftover"] == 1, fig
    why, other = ("reruns_wide", "reruns_leftover") if high else ("reruns_leftover", "reruns_wide")
    if lean == "2":
        assert fig["reruns"] >= 1 and fig[why] >= 1, fig
    before = fig
    with _guard(), _env(env):
        b.scan(sc, upload=False, reduce=True)  # the second step on the same ctx
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows
    assert b.assembly_paths(sc) == words
    fig = sc.assembly_figures()
    assert fig["reruns"] - before["reruns"] == fig[why] - before[why] == (1 if lean == "2" else 0), (before, fig)
    # the side of the 8 192 records, from the device flag's reruns: 2 400 records never miss the wide
    # kernels, the batch without a give-up never the leftover pass
    assert fig[other] == before[other], (before, fig)
    # predicted: the wide kernels again for the many records, the leftover pass again for the
    # region given up -- each batch leaves out the other
    assert (fig["wide"], fig["leftover"]) == ((1, 1) if lean != "1" else (1, 0) if high else (0, 1)), fig


@pytest.mark.parametrize("key", [("spill_300", "inner_33"), ("spill_6000",), "mixed"])
def test_step_graph_replays(key, mixed_key):
    """tfbs_step five times on a ctx without the trace (the third alike is captured, the next
    replays the graph: one launch), then the reduction's download: the oracle's keys and rows."""
    key = mixed_key if key == "mixed" else key
    specs = [A.case(n) for n in key]
    env = dict(specs[0]["env"], TFBS_MFMA="1")
    okeys, orows = A.oracle(key)
    with _guard(), _env(env):
        sc = T.Scanner(A.pattern_set("full"))
        try:
            b = build_batch(*A.materialize(specs))
            T.check(T.lib().tfbs_batch_upload(sc.h, b.h))
            for _ in range(5):
                T.check(T.lib().tfbs_step(sc.h, b.h))
            assert T.lib().tfbs_ctx_last_scan_launches(sc.h) == 1
            T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
            _assert_keys(b, okeys)
            assert b.rows(CHROM)[0] == orows
        finally:
            sc.close()


def test_trace_is_off_by_default_and_never_reads_stale_words(scanner):
    """Off: a state error.  Turned on after the last assembly, on a ctx that traced a larger batch
    before: a state error too, not that batch's words; the next assembly's words are the batch's."""
    with _guard(), _env({"TFBS_MFMA": "1"}):
        sc = T.Scanner(A.pattern_set("full"))
        try:
            b = build_batch(*A.materialize([A.case("core")]))
            b.scan(sc, reduce=True)
            with pytest.raises(T.TfbsError, match="assembly trace is off"):
                b.assembly_paths(sc)
            assert sc.assembly_figures()["left"] == 0
            sc.assembly_trace(True)
            two = build_batch(*A.materialize([A.case("refs_257"), A.case("core")]))
            two.scan(sc, reduce=True)
            assert [bool(w & T.PATH_BITS["GIVEUP"]) for w in two.assembly_paths(sc)] == [True, False]
            sc.assembly_trace(False)
            b.scan(sc, reduce=True)
            sc.assembly_trace(True)
            with pytest.raises(T.TfbsError, match="before the assembly trace was turned on"):
                b.assembly_paths(sc)
            b.scan(sc, upload=False, reduce=True)
            (word,) = b.assembly_paths(sc)
            assert word & T.PATH_BITS["FAST"] and not word & T.PATH_BITS["GIVEUP"]
        finally:
            sc.close()


def test_every_bit_was_seen_set_and_clear():
    """(Last in the module.)  Over the tests above each bit of the report was set for some
    region and clear for another -- but the two of ONE_VALUE -- and key_fast_kernel gave up for
    the shape (0), the reference hits (3) and the arena (4, 5); reason 2 (65 536 staged runs)
    has no input: the span is at most 2 048 x 32 - 16 = 65 520."""
    if FED != FEEDERS or HIP_ERROR:
        pytest.fail("needs the whole module run in one process: its words come from %s (ran: %s)%s"
                    % (sorted(FEEDERS), sorted(FED), "; a HIP error ended the GPU work" if HIP_ERROR else ""))
    wrong = {name: SEEN.get(name) for name in T.PATH_BITS if SEEN.get(name) != ONE_VALUE.get(name, {False, True})}
    assert not wrong
    assert SEEN["why"] == {0, 3, 4, 5}
