"""key_fast_kernel's front (key_kernels.hip): the static records made at upload
(region_asm_kernel, window_lists.hip; tfbs_ctx_region_asm) and the two rounds of loads that read
them, and the persistent grid's tickets past regions that leave before either round.

Every run: the oracle's keys and rows from the device reduction, the same digests under
TFBS_KEY_FAST_MAXU=0 (key_asm_kernel does everything and reads no record), the records against
values computed here from the host batch (tfbs_batch_region_layout, tfbs_batch_region_hap_runs,
tfbs_batch_region_haplotype), and the path words the case was built for.

Cases: regions with and without a reusing haplotype, the only reusing one first | last, an
indel haplotype first (run0 behind its own-column list), no reference haplotype, a helper
reference longer than every haplotype; U = 1, 64, 65, 256, 257, 384, 385, 512, 513 on the
default shapes, all on the small one and all on the big one; 97 | 96 haplotypes of 16 runs
(1 552 | 1 536 staged runs) and a region without a run beside reference hits; 0, 1, 63, 64, 65
reference hits, the 65th through the spill list, and a second step without the post-scan
stage; 9 regions with one without keys, one given up on its shape and one on its reference
hits in the middle, under 1, 2, 3 persistent workgroups and one workgroup per region; replayed
steps, another batch on the same ctx and back, and a batch after the one-haplotype upload."""
import contextlib
import functools
import os
import random

import numpy as np
import pytest

import assembly_cases as A
import reuse_cases as K
from helpers import T, build_batch, run_oracle

pytestmark = pytest.mark.gpu

CHROM = "chr1"
NONE = 0xFFFFFFFF
BIT = T.PATH_BITS


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
    """One tracing Scanner per (pattern set, environment): the knobs are read when it is made."""
    made = {}

    def get(ps, env):
        key = (id(ps), tuple(sorted(env.items())))
        if key not in made:
            with _env(dict(env, TFBS_MFMA="1")):
                made[key] = T.Scanner(ps)
            made[key].assembly_trace(True)
        return made[key]

    yield get
    for sc in made.values():
        sc.close()


# ------------------------------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def u_spec(U, n_a=8, n_plants=6, seed=2, **kw):
    return A.family("front_u%d_a%d_p%d" % (U, n_a, n_plants), U, n_a=n_a, n_plants=n_plants, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def runs_spec(U):
    """U haplotypes of 16 one-column runs each: 16 of 18 sites."""
    return A.family("front_runs_%d" % U, U, m_sites=18, sizes=(16,), n_plants=4, n_a=6, seed=41)


@functools.lru_cache(maxsize=None)
def nokeys_spec():
    """A region without an inner range: no key (key_fast_kernel leaves at once)."""
    return A.family("front_nokeys", 4, n_a=4, seed=5, ranges=lambda lay: [])


@functools.lru_cache(maxsize=None)
def case_batch(names):
    """(pattern set, samples, beds, regions, oracle keys, oracle rows) of the specs named: the
    oracle runs once per batch, its result shared by every mode."""
    specs = [SPECS[n]() for n in names]
    ps, n, beds, regions = A.materialize(specs)
    keys, rows, _ = run_oracle(ps, n, beds, regions)
    return ps, n, beds, regions, keys, rows


SPECS = {"u%d" % U: functools.partial(u_spec, U) for U in (1, 64, 65, 256, 257, 384, 385, 512, 513)}
SPECS.update({"runs97": functools.partial(runs_spec, 97), "runs96": functools.partial(runs_spec, 96),
              "nokeys": nokeys_spec, "u128": functools.partial(u_spec, 128),
              "refs257": functools.partial(u_spec, 9, 251, 6, 8, merged_len=280)})
for _k in (0, 1, 63, 64, 65):  # the reference hits: _k one-column 'A' plants and nothing else
    SPECS["refs%d" % _k] = functools.partial(u_spec, 5, _k, 0, 20 + _k)
for _i in range(6):
    SPECS["small%d" % _i] = functools.partial(u_spec, 3 + 5 * _i, 4, 2, 30 + _i)


def _snvs(ref, first, count=17):
    return [K.record(ref, first + 2 * t, "snv", None) for t in range(count)]


@functools.lru_cache(maxsize=None)
def record_batch():
    """Regions over reuse_cases' window (4 samples: ids 0-7) that put the records on their edges."""
    ref = K.base_ref()
    rnd = random.Random(77)
    a17, b17 = _snvs(ref, 4), _snvs(ref, 41)  # 17 runs each: no reuse
    # (distinct haplotypes stand in the order of their first record)
    early, one = K.record(ref, 2, "snv", None), K.record(ref, 90, "snv", None)
    rest = [3, 4, 5, 6, 7]
    regs = [
        # nobody reuses (two haplotypes of 17 runs, every id on one of them)
        K.region("no_reuse", 0, ref, [[x] for x in a17] + [[x] for x in b17],
                 carriers=[[0, 1, 2, 3]] * 17 + [[4, 5, 6, 7]] * 17),
        # the only reusing haplotype is the first (id 0), the others have 17 runs
        K.region("first_reuses", 1, ref, [[early]] + [[x] for x in a17] + [[x] for x in b17],
                 carriers=[[0]] + [[1, 2]] * 17 + [rest] * 17),
        # ... is the last (U - 1)
        K.region("last_reuses", 2, ref, [[x] for x in a17] + [[x] for x in b17] + [[one]],
                 carriers=[[0, 1]] * 17 + [[2, 3, 4, 5, 6]] * 17 + [[7]]),
        # an insertion on the first haplotype: its reference-column list lies behind its own
        K.region("first_indel", 3, ref, [[K.record(ref, 30, "ins3", rnd)], [K.record(ref, 60, "snv", rnd)]],
                 carriers=[[0], [1, 2]]),
        # every id deletes three bases: the reference is the helper haplotype and the longest
        K.region("all_delete", 4, ref, [[K.record(ref, 44, "del3", rnd)], [K.record(ref, 20, "snv", rnd)],
                                         [K.record(ref, 80, "snv", rnd)]],
                 carriers=[list(range(8)), [1, 2], [2, 3]]),
    ]
    # 1 025 columns: nobody reuses and the region has no reference haplotype
    longer = K.base_ref(1025, K.SEED + 3)
    regs.append(K.region("len_1025", 5, longer, [[K.record(longer, 500, "ins1", rnd)], [K.record(longer, 300, "snv", rnd)]]))
    # assembly_cases' literal motifs over reuse_cases' window (the same margin of 31 columns): a few
    # dozen reference hits of the one-column motif, within key_fast_kernel's 256
    ps = A.pattern_set("full")
    assert A.margin("full") == K.LMAX - 1
    beds = K.beds(regs)
    keys, rows, _ = run_oracle(ps, 4, beds, regs)
    return ps, 4, beds, tuple(regs), keys, rows


# ----------------------------------------------------------------------------------- the checks
def host_records(b, regions):
    """(region_asm, hap_reuse) as the upload must make them, from the host batch alone."""
    ra, hr = [], {}
    for r, reg in enumerate(regions):
        hb, U, ref_hap, _ = b.layout(r)
        runs = [b.hap_runs(r, l) for l in range(U)]
        offs = [(off, off + len(rr)) for reuses, off, rr in runs if reuses]
        run0 = min(o for o, _ in offs) if offs else NONE
        nruns = max(e for _, e in offs) - run0 if offs else 0
        lens = [len(b.haplotype(r, l)[0]) for l in range(U)]
        if ref_hap is not None:  # the reference group's haplotype or the helper copy: the reference
            lens.append(len(reg["ref"]))
        ra.append((run0, nruns, max(lens) if lens else 0, 0))
        for l, (reuses, off, rr) in enumerate(runs):
            hr[hb + l] = ((off - run0) | (len(rr) << 16)) if reuses else NONE
    return ra, hr


def assert_records(b, sc, regions):
    got_ra, got_hr = sc.region_asm()
    want_ra, want_hr = host_records(b, regions)
    assert got_ra == want_ra
    assert len(got_hr) >= max(want_hr, default=-1) + 1
    for h, x in enumerate(got_hr):  # (a helper reference haplotype: in no region's count, no reuse)
        assert x == want_hr.get(h, NONE), (h, hex(x))
    return want_ra


def _assert_keys(b, okeys):
    assert b.num_regions == len(okeys)
    for i, want in enumerate(okeys):
        assert b.keys(i) == want, i


def run(batch, env, scanner, steps=1):
    """The batch reduced on the device under env: oracle keys and rows, the records, and the same
    digests from key_asm_kernel alone; returns (batch, scanner, path words, region_asm)."""
    ps, n, beds, regions, okeys, orows = batch
    sc = scanner(ps, env)
    with _env(env):
        b = build_batch(ps, n, beds, list(regions))
        b.scan(sc, reduce=True)
        for _ in range(steps - 1):
            b.scan(sc, upload=False, reduce=True)
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows
    words = b.assembly_paths(sc)
    ra = assert_records(b, sc, regions)
    assert_same_without_key_fast(b, batch, env, scanner)
    return b, sc, words, ra


def assert_same_without_key_fast(b, batch, env, scanner):
    """The batch again under TFBS_KEY_FAST_MAXU=0 -- every region with a key through
    key_asm_kernel, which reads no record --: the same key and row digests as b's."""
    ps, n, beds, regions = batch[:4]
    env0 = dict(env, TFBS_KEY_FAST_MAXU="0")
    sc0 = scanner(ps, env0)
    with _env(env0):
        b0 = build_batch(ps, n, beds, list(regions))
        b0.scan(sc0, reduce=True)
    for x, y in zip(b.region_digests(), b0.region_digests()):
        assert np.array_equal(x, y)
    for r, w in enumerate(b0.assembly_paths(sc0)):
        assert bool(w & BIT["ASM"]) == (b.layout(r)[1] != 0 and b.layout(r)[3] != 0), (r, hex(w))


# ------------------------------------------------------------------------------------ the tests
def test_records_against_the_host(scanner):
    batch = record_batch()
    b, sc, words, ra = run(batch, {}, scanner)
    regions = batch[3]
    name = {reg["name"]: r for r, reg in enumerate(regions)}
    reuses = lambda r: [b.hap_runs(r, l)[0] for l in range(b.layout(r)[1])]
    # the cases are what they are said to be
    assert not any(reuses(name["no_reuse"])) and ra[name["no_reuse"]][:2] == (NONE, 0)
    f = reuses(name["first_reuses"])
    assert f[0] and not any(f[1:]) and len(f) == 3
    f = reuses(name["last_reuses"])
    assert f[-1] and not any(f[:-1]) and len(f) == 3
    r = name["first_indel"]
    own, rq = b.hap_own_runs(r, 0), b.hap_runs(r, 0)
    assert own[0] and rq[1] == own[1] + len(own[2]) and len(own[2]) > 0  # a list of its own, in front
    assert ra[r][0] == rq[1]                                             # run0 lies behind it
    r = name["all_delete"]
    hb, U, ref_hap, _ = b.layout(r)
    assert ref_hap is not None and ref_hap >= hb + U                     # the helper haplotype
    assert all(len(b.haplotype(r, l)[0]) < len(regions[r]["ref"]) for l in range(U))
    assert ra[r][2] == len(regions[r]["ref"])                            # lmax from it alone
    r = name["len_1025"]
    assert b.layout(r)[2] is None and ra[r][:2] == (NONE, 0) and ra[r][2] == 1026  # (the insertion's haplotype)
    for w in words:
        assert w & BIT["FAST"] and not w & BIT["GIVEUP"], hex(w)
    assert "A" in regions[name["first_reuses"]]["ref"]  # (reference hits to inherit)


U_NAMES = ("u1", "u64", "u65", "u256", "u257", "u384", "u385", "u512", "u513")


@pytest.mark.parametrize("mode", ["default", "bigu0", "bigu1"])
def test_thread_and_shape_edges(mode, scanner):
    env = {"default": {}, "bigu0": {"TFBS_KF_BIGU": "0"}, "bigu1": {"TFBS_KF_BIGU": "1"}}[mode]
    batch = case_batch(U_NAMES)
    b, sc, words, ra = run(batch, env, scanner)
    for name, w in zip(U_NAMES, words):
        U = int(name[1:])
        big = {"default": U > 384, "bigu0": False, "bigu1": U > 1}[mode]
        assert w & BIT["FAST"] and not w & BIT["GIVEUP"], (name, hex(w))
        assert bool(w & BIT["BIG"]) == big, (name, hex(w))
        assert bool(w & BIT["HAP_GLOBAL"]) == (U > (2048 if big else 512)), (name, hex(w))
    # a region of the reference alone: no run, and reference hits beside it
    assert ra[0][:2] == (NONE, 0) and len(A.reference_hits(SPECS["u1"]())) > 0


def test_staged_runs_limit(scanner):
    batch = case_batch(("runs97", "runs96", "u1"))
    b, sc, words, ra = run(batch, {}, scanner)
    assert [x[1] for x in ra] == [16 * 97, 16 * 96, 0]
    assert [bool(w & BIT["RUNS_L2"]) for w in words] == [True, False, False]
    assert not any(w & BIT["GIVEUP"] for w in words)


def test_reference_hits_and_the_spill_list(scanner):
    names = ("refs0", "refs1", "refs63", "refs64", "refs65")
    assert [len(A.reference_hits(SPECS[n]())) for n in names] == [0, 1, 63, 64, 65]
    b, sc, words, _ = run(case_batch(names), {}, scanner)
    assert sc.assembly_figures()["spill"] >= 1 and not sc.post_figures()["left_out"]  # the 65th: a spill record
    assert not any(w & BIT["GIVEUP"] for w in words)
    # without it nothing spills: the second step leaves the post-scan stage out (no bucket is read;
    # wave lists of 8 192 candidates: none past a list, which would keep the stage)
    b, sc, words, _ = run(case_batch(names[:4]), {"TFBS_CAND_CAP": "8192"}, scanner, steps=2)
    assert sc.assembly_figures()["spill"] == 0 and sc.post_figures()["left_out"]
    assert not any(w & BIT["GIVEUP"] for w in words)


TICKET_NAMES = ("small0", "small1", "small2", "nokeys", "u128", "refs257", "small3", "small4", "small5")


@pytest.mark.parametrize("mode", ["grid1", "grid2", "grid3", "persist0"])
def test_tickets_past_regions_that_leave_early(mode, scanner):
    """TFBS_KEY_FAST_MAXU=100: the region of 128 haplotypes gives up on its shape, the one of 257
    reference hits on those, the one without an inner range leaves before either (the exit of
    `U == 0 || K == 0`, in front of the second round of loads: a region of a batch with samples has
    at least its reference haplotype, so only a batch of zero samples reaches U == 0).  Every region's
    word is written (the trace is zeroed before the launch: a skipped region reads 0; a region
    taken twice would be listed twice for key_asm_kernel or counted twice in the varying lists,
    which the figures and the oracle's keys exclude) and every region but a workgroup's first
    came by ticket."""
    env = {"TFBS_KEY_FAST_MAXU": "100"}
    env.update({"persist0": {"TFBS_KF_PERSIST": "0"}}.get(mode, {"TFBS_KF_GRID": mode[4:]}))
    batch = case_batch(TICKET_NAMES)
    ps, n, beds, regions, okeys, orows = batch
    sc = scanner(ps, env)
    with _env(env):
        b = build_batch(ps, n, beds, list(regions))
        b.scan(sc, reduce=True)
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows
    assert_records(b, sc, regions)
    words = b.assembly_paths(sc)
    assert b.layout(TICKET_NAMES.index("nokeys"))[3] == 0
    assert all(w & BIT["FAST"] for w in words), [hex(w) for w in words]
    gave_up = {TICKET_NAMES[r]: T.path_why(w) for r, w in enumerate(words) if w & BIT["GIVEUP"]}
    assert gave_up == {"u128": 0, "refs257": 3}
    assert sc.assembly_figures()["left"] == 2
    tickets = sum(1 for w in words if w & BIT["TICKET"])
    assert tickets == (0 if mode == "persist0" else len(words) - int(mode[4:]))
    assert_same_without_key_fast(b, batch, env, scanner)


def test_replay_and_staleness(scanner):
    """Five tfbs_step calls on X (plain ones, the captured one, replays), batch Y of other region
    sizes on the same ctx, X again, then a batch after the one-haplotype upload of tfbs_matches:
    each time the records are the resident batch's and the reduction the oracle's; the batches'
    digests under TFBS_KEY_FAST_MAXU=0 and their path words on a tracing ctx (a traced step takes
    no graph) besides."""
    X, Y = case_batch(("u65", "small1", "refs64", "u257")), case_batch(("small4", "u256", "refs1"))
    with _env({"TFBS_MFMA": "1"}):
        sc = T.Scanner(X[0])  # (no trace: the steps take the graph)
        try:
            def steps(batch, count):
                ps, n, beds, regions, okeys, orows = batch
                b = build_batch(ps, n, beds, list(regions))
                T.check(T.lib().tfbs_batch_upload(sc.h, b.h))
                assert_records(b, sc, regions)
                for _ in range(count):
                    T.check(T.lib().tfbs_step(sc.h, b.h))
                T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
                _assert_keys(b, okeys)
                assert b.rows(CHROM)[0] == orows
                return b

            for batch in (X, Y):
                traced = scanner(batch[0], {})
                t = build_batch(*batch[:3], list(batch[3]))
                t.scan(traced, reduce=True)
                assert all(w & BIT["FAST"] and not w & BIT["GIVEUP"] for w in t.assembly_paths(traced))
                assert_same_without_key_fast(steps(batch, 1), batch, {}, scanner)
            steps(X, 5)
            steps(Y, 1)
            steps(X, 1)
            sc.matches_all([("ACGT"[i % 4], 100 + i) for i in range(50)])
            ra, hr = sc.region_asm()
            assert ra == [(NONE, 0, 50, 0)] and hr == [NONE]
            steps(Y, 4)
        finally:
            sc.close()
