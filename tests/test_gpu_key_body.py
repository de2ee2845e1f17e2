"""key_fast_kernel's region body (key_kernels.hip) on the edges of its hit-major dirty test and of
its counter chunks, on key_body_cases.py's regions (test_key_body_cases_cpu.py shows without a
device that each sits on its edge).

The dirty test: 0, 1, 7, 8, 9, 63, 64, 65, 128, 256 reference hits (a group of 8, a slice of 64,
the hits past the region's list of 64 through the spill records), every hit dirty for exactly one
haplotype, so a hit that is dropped shows; 70 hits under 140 and 520 haplotypes (no hit shares on
either shape: one wave meets a second slice of 6 hits); U = 1, 63, 64, 65, 128 | 129 (the hit shares of the
common shape), 257, 512 | 513 (those of the big shape); 0, 1, 7, 9 and 16 runs per haplotype, a
haplotype without reuse between reusing ones, a run on a window's first column only and on its
last only (assembly_cases' core), hits under 1, 2 and 32 ranges, and 3 585 dirty corrections, one
more than the top of the list holds (the second pass).  All of it on the default shapes and on
the big one alone (TFBS_KF_BIGU=1).

The chunks: T = rows_per - 1 | rows_per | rows_per + 1 and 256 | 257 (the rows' keys once | per
chunk), U = 1, 2, 3 and odd | even, rows that are equal and not 0, that cancel to 0, that differ
on the first or on the last haplotype alone, in a chunk's first and last rows, varying rows on
either side of the chunk's 64th row; with compact lists that regrow (TFBS_VAR_CAP), under the
any-placement body (TFBS_KEY_COR_LDS=0) and through three replayed tfbs_step calls.

Every run: the oracle's keys, per-sample vectors and rows, the path words assembly_cases.predict
gives the figures, and the same digests under TFBS_KEY_FAST_MAXU=0 (key_asm_kernel alone)."""
import contextlib
import os

import numpy as np
import pytest

import assembly_cases as A
import key_body_cases as C
from helpers import T, build_batch

pytestmark = pytest.mark.gpu

CHROM = "chr1"
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
    """One Scanner per (pattern set, environment, tracing): the knobs are read when it is made."""
    made = {}

    def get(kind, env, trace=True):
        key = (kind, tuple(sorted(env.items())), trace)
        if key not in made:
            with _env(dict(env, TFBS_MFMA="1")):
                made[key] = T.Scanner(A.pattern_set(kind))
            made[key].assembly_trace(trace)
        return made[key]

    yield get
    for sc in made.values():
        sc.close()


def _assert_oracle(b, key):
    okeys, orows = A.oracle(key)
    assert b.num_regions == len(okeys)
    for i, want in enumerate(okeys):
        got = b.keys(i)
        assert got.keys() == want.keys(), (key[i], sorted(set(got) ^ set(want))[:4])
        for k in want:
            assert got[k] == want[k], (key[i], k)
    assert b.rows(CHROM)[0] == orows


def _reduce(key, env, scanner):
    specs = [A.case(n) for n in key]
    sc = scanner(specs[0]["kind"], env)
    with _env(env):
        b = build_batch(*A.materialize(specs))
        b.scan(sc, reduce=True)
    return b, sc


def _lists_per_group(kind):
    return 8 * A.pattern_set(kind).plan_stats(mfma=True)["n_mfma_supers"]


def run(batch, env, scanner, **predict_kw):
    """The batch reduced under env: the oracle's keys and rows, the predicted path words, and the
    same digests from key_asm_kernel alone."""
    key = C.BATCHES[batch]
    b, sc = _reduce(key, env, scanner)
    _assert_oracle(b, key)
    words = b.assembly_paths(sc)
    figs, preds = A.mixed_predictions(key, _lists_per_group(A.case(key[0])["kind"]), **predict_kw)
    for r, (P, why) in enumerate(preds):
        print(key[r], hex(words[r]), figs[r])
        for name, want in P.items():
            if want is not None:
                assert bool(words[r] & BIT[name]) == want, (key[r], name, hex(words[r]), figs[r])
        assert why is None and not words[r] & BIT["GIVEUP"], (key[r], hex(words[r]))
    b0, sc0 = _reduce(key, dict(env, TFBS_KEY_FAST_MAXU="0"), scanner)
    for r, (x, y) in enumerate(zip(b.region_digests(), b0.region_digests())):
        assert np.array_equal(x, y), key[r]
    assert all(w & BIT["ASM"] for w in b0.assembly_paths(sc0))
    return words, figs


SHAPES = {"default": ({}, {}), "bigu1": ({"TFBS_KF_BIGU": "1"}, dict(big_u=1))}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("batch", list(C.DIRTY_BATCHES))
def test_dirty_test(batch, shape, scanner):
    env, kw = SHAPES[shape]
    words, figs = run(batch, env, scanner, **kw)
    for name, w, f in zip(C.BATCHES[batch], words, figs):
        assert not w & BIT["WALK"], name  # the pairwise test
        assert bool(w & BIT["BIG"]) == (f["U"] > (1 if shape == "bigu1" else A.BIG_U)), name
        if name == "listed_3585":  # (the big shape's list holds them)
            assert bool(w & BIT["DIRTY_LISTED"]) == (shape == "bigu1")
        elif f["nref"]:
            assert w & BIT["DIRTY_LISTED"], name


CHUNK_MODES = {"default": ({}, {}),
               "var_cap": ({"TFBS_VAR_CAP": "8"}, {}),
               "cor_lds0": ({"TFBS_KEY_COR_LDS": "0"}, dict(cor_lds=0))}


@pytest.mark.parametrize("mode", list(CHUNK_MODES))
@pytest.mark.parametrize("batch", list(C.CHUNK_BATCHES))
def test_counter_chunks(batch, mode, scanner):
    env, kw = CHUNK_MODES[mode]
    words, figs = run(batch, env, scanner, **kw)
    for name, w, f in zip(C.BATCHES[batch], words, figs):
        assert not w & BIT["BIG"], name
        assert bool(w & BIT["CNT_ARENA"]) == (mode == "cor_lds0"), name
        assert bool(w & BIT["U32"]) == (mode == "cor_lds0"), name  # packed counters: the typed body


@pytest.mark.parametrize("batch", list(C.CHUNK_BATCHES))
def test_replayed_steps(batch, scanner):
    """Three tfbs_step calls (plain, captured, replayed) on a ctx without a trace, then the reduction."""
    key = C.BATCHES[batch]
    specs = [A.case(n) for n in key]
    sc = scanner(specs[0]["kind"], {}, trace=False)
    b = build_batch(*A.materialize(specs))
    T.check(T.lib().tfbs_batch_upload(sc.h, b.h))
    for _ in range(3):
        T.check(T.lib().tfbs_step(sc.h, b.h))
    T.check(T.lib().tfbs_batch_reduce(sc.h, b.h))
    _assert_oracle(b, key)
