"""Device contexts that come and go in one process: everything a context allocates lazily is
used on one, which is destroyed while its batch lives on; the batch's host paths, a context
that was alive beside it and one made afterwards must all give what the oracle gives.  Results
and return codes only (the cases are synthetic: a handful of regions, 24 samples, one mono and
one dinucleotide pattern -- the mono PWM embedded, so the oracle scores both)."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import dinuc_ref as D
import effects_ref as E
from helpers import T, make_regions_synth, run_oracle, synth_patterns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


def rows_set_async(sc, on):
    """tfbs::rows_set_async (rows.hpp; the run flow's switch, no C-ABI entry point): a drained
    slot's blocks are copied back and written by the context's two writer threads."""
    fn = getattr(T.lib(), "_ZN4tfbs14rows_set_asyncEP8tfbs_ctxb")
    fn.argtypes = [ctypes.c_void_p, ctypes.c_bool]
    fn.restype = None
    fn(sc.h, on)


def outputs(b, sc):
    return b.hits(sc), b.best(sc), b.score_rows(sc, "chr1"), b.effects(sc)


def same_outputs(x, y):
    return all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(x, y))


def test_contexts_come_and_go(tmp_path, monkeypatch):
    monkeypatch.setenv("TFBS_BGZF_BATCH_BLOCKS", "1")  # (every launch takes another slot)
    mono, _ = synth_patterns(tmp_path, 2, 2, 31, thr=2e-3)
    first_id = min(p.pattern_id for p in mono.to_list())
    ps = T.PatternSet.from_patterns([
        p if p.pattern_id == first_id else
        T.Pattern.DiPWM(D.embed_mono([w.acgtn[:4] for w in p.weights]), p.name, p.pattern_id, p.min_score, p.direction)
        for p in mono.to_list()])
    assert {p.kind for p in ps.to_list()} == {T.KIND_PWM, T.KIND_DIPWM}
    n = 24
    regions = make_regions_synth(5, 0, 5, n, mono.max_length, 30)
    assert all("N" not in r["ref"] for r in regions)  # (an embedded PWM scores N-free windows as the mono one)
    beds = [("a.bed", [r["merged"] for r in regions])]
    okeys, orows, _ = run_oracle(mono, n, beds, regions)
    assert sum(sum(l) + sum(r) for k in okeys for l, r in k.values()) >= 20 and orows.count("\n") >= 3
    L = T.lib()
    b = E.build_batch(ps, n, beds, regions)  # (keeps its variants: effects)
    nr = b.num_regions
    sc1, sc2 = T.Scanner(ps), T.Scanner(ps)
    try:
        b.upload(sc1)
        for _ in range(4):  # plain, plain, captured, replayed
            T.check(L.tfbs_step(sc1.h, b.h))
        T.check(L.tfbs_batch_reduce(sc1.h, b.h))
        b.encode(sc1)
        rows_set_async(sc1, True)
        fd = os.open(str(tmp_path / "rows1.gz"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
        try:
            _, _, n_rows, _ = b.rows_bgzf(sc1, "chr1", fd=fd)
            out1 = outputs(b, sc1)
            sc1.close()  # its writer threads' queued blocks go out first; the batch lives on
        finally:
            os.close(fd)
        assert n_rows == orows.count("\n")
        assert gzip.decompress(open(str(tmp_path / "rows1.gz"), "rb").read()).decode() == orows
        # the batch's host paths: its varying counts came to the host when their context went
        assert [b.keys(r) for r in range(nr)] == okeys
        assert b.rows("chr1")[0] == orows
        # the context that was alive beside it: the same batch from scratch
        b.scan(sc2, reduce=True, encode=True)
        assert [b.keys(r) for r in range(nr)] == okeys
        assert b.rows("chr1")[0] == orows
        data, _, n_rows, _ = b.rows_bgzf(sc2, "chr1")
        assert n_rows == orows.count("\n") and gzip.decompress(data).decode() == orows
        assert same_outputs(outputs(b, sc2), out1)
        assert len(out1[0]) > 0 and len(out1[1]) > 0 and len(out1[3]) > 0
        sc2.close()
        sc3 = T.Scanner(ps)  # and one made after both went
        try:
            b.upload(sc3)
            T.check(L.tfbs_step(sc3.h, b.h))
            T.check(L.tfbs_batch_reduce(sc3.h, b.h))
            assert [b.keys(r) for r in range(nr)] == okeys
        finally:
            sc3.close()
        assert [b.keys(r) for r in range(nr)] == okeys
    finally:
        sc1.close()
        sc2.close()
