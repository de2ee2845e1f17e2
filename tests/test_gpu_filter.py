"""The matrix-core filter on the device against its restatement in tests/filter_ref.py.

tfbs_matches scans one haplotype with every window listed, no reuse and zeroed pad words,
so the candidates the scan kernel counts (tfbs_ctx_scan_counters' out[2]) are a pure
function of the uploaded image and the bases: the model predicts them to the unit.  Every
case of tests/filter_cases.py (proven on its edge by test_filter_cases_cpu.py) runs in
every mode; the hits must equal the oracle's and the count the model's.  A filter that
over-fires changes only the count; one that under-fires loses a hit planted on its edge."""
import ctypes
import random

import pytest

import filter_cases as FC
import filter_ref as F
import oracle_py as O
from helpers import T, build_batch, run_oracle

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "lds8": {"TFBS_MFMA_LDS_KB": "8"},
         "small_lists": {"TFBS_CAND_CAP": "64", "TFBS_CAND_OVER_CAP": "16"}}
ENV = ("TFBS_MFMA", "TFBS_MFMA_LDS_KB", "TFBS_CAND_CAP",
       "TFBS_CAND_OVER_CAP", "TFBS_SCAN_UNIT", "TFBS_MFMA_HAPS_PER_BLOCK", "TFBS_DEDUP", "TFBS_SHARE")
CASES = ["neighbours", "every_place_1", "every_place_2", "every_place_63", "every_place_64", "every_place_65",
         "depths", "t0mix", "lists", "scales"]
WAVES, LDS_CANDS = 8, 48  # waves per scan workgroup, a wave's candidates kept in LDS


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in FC.all_cases()}


_oracle = {}


def oracle_matches(case, name):
    """Per pattern the oracle's [(start, end)] of a case haplotype (positions = indices),
    computed once for all modes."""
    key = (case.name.split("@")[0], name)
    if key not in _oracle:
        hap = [(ch, j) for j, ch in enumerate(case.haps[name])]
        _oracle[key] = [O.matches([w.acgtn for w in p.weights], p.min_score, hap) for p in case.patterns]
    return _oracle[key]


def counters(sc):
    out = (ctypes.c_uint64 * 5)()
    T.check(T.lib().tfbs_ctx_scan_counters(sc.h, out))
    return [int(x) for x in out]


def check_lists(out, n_wg, cap_wg, where):
    """out[1] (past the waves' lists) and out[3] (in the waves' global lists) against the
    capacities in force: n_wg workgroups of 8 waves, each wave min(cap, 48) LDS entries and
    cap = cap_wg / 8 global ones."""
    over, total, glob = out[1], out[2], out[3]
    cap = cap_wg // WAVES
    lcap = min(cap, LDS_CANDS)
    waves = WAVES * n_wg
    assert over + glob <= total, where
    assert total - over - glob <= waves * lcap and glob <= waves * cap, where
    if total <= lcap:
        assert over == 0 and glob == 0, where
    if total <= lcap + cap:
        assert over == 0, where
    if over:
        assert glob >= cap, where
    assert over >= total - waves * (lcap + cap), where


def set_mode(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_candidates_equal_the_model(cases, monkeypatch, mode, name):
    case = cases[name]
    env = MODES[mode]
    set_mode(monkeypatch, env)
    fp = F.FilterPlan(case.pset.mfma_plan(int(env.get("TFBS_MFMA_LDS_KB", 0))))
    n_supers = len(fp.supers)
    cand_cap = int(env.get("TFBS_CAND_CAP", 1024))
    n_wg, cap_wg = 1, min(1 << 16, cand_cap * n_supers)
    sc = T.Scanner(case.pset)
    try:
        for hname, hap in case.haps.items():
            got = sc.matches_all([(ch, j) for j, ch in enumerate(hap)])
            want = oracle_matches(case, hname)
            for i in range(len(case.patterns)):
                assert got[i] == want[i], (mode, name, hname, i)
            out = counters(sc)
            total, _, per_class = F.candidates(fp, hap)
            print(mode, name, hname, "candidates", out[2], "model", total, per_class, "global", out[3], "over", out[1])
            assert out[2] == total, (mode, name, hname, out, per_class)
            check_lists(out, n_wg, cap_wg, (mode, name, hname, out))
            if mode == "small_lists" and name == "lists":
                assert out[1] > 16, out  # past the 16 overflow entries: the list grew, the scan ran again
    finally:
        sc.close()


def _region(lmax, start, n, n_distinct, seed):
    """n random bases (extended start to extended end); distinct haplotype t = 1 ..
    n_distinct - 1 is the reference with one SNV, carried by haplotype id t alone; every
    other id is the reference.  Returns the region and its distinct haplotypes' texts."""
    rnd = random.Random(seed)
    ref = "".join(rnd.choice("ACGT") for _ in range(n))
    es = start - lmax + 1
    step = (n - 20) // n_distinct
    recs, texts = [], [ref]
    for t in range(1, n_distinct):
        p = 10 + step * t
        alt = "ACGT"[("ACGT".index(ref[p]) + 1) % 4]
        recs.append(("car", es + p, ref[p], alt, [t]))
        texts.append(ref[:p] + alt + ref[p + 1:])
    return {"merged": (start, start + n - 2 * lmax + 1), "ref": ref, "records": recs}, texts


@pytest.mark.parametrize("unit", ["1", "2", "4"])
def test_batch_candidates_equal_the_model(cases, monkeypatch, unit):
    """Three regions of 70 distinct haplotypes through RegionBatch.scan, every haplotype
    scanned whole (TFBS_DEDUP=0, TFBS_SHARE=0), groups of 4 in units of 1, 2 and 4: the
    window lists, the candidates and the keys."""
    case = cases["depths"]
    ps = case.pset
    set_mode(monkeypatch, {"TFBS_DEDUP": "0", "TFBS_SHARE": "0", "TFBS_SCAN_UNIT": unit,
                           "TFBS_MFMA_HAPS_PER_BLOCK": "4"})
    fp = case.plan
    regs, texts = [], []
    for j in range(3):
        reg, tx = _region(ps.max_length, 5000 + 3000 * j, 250 + 11 * j, 70, 40 + j)
        regs.append(reg)
        texts += tx
    beds = [("synthetic.bed", [r["merged"] for r in regs])]
    okeys, _, _ = run_oracle(ps, 40, beds, regs)
    lmin = fp.class_lmin()
    want_lists = [sum(F.n_windows(len(h), lmin[c]) for h in texts) for c in (0, 1)]
    want_cands = sum(F.candidates(fp, h)[0] for h in texts)
    sc = T.Scanner(ps)
    try:
        b = build_batch(ps, 40, beds, regs)
        assert b.num_haplotypes == len(texts) == 210  # (the reference is one of them: no helper copy)
        b.scan(sc)
        for i, want in enumerate(okeys):
            assert b.keys(i) == want, (unit, i)
        ent, sec = (ctypes.c_uint64 * 2)(), ctypes.c_double()
        T.check(T.lib().tfbs_ctx_window_lists(sc.h, ent, ctypes.byref(sec)))
        assert [int(ent[0]), int(ent[1])] == want_lists
        out = counters(sc)
        print("unit", unit, "candidates", out[2], "model", want_cands, out)
        assert out[2] == want_cands, (unit, out)
        assert out[1] + out[3] <= out[2]
    finally:
        sc.close()
