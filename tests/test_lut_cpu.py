"""The LUT and generic scan paths on the host: the model (lut_ref.py) against the oracle on every
mono case, the properties of the copied plan (PatternSet.lut_plan) that scan_fast_kernel and
scan_generic_kernel rely on, every table entry and the lookup loop's decisions against the
specification, the model-only conditions that make the cases bite, and the proofs that each case
reaches the path it names.  Integer work: every comparison is exact."""
import ctypes as C
import random

import pytest

import dinuc_cases as K
import dinuc_ref as D
import lut_ref as R
import mono_cases as M
from helpers import T, run_oracle

TFBS_E_ARG = -1
OPTION_SETS = ((8, False), (20, False), (36, False), (20, True))
CASE_NAMES = sorted(M.CASES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_model_equals_the_oracle(name):
    """The C restatement of the reference checks the Python one: keys on every case, rows (rebuilt
    from the model's keys) where the GPU tests compare rows."""
    case = M.CASES[name]()
    ps = T.PatternSet.from_patterns(case["pats"])
    keys, rows, _ = run_oracle(ps, case["n"], case["beds"], case["regions"])
    for i, want in enumerate(case["want"]):
        assert keys[i] == want, i
    if name in ("tiles", "reduction"):
        assert rows == K.rebuild_rows(case["want"], case["beds"], ps.name_of)
        assert rows.count("\n") >= 20


# ---------------------------------------------------------------------------------------
# plan properties
# ---------------------------------------------------------------------------------------
def group_need(pats, strands):
    """The blocks one pattern_id's strands need alone: octet strands 8 to a unit, quad strands 4,
    a unit as deep as its longest strand."""
    need = 0
    for octet, per in ((True, 8), (False, 4)):
        blk = [(len(pats[i]) + 3) // 4 for i in strands if R.is_octet(pats[i]) == octet]
        need += sum(max(blk[u:u + per]) for u in range(0, len(blk), per))
    return need


def check_plan(pats, plan, tile_blocks):
    lp = R.LutPlan(plan)
    scannable = [i for i, p in enumerate(pats) if p.kind == T.KIND_PWM and len(p) >= 1]
    by_pid = {}
    for i in scannable:
        by_pid.setdefault(pats[i].pattern_id, []).append(i)
    generic = R.generic_ids(pats)
    # the slot order
    order = sorted(by_pid, key=lambda pid: (pid in generic, max(len(pats[i]) for i in by_pid[pid]), pid))
    assert plan["slot_pid"] == order
    slot_of = {pid: k for k, pid in enumerate(order)}
    # every strand exactly once, on the path its pattern_id's group takes
    for i in scannable:
        pid = pats[i].pattern_id
        places = len(lp.fast.get(i, [])) + len(lp.gen.get(i, [])) + plan["slot_mfma"][slot_of[pid]]
        assert places == 1, (i, places)
        assert (i in lp.gen) == (pid in generic)
    assert set(lp.fast) | set(lp.gen) <= set(scannable)
    # tiles
    rnd = random.Random(5)
    images = [[0] * 32, [3] * 32] + [[rnd.randrange(4) for _ in range(32)] for _ in range(30)]
    n_blocks = len(plan["lut"]) // 1024
    assert len(plan["lut"]) == 1024 * n_blocks
    prev_end, prev_lut = -1, 0
    for ti, t in enumerate(plan["tiles"]):
        assert 1 <= t["nslots"] <= 64
        assert t["slot_begin"] > prev_end
        prev_end = t["slot_begin"] + t["nslots"] - 1
        assert t["lut_begin"] == prev_lut and t["nblocks"] >= 1
        prev_lut += t["nblocks"]
        assert t["first"] < t["last"] and (ti == 0 or t["first"] == plan["tiles"][ti - 1]["last"])
        members, spans = [], []
        for ui in range(t["first"], t["last"]):
            U = plan["units"][ui]
            width = lp.width(U)
            assert U["kind"] in (R.OCTET, R.QUAD) and 1 <= U["nstrand"] <= width
            real = [s for s in range(width) if U["orig_index"][s] != R.NO_STRAND]
            assert real == list(range(U["nstrand"]))
            for s in real:
                p = pats[U["orig_index"][s]]
                assert (U["kind"] == R.OCTET) == R.is_octet(p), (ti, ui, s)
                assert U["len"][s] == len(p) and U["min_score"][s] == p.min_score
                assert t["slot_begin"] + U["slot_local"][s] == slot_of[p.pattern_id]
                assert U["slot_local"][s] < t["nslots"]
                members.append(U["orig_index"][s])
            assert U["nblk"] == max((len(pats[U["orig_index"][s]]) + 3) // 4 for s in real)
            spans.append((U["lut_off"], U["lut_off"] + U["nblk"]))
            for s in range(U["nstrand"], width):  # padding: never a hit
                assert not any(lp.decode_at(ti, ui, s, img) for img in images), (ti, ui, s)
        spans.sort()
        assert spans[0][0] >= 0 and spans[-1][1] <= t["nblocks"]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert t["lmin"] == min(len(pats[i]) for i in members)
        assert t["slot_begin"] + t["nslots"] - 1 == max(slot_of[pats[i].pattern_id] for i in members)
        pids = {pats[i].pattern_id for i in members}
        for pid in pids:  # whole groups
            assert set(by_pid[pid]) <= set(members)
        assert t["nblocks"] <= max(tile_blocks, max(group_need(pats, by_pid[pid]) for pid in pids))
        assert len(pids) == 1 or t["nblocks"] <= tile_blocks
    assert prev_lut == n_blocks
    # generic tiles: one per pattern_id, its strands' own columns with N = 0
    for gi, t in enumerate(plan["gen_tiles"]):
        assert t["nslots"] == 1 and t["slot_begin"] > prev_end
        prev_end = t["slot_begin"]
        pid = order[t["slot_begin"]]
        assert pid in generic
        assert [plan["gen_pats"][k]["orig_index"] for k in range(t["first"], t["last"])] == by_pid[pid]
        for k in range(t["first"], t["last"]):
            g = plan["gen_pats"][k]
            p = pats[g["orig_index"]]
            assert (g["len"], g["min_score"], g["slot_local"]) == (len(p), p.min_score, 0)
            assert lp.gen_columns(k) == [c + [0] for c in R.columns(p)]
        assert t["lmin"] == min(len(pats[i]) for i in by_pid[pid])
    return lp


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_properties(name):
    case = M.CASES[name]()
    ps = T.PatternSet.from_patterns(case["pats"])
    for tile_blocks, mfma in OPTION_SETS:
        plan = ps.lut_plan(tile_blocks, mfma)
        check_plan(case["pats"], plan, tile_blocks)
        st = ps.plan_stats(tile_blocks, mfma)
        assert (st["n_fast_tiles"], st["n_fast_units"], st["n_generic_tiles"], st["n_generic_strands"]) == (
            len(plan["tiles"]), len(plan["units"]), len(plan["gen_tiles"]), len(plan["gen_pats"]))
        assert st["lut_bytes"] == 4 * len(plan["lut"])


# ---------------------------------------------------------------------------------------
# decoded tables
# ---------------------------------------------------------------------------------------
def check_entries(lp, pats):
    """Every entry of every block of every fast strand against the specification."""
    for i, places in lp.fast.items():
        (ti, ui, s), = places
        U, p = lp.units[ui], pats[i]
        cols = R.columns(p)
        octet = U["kind"] == R.OCTET
        br = R.block_ranges(p)
        for b in range(U["nblk"]):
            for code in range(256):
                exact = sum(cols[4 * b + j][(code >> (2 * j)) & 3] for j in range(4) if 4 * b + j < len(cols))
                e = lp.entry(ti, ui, s, b, code)
                if b >= len(br):  # past a short strand's last block
                    assert e == 0, (i, b, code)
                elif octet:
                    assert e == exact - br[b][1] and -32767 <= e <= 0, (i, b, code)
                else:
                    assert e == D.wrap32(exact), (i, b, code)
        if octet:
            thr = min(p.min_score - sum(hi for _, hi in br), 0)
            assert -32768 <= thr and U["thr"][s] == thr
            assert lp.init_half(ui, s) == -(thr + 1)
        else:
            assert U["thr"][s] == p.min_score


def check_decisions(lp, pats, seqs_per_region, max_seqs=3):
    """decode() against score > min_score on the cases' N-free windows and on every strand's
    all-lowest and all-highest window, each image under two different tails; returns the number
    of windows tied with and one above the threshold."""
    tied = one_off = 0

    def check(i, p, window, follow):
        exact = sum(c[x] for c, x in zip(R.columns(p), window))
        want = D.wrap32(exact) > p.min_score
        for tail in (follow + [0], [3 - x for x in follow] + [3, 1]):
            assert lp.decode(i, R.image_of(window, tail)) == want, (i, window, tail)
        return D.wrap32(exact) - p.min_score

    for i in lp.fast:
        p = pats[i]
        L = len(p)
        for highest in (False, True):
            check(i, p, R.extreme_window(p, highest), [1, 2])
        for sq in seqs_per_region:
            for codes, _ in sorted(set(sq))[:max_seqs]:
                for w in range(len(codes) - L + 1):
                    window = list(codes[w:w + L])
                    if 4 in window:
                        continue  # rescored exactly, column by column: not the table's business
                    d = check(i, p, window, [0 if c == 4 else c for c in codes[w + L:w + 32]])
                    tied += d == 0
                    one_off += d == 1
    return tied, one_off


@pytest.mark.parametrize("name", CASE_NAMES)
def test_decoded_tables(name):
    case = M.CASES[name]()
    ps = T.PatternSet.from_patterns(case["pats"])
    for tile_blocks, mfma in ((20, False), (8, False), (20, True)) if name in ("tiles", "interleaved") else ((20, False),):
        lp = R.LutPlan(ps.lut_plan(tile_blocks, mfma))
        check_entries(lp, case["pats"])
        if tile_blocks == 20:
            tied, one_off = check_decisions(lp, case["pats"], case["seqs"])
            if name == "arithmetic":
                assert tied >= 5 and one_off >= 5
            elif name not in ("generic",) and not mfma:
                assert tied >= 5


# ---------------------------------------------------------------------------------------
# the cases bite
# ---------------------------------------------------------------------------------------
def test_cases_bite():
    st = M.case_n_and_indels()["stats"]
    for k in ("n_first", "n_last", "a_hits_exact_not", "exact_hits_a_not", "differ_32", "after_indel", "tied"):
        assert st[k] >= 5, k
    st = M.case_arithmetic()["stats"]
    for k in ("outside_int32", "tied", "n_first", "n_last"):
        assert st[k] >= 5, k
    st = M.case_generic()["stats"]
    for k in ("n_first", "n_last", "a_hits_exact_not", "exact_hits_a_not", "differ_long", "after_indel", "tied"):
        assert st[k] >= 5, k


def test_every_pattern_id_has_a_key():
    for name in CASE_NAMES:
        case = M.CASES[name]()
        silent = {p.pattern_id for p in case["pats"] if p.min_score == M.INT32_MAX}
        assert K.ids_with_a_key(case["want"]) == {p.pattern_id for p in case["pats"]} - silent, name
        assert K.total_hits(case["want"]) >= 100, name
    assert len({p.pattern_id for p in M.case_arithmetic()["pats"] if p.min_score == M.INT32_MAX}) == 5


def test_geometry_window_counts_and_haplotypes():
    case = M.case_geometry()
    lengths = {len(codes) for sq in case["seqs"] for codes, _ in sq}
    assert set(M.GEOMETRY_WINDOWS) <= lengths  # windows of the 1-column strands
    assert len(set(case["seqs"][-1])) > 128
    # hits of the short strands in the last two chunks of a three-chunk tail, and of a 32-column
    # strand whose windows end before the tile's
    for nwin in (129, 191, 192):
        reg = M.GEOMETRY_WINDOWS.index(nwin)
        late = 0
        for codes, pos in set(case["seqs"][reg]):
            for p in case["pats"]:
                late += sum(1 for i, v in enumerate(R.exact_scores(p, codes)) if i >= 64 and v > p.min_score)
        assert late >= 5, nwin
    assert {len(p) for p in case["pats"]} == set(M.GEOMETRY_LENGTHS)


def test_reduction_pass_edges():
    case = M.case_reduction()
    n_inner = [len(T.select_inner_peaks(r["merged"], case["beds"])) for r in case["regions"]]
    assert n_inner[:3] == [40, 8, 9]
    twice = T.select_inner_peaks(case["regions"][3]["merged"], case["beds"])
    assert len(twice) == 3 and len(set(twice)) == 2


def test_arithmetic_edges_are_what_they_say():
    case = M.case_arithmetic()
    bias0, bias1, range0, range1, mag0, mag1 = case["edges"]
    for p, biased in ((bias0, -32768), (bias1, -32769)):
        assert p.min_score - sum(hi for _, hi in R.block_ranges(p)) == biased
    assert [max(hi - lo for lo, hi in R.block_ranges(p)) for p in (range0, range1)] == [32767, 32768]
    assert [sum(max(abs(lo), abs(hi)) for lo, hi in R.block_ranges(p)) for p in (mag0, mag1)] == [(1 << 30) - 1, 1 << 30]
    assert [R.is_octet(p) for p in case["edges"]] == [True, False] * 3
    # the planted windows: every block's lowest (its 16-bit sum saturates on the way) and highest
    ref = M.codes_of(case["regions"][0]["ref"])
    lo, hi = R.extreme_window(bias0, False), R.extreme_window(bias0, True)
    assert ref[62:74] == lo and ref[76:88] == hi
    br = R.block_ranges(bias0)
    assert sum(l - h for l, h in br) < -32768 and sum(l - h for l, h in br[:2]) < -32768 + 32767
    thresholds = {p.min_score for p in case["pats"]}
    assert {M.INT32_MIN, M.INT32_MAX} <= thresholds


# ---------------------------------------------------------------------------------------
# path proofs
# ---------------------------------------------------------------------------------------
def tile_kinds(plan):
    return [{plan["units"][u]["kind"] for u in range(t["first"], t["last"])} for t in plan["tiles"]]


def test_paths_are_taken():
    ps = T.PatternSet.from_patterns(M.case_tiles()["pats"])
    plan = ps.lut_plan(8)
    assert len(plan["tiles"]) >= 3 and any(k == {R.OCTET, R.QUAD} for k in tile_kinds(plan))
    assert len(plan["slot_pid"]) > 64 and plan["slot_pid"] != sorted(plan["slot_pid"])
    for tb in (20, 36):
        assert any(k == {R.OCTET, R.QUAD} for k in tile_kinds(ps.lut_plan(tb)))
    lp = R.LutPlan(ps.lut_plan(20))
    pats = M.case_tiles()["pats"]
    kinds_of = {}
    for i, ((_, ui, _),) in lp.fast.items():
        kinds_of.setdefault(pats[i].pattern_id, set()).add(lp.units[ui]["kind"])
    assert sum(1 for k in kinds_of.values() if len(k) == 2) >= 5  # ids with a strand of each kind
    assert any(u["nstrand"] < lp.width(u) for u in lp.units)  # padded units
    assert any(len({u["len"][s] for s in range(u["nstrand"])}) > 1 for u in lp.units)  # mixed lengths
    # a tile whose shortest strand is shorter than another strand of it
    plan = T.PatternSet.from_patterns(M.case_geometry()["pats"]).lut_plan(20)
    assert len(plan["tiles"]) == 1 and plan["tiles"][0]["lmin"] == 1
    ps = T.PatternSet.from_patterns(M.case_generic()["pats"])
    assert len(ps.lut_plan()["gen_tiles"]) >= 3 and ps.plan_stats()["n_generic_strands"] == 12
    assert not ps.lut_plan()["tiles"]  # the 5-column strand goes with its pattern_id
    ps = T.PatternSet.from_patterns(M.case_interleaved()["pats"])
    assert ps.plan_stats(mfma=True)["n_octet_strands"] > 0 and ps.plan_stats(mfma=True)["n_mfma_strands"] > 0
    plan = ps.lut_plan(20, True)
    assert any(any(plan["slot_mfma"][t["slot_begin"]:t["slot_begin"] + t["nslots"]]) for t in plan["tiles"])
    assert plan["slot_mfma"][:12] == [1, 0] * 6
    ps = T.PatternSet.from_patterns(M.case_big_group()["pats"])
    for mfma in (False, True):
        assert 20 < ps.plan_stats(mfma=mfma)["max_tile_blocks"] <= 36
    assert ps.plan_stats(tile_blocks=36)["max_tile_blocks"] > 16
    ps = T.PatternSet.from_patterns(M.refused_group())
    assert ps.plan_stats()["max_tile_blocks"] > 40  # refused at tfbs_ctx_create (test_gpu_lut_counts.py)


# ---------------------------------------------------------------------------------------
# the accessor's own argument errors
# ---------------------------------------------------------------------------------------
def test_lut_plan_argument_errors():
    case = M.case_big_group()
    ps = T.PatternSet.from_patterns(case["pats"])
    f = T.lib().tfbs_patterns_lut_plan
    cap = T._capi
    sz = cap.tfbs_lut_plan_sizes()
    assert f(None, 20, 0, None, C.byref(sz)) == TFBS_E_ARG
    assert f(ps.h, 20, 0, None, None) == TFBS_E_ARG
    assert f(ps.h, 20, 0, None, C.byref(sz)) == 0
    want = ps.lut_plan()
    assert (sz.n_tiles, sz.n_units, sz.lut_ints, sz.n_slots) == (len(want["tiles"]), len(want["units"]),
                                                                 len(want["lut"]), len(want["slot_pid"]))
    assert sz.n_tiles and sz.n_units and sz.lut_ints and sz.n_slots
    sizes = {"tiles": sz.n_tiles, "units": sz.n_units, "lut": sz.lut_ints, "slot_pid": sz.n_slots,
             "slot_mfma": sz.n_slots}
    types = {"tiles": cap.tfbs_lut_tile, "units": cap.tfbs_lut_unit, "lut": C.c_int32, "slot_pid": C.c_uint16,
             "slot_mfma": C.c_uint8}
    for name, n in sizes.items():  # one array alone: a capacity one short is refused, the exact one copies
        arr = (types[name] * n)()
        buf = cap.tfbs_lut_plan_buffers()
        setattr(buf, name, arr)
        setattr(buf, name + "_cap", n - 1)
        assert f(ps.h, 20, 0, C.byref(buf), C.byref(sz)) == TFBS_E_ARG, name
        setattr(buf, name + "_cap", n)
        assert f(ps.h, 20, 0, C.byref(buf), C.byref(sz)) == 0, name
    assert list(arr) == want["slot_mfma"]
    # generic arrays of a set that has generic strands
    ps = T.PatternSet.from_patterns(M.case_generic()["pats"])
    assert f(ps.h, 20, 0, None, C.byref(sz)) == 0 and sz.n_gen_pats == 12 and sz.gen_w_ints > 0
    buf = cap.tfbs_lut_plan_buffers()
    buf.gen_w = (C.c_int32 * sz.gen_w_ints)()
    buf.gen_w_cap = sz.gen_w_ints - 1
    assert f(ps.h, 20, 0, C.byref(buf), C.byref(sz)) == TFBS_E_ARG
    assert ps.lut_plan() == ps.lut_plan(20, False)
