"""assembly_cases.py's cases sit on the edges they are named for -- shown with the oracle's
keys and the host batch accessors alone (tfbs_batch_region_layout, tfbs_batch_region_hap_runs,
membership, haplotype; no device), so that a case that drifts off its edge fails here and
cannot pass vacuously on the GPU (test_gpu_assembly_paths.py)."""
import pytest

import assembly_cases as A

S, B = A.SHAPES["small"], A.SHAPES["big"]


def _figures(name, dedup=True):
    key = A.batch_key(name)
    hpb = int(A.case(name)["env"].get("TFBS_MFMA_HAPS_PER_BLOCK", 64))
    return A.figures(key, len(key) - 1, dedup=dedup, hpb=hpb)


def test_the_case_list_covers_the_edges():
    edges = {}
    for c in A.cases():
        edges.setdefault(c["edge"], []).append(c["side"])
    assert sorted(edges["shape"]) == [384, 385] and sorted(edges["hap_lds"]) == [512, 513]
    assert sorted(edges["walk"]) == [163, 164, 256, 257]
    assert sorted(edges["stepbits"]) == [128, 129, 256, 257]
    assert sorted(edges["refs"]) == [256, 257] and sorted(edges["dirty_listed"]) == [0, 1]
    assert sorted(edges["runs"]) == [0, 1] and sorted(edges["chunks"]) == [0, 1]
    assert sorted(edges["max_u"]) == [2048, 2049] and sorted(edges["n_inner"]) == [32, 33]
    assert sorted(edges["lmax"]) == [16319, 16320] and sorted(edges["lists"]) == [61, 62]
    assert sorted(edges["keys"]) == [16384, 16416] and sorted(edges["spill"]) == [300, 6000]
    assert "core" in edges


@pytest.mark.parametrize("kind", ["full", "short"])
def test_motifs_cannot_occur_in_the_background(kind):
    st = A.strands(kind)
    assert 8 <= A.n_ids(kind) <= 17
    for pid, _, L, motif in st:
        assert len(motif) == L and L in (1, 8, 9, 16, 17, 31, 32)
        if L == 1:
            assert motif == "A" and pid == 1
        else:  # a G at both ends: no window that is partly background matches
            assert motif[0] == "G" and motif[-1] == "G" and "A" not in motif
    if kind == "full":
        assert {L for _, _, L, _ in st} == {1, 8, 9, 16, 17, 31, 32}
        assert _literal_pwms(kind)


def _literal_pwms(kind):
    return all(p.min_score == len(p.weights) - 1 and all(sorted(w.acgtn[:4]) == [0, 0, 0, 1] for w in p.weights)
               for p in A.pattern_set(kind).to_list())


@pytest.mark.parametrize("name", A.names())
def test_no_motif_occurs_by_accident(name):
    """The reference's hits are exactly the plants; the background holds C and T only; no
    variant writes an A or a G except the one that completes a broken motif."""
    c = A.case(name)
    assert sorted(A.reference_hits(c)) == sorted(c["plants"])
    planted = set()
    for i, w in c["plants"]:
        planted.update(range(w, w + A.strands(c["kind"])[i][2]))
    loose = {ch for k, ch in enumerate(c["ref"]) if k not in planted}
    assert {ch for ch in loose if ch in "AG"} <= set("G")  # (G: only inside the broken motif of `core`)
    if name != "core":
        assert loose <= set("CT")
        for col, rlen, alt in c["variants"]:
            assert rlen == 1 and alt in ("C", "T")


@pytest.mark.parametrize("name", A.names())
def test_case_sits_on_its_edge(name):
    c = A.case(name)
    f = _figures(name)
    edge, side = c["edge"], c["side"]
    assert f["U"] == len(c["haps"]) and f["K"] == A.n_ids(c["kind"]) * f["n_inner"]
    pw = f["U"] * f["nref"]
    if edge == "shape":
        assert f["U"] == side and (side > A.BIG_U) == (side == 385)
    elif edge == "hap_lds":
        assert f["U"] == side and S["hap_lds"] == 512
    elif edge == "walk":
        want = {256: 65536, 257: 65792, 163: 65200, 164: 65600}[side]
        assert pw == want and f["nref"] <= 256 and (f["U"] > A.BIG_U) == (side < 200)
    elif edge == "stepbits":
        assert f["nref"] == (64 if name.startswith("steps64") else 128) and f["U"] == side and pw <= A.PAIR_LIMIT
        per_wave = 1  # nref >= 64: a lane per hit, one haplotype per wave and step
        steps = -(-f["U"] // (4 * per_wave)) * -(-f["nref"] // 64)
        assert (steps <= 64) == (side in (256, 128)) and steps in (64, 65, 66)
    elif edge == "refs":
        assert f["nref"] == side and S["refs"] == 256 == A.ASM["refs"]
    elif edge == "dirty_listed":
        assert f["nD"] == S["cor"] + side and pw <= A.PAIR_LIMIT and f["U"] <= A.BIG_U
    elif edge == "runs":
        assert f["nruns"] == S["runs"] + side and f["U"] == 384
    elif edge == "chunks":
        assert f["U"] == 384 and f["T"] == 512 + side and 2 * S["cnt"] // f["U"] == 16 and f["lmax"] < 16000
    elif edge == "max_u":
        assert f["U"] == side
    elif edge == "n_inner":
        assert f["n_inner"] == side
    elif edge == "lmax":
        assert f["lmax"] == side and (4 * (side + 64) < 65536) == (side == 16319) and f["U"] % 2 == side % 2
        keys = A.oracle(A.batch_key(name))[0][0]
        assert max(max(l) for l, _ in keys.values()) >= 299  # the poly-A stretch under the one-column motif
    elif edge == "spill":  # every hit an own hit (no reuse): the lists of 8 entries per wave spill the rest
        assert not f["refs_on"] and f["ent_lo"] == f["ent_hi"]
        assert (f["ent_hi"] < 4000) if side == 300 else (f["ent_hi"] > 40000)
    elif edge == "keys":
        assert f["K"] == side and f["n_inner"] == 32 and (side > A.MAX_K) == (side == 16416)
    elif edge == "lists":
        assert f["hap_begin"] % 4 != 0 and f["groups"] * 8 == (128 if side == 61 else 136) and S["lists"] == 128
    elif edge == "core":
        _core_geometry(c, f)


def _core_geometry(c, f):
    """Every strand length has a reference hit at a - L + 1 and at b (dirty) and at a - L and b + 1
    (clean) of some haplotype's run [a, b]; the helper reference, a run to the end without one
    in the haplotype's own columns, the boundary run (a, a - 1); masks of 0, 1 and 3 ranges."""
    b = A.host_batch(("core",))
    hb, U, ref_hap, _ = b.layout(0)
    assert ref_hap == hb + U  # every haplotype carries an SNV: no reference group, the helper copy
    runs = [rr for l in range(U) for rr in b.hap_runs(0, l)[2]]
    assert any(e == 0xFFFFFFFF for _, e in runs) and any(e + 1 == a for a, e in runs)
    st = A.strands("full")
    seen = {}
    for i, w in c["plants"]:
        L = st[i][2]
        for a, e in runs:
            for rel, at in (("a-L+1", a - L + 1), ("a-L", a - L), ("b", e), ("b+1", e + 1)):
                if w == at:
                    assert A.run_meets(a, e, w, L) == (rel in ("a-L+1", "b"))
                    seen.setdefault(L, set()).add(rel)
    for L in (1, 8, 9, 16, 17, 31, 32):
        assert seen[L] == {"a-L+1", "a-L", "b", "b+1"}, (L, seen.get(L))
    bits = {A.range_bits(c, w, st[i][2]) for i, w in c["plants"]}
    assert {0, 1, 3} <= bits
    assert f["ent_lo"] >= 1  # the completed motif: an own hit in a dirty window


MODES = {"default": {}, "bigu1": dict(big_u=1), "maxu0": dict(fast_max_u=0), "corlds0": dict(cor_lds=0),
         "dedup0": {}}


@pytest.mark.parametrize("name", A.names())
def test_prediction_is_determinate(name):
    """In every mode the GPU test runs, the figures' bounds leave no bit of the case's path open
    but the launch's own (tickets) and, for the indel haplotypes of `core`, nothing at all: the
    in-LDS | arena cases keep their margin."""
    c = A.case(name)
    for mode, kw in MODES.items():
        f = _figures(name, dedup=mode != "dedup0")
        P, why = A.predict(f, lists_per_group=8, **kw)
        assert [k for k, v in P.items() if v is None] == ["TICKET"], (mode, f, P)
    f = _figures(name)
    P, why = A.predict(f, lists_per_group=8)
    want = {"refs_257": 3, "maxu_2049": 0, "inner_33": 0, "keys_513": 0}.get(name)
    assert why == want
    if c["edge"] == "dirty_listed":
        assert P["DIRTY_LISTED"] == (c["side"] == 0) and P["COR_ARENA"] == (c["side"] == 1)
    if c["edge"] == "walk":
        assert P["WALK"] == (c["side"] in (257, 164))
    if c["edge"] == "runs":
        assert P["RUNS_L2"] == bool(c["side"])
    if c["edge"] == "chunks":
        assert P["CNT_ARENA"] == bool(c["side"]) and not P["COR_ARENA"]
    if c["edge"] == "lists":
        assert P["LISTS_SLICED"] == (c["side"] == 62)
    if c["edge"] == "lmax":
        assert P["U32"] == (c["side"] == 16320)


@pytest.mark.parametrize("kind", ["full", "short"])
def test_mixed_batch_predictions_are_determinate(kind):
    """All cases of a pattern set as regions of one batch: with the listed hits of every other
    region that has a haplotype in one of a region's groups counted against it, no in-LDS |
    arena decision is left open; both shapes take a dozen regions between them."""
    key = tuple(A.mixed_names(kind))
    assert sorted(key) == sorted(c["name"] for c in A.cases() if c["kind"] == kind)
    figs, preds = A.mixed_predictions(key, 8)
    for name, f, (P, why) in zip(key, figs, preds):
        assert [k for k, v in P.items() if v is None] == ["TICKET"], (name, f)
    shared = sum(1 for a, b in zip(figs, figs[1:]) if b["hap_begin"] % 64)
    assert shared >= (len(figs) // 2 if kind == "full" else 1)  # neighbours do share groups
    if kind == "full":
        assert sum(1 for f in figs if f["U"] > A.BIG_U) >= 6 and sum(1 for f in figs if f["U"] <= A.BIG_U) >= 12
        assert sorted(w for _, w in preds if w is not None) == [0, 0, 3]
        assert figs[0]["nD"] == S["cor"] and not preds[0][0]["COR_ARENA"]  # the list's limit, kept in LDS
    else:
        assert [P["CNT_ARENA"] for P, _ in preds[:2]] == [False, True]


def test_give_up_2_has_no_input():
    """The staged span of a region's runs: at most 2 048 haplotypes of 16 + 16 runs, from the
    first one's reference-column list, which lies behind its own 16."""
    assert A.MAX_U * 32 - 16 < 65536 and 16 + (A.MAX_U - 1) * 32 < 65536


def test_hap_runs_and_layout_reject_bad_indices():
    b = A.host_batch(("core",))
    with pytest.raises(Exception):
        b.layout(1)
    with pytest.raises(Exception):
        b.hap_runs(0, 31)


@pytest.mark.parametrize("name", sorted(A.CAP_CASES))
def test_arena_cases_end_where_they_say(name):
    lds, cap, want = A.CAP_CASES[name]
    P, why = A.predict(_figures(name), lists_per_group=8, cor_lds=lds, cor_cap=cap)
    assert why == want and [k for k, v in P.items() if v is None] == ["TICKET"]
    if want is None:
        assert P["COR_ARENA"] and P["DIRTY_LISTED"] == (name == "listed_3584")
    if want == 5:
        assert P["CNT_ARENA"] and P["COR_ARENA"]
