"""Host side of the hit lists, no GPU: a region's distinct haplotypes and membership read back
from the batch (tfbs_batch_region_haplotype / _membership) against the cases' per-haplotype-id
sequences, and tfbs_batch_hits_tsv against a plain Python formatter on hits made in Python from
the reference restatements (hits_ref.py).  Integer work: every comparison is exact."""
import collections
import ctypes as C
import functools

import pytest

import dinuc_cases as K
import hits_ref as H
from helpers import T, build_batch


def case_patterns(case):
    return sorted(case.get("mono", []) + case["pats"], key=lambda p: p.pattern_id) if "mono" in case else case["pats"]


@functools.lru_cache(None)
def built(name):
    """(case, patterns, PatternSet, batch) of a case, built once and never modified."""
    case = getattr(K, name)()
    pats = case_patterns(case)
    ps = T.PatternSet.from_patterns(pats)
    return case, pats, ps, build_batch(ps, case["n"], case["beds"], case["regions"])


@pytest.mark.parametrize("name", ["case_all_kernels", "case_n_and_indels", "case_geometry"])
def test_haplotypes_and_membership(name):
    case, _, _, b = built(name)
    for r, seqs in enumerate(case["seqs"]):
        want = collections.Counter(seqs)  # {(codes, pos): carrier ids}
        got = {}
        for h in range(b.region_stats(r)[0]):
            codes, pos, carriers = b.haplotype(r, h)
            assert (codes, pos) not in got
            got[(codes, pos)] = carriers
        assert got == dict(want), r
        memb = b.membership(r)
        assert len(memb) == 2 * case["n"]
        order = H.library_order(b, r)
        assert [order[memb[hid]] for hid in range(2 * case["n"])] == list(seqs), r


def test_haplotype_short_capacity_reports_the_need():
    case, _, _, b = built("case_n_and_indels")
    need = len(b.haplotype(0, 0)[0])
    assert need > 4
    nucs, pos = (C.c_uint8 * need)(), (C.c_uint64 * need)()
    n = C.c_size_t(0)
    assert T.lib().tfbs_batch_region_haplotype(b.h, 0, 0, nucs, pos, need - 1, C.byref(n), None) == -1  # TFBS_E_ARG
    assert n.value == need
    car = C.c_uint32(0)
    assert T.lib().tfbs_batch_region_haplotype(b.h, 0, 0, nucs, pos, need, C.byref(n), C.byref(car)) == 0
    assert (tuple(nucs), tuple(pos), car.value) == b.haplotype(0, 0)
    with pytest.raises(T.TfbsError):
        b.haplotype(0, b.region_stats(0)[0])
    with pytest.raises(T.TfbsError):
        b.haplotype(b.num_regions, 0)


def test_membership_needs_keep_membership():
    case, _, ps, _ = built("case_n_and_indels")
    reg = case["regions"][0]
    b = T.RegionBatch(ps, case["n"], keep_membership=False)
    b.add_bed("a.bed")
    b.begin(reg["merged"][0], reg["merged"][1], reg["ref"])
    for rec in reg["records"]:
        b.add_record_carriers(rec[1], rec[2], rec[3], rec[4])
    b.end()
    assert b.region_stats(0)[0] == len(set(case["seqs"][0]))  # (the haplotypes are there all the same)
    with pytest.raises(T.TfbsError) as ei:
        b.membership(0)
    assert ei.value.code == -14  # TFBS_E_STATE


def tsv_inputs(name, regions=None):
    case, pats, ps, b = built(name)
    if regions is not None:  # a batch of these regions alone
        regs = [case["regions"][r] for r in regions]
        seqs = [case["seqs"][r] for r in regions]
        b = build_batch(ps, case["n"], case["beds"], regs)
    else:
        regs, seqs = case["regions"], case["seqs"]
    order = [H.library_order(b, r) for r in range(b.num_regions)]
    return pats, b, regs, order, seqs, H.expected_hits(pats, order)


@pytest.mark.parametrize("mode", ["all", "diff"])
def test_tsv_repeated_keys_and_tied_baselines(mode):
    """case_n_and_indels: an insertion gives several windows one position (repeated (pattern,
    start, end) keys: the multiset rule), the baselines of regions 0 and 1 tie on the carrier
    count (the lowest haplotype id decides)."""
    pats, b, regs, order, seqs, hits = tsv_inputs("case_n_and_indels")
    for r in range(len(regs)):  # what makes the case bite: hundreds of gains + losses, repeated keys
        changed, repeated = H.diff_counts(hits, order[r], seqs[r], r)
        assert 468 <= changed <= 785 and 9 <= repeated <= 20, (r, changed, repeated)
        assert 2877 <= sum(1 for x in hits if x[0] == r) <= 3681
    for r in (0, 1):
        sizes = sorted((len(v) for v in H.carrier_ids(seqs[r]).values()), reverse=True)
        assert sizes[0] == sizes[1], (r, sizes)
    want = H.format_tsv("chr7", pats, regs, order, seqs, hits, mode)
    assert want.count("\n") > 1000
    if mode == "diff":
        kinds = collections.Counter(l.split("\t")[4] for l in want.splitlines())
        assert min(kinds[k] for k in ("hap", "base", "gain", "loss")) >= 30, kinds
    assert b.hits_tsv(H.as_array(hits), "chr7", mode) == want
    assert b.hits_tsv(H.as_array(hits), "chr7", mode, header=True) == H.HEADER + want


@pytest.mark.parametrize("mode", ["all", "diff"])
def test_tsv_region_without_a_hit(mode):
    """case_geometry region 0 (haplotypes of 2 bases, no hit): `hap` lines only in diff mode,
    nothing in all mode."""
    pats, b, regs, order, seqs, hits = tsv_inputs("case_geometry", regions=(0,))
    assert hits == [] and len(order[0]) >= 3
    want = H.format_tsv("1", pats, regs, order, seqs, hits, mode)
    assert want.count("\n") == (len(order[0]) if mode == "diff" else 0)
    assert b.hits_tsv(H.as_array(hits), "1", mode) == want


def test_tsv_refuses_unsorted_or_foreign_hits():
    pats, b, regs, order, seqs, hits = tsv_inputs("case_n_and_indels")
    swapped = [hits[1], hits[0]] + hits[2:]
    with pytest.raises(T.TfbsError):
        b.hits_tsv(H.as_array(swapped), "chr7", "all")
    foreign = [(len(regs),) + hits[0][1:]]
    with pytest.raises(T.TfbsError):
        b.hits_tsv(H.as_array(foreign), "chr7", "diff")
