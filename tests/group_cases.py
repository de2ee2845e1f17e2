"""Cases that put the haplotype grouper (build_gpu.hip; group_host.cpp) at its limits.

A case is a list of calls on one grouper handle, a call is (H, regions), a region is
its records, a record the ascending haplotype ids carrying it (its rank is its index).
Everything is literal or a closed formula: no random numbers.  Every case states what
it is there to reach in `claims`; tests/test_group_cases_cpu.py proves each claim
from tests/group_ref.py alone, so a case cannot silently stop reaching its limit.

claims:
  "G"         per call, per region: the distinct masks, None for an overflow
  "free"      {(call, region): the ids without a mask (their row entry is G)}
  "masks"     {(call, region): the masks in Vec<Diff> order, written out by hand}
  "count"     {(call, region, mask): its carriers}
  "slots"     {slot: how many of the region's masks hash there} for (call 0, region 0)
  "occupied"  the LDS slots the masks of (call 0, region 0) end up in
"""
import group_ref as R


def _nonempty(records):
    return [r for r in records if r]


def from_masks(n_rec, by_id):
    """{id: ranks} -> the records' carrier lists."""
    recs = [[] for _ in range(n_rec)]
    for h in sorted(by_id):
        for k in by_id[h]:
            recs[k].append(h)
    assert all(recs), "a record without a carrier"
    return recs


def bits(m):
    return [k for k in range(64) if m >> k & 1]


def mask(*rk):
    return sum(1 << k for k in rk)


# ---- row geometry -------------------------------------------------------------------
def some(H):  # id 0 has a mask, the last id has none (the row ends in G)
    return _nonempty([[h for h in range(H - 1) if h % 3 == 0], [h for h in range(H - 1) if h % 2 == 1]])


def full(H):  # every id has a mask (no entry is G)
    return [list(range(0, H, 2)), list(range(1, H, 2)), list(range(0, H, 5))]


def tail(H):  # id 0 has none, the last id has one (the row ends in a group's index)
    return [[H - 1], [h for h in range(1, H) if h % 4 == 1 or h == H - 1]]


def _rows_case(H):
    return {"calls": [(H, [some(H), full(H), tail(H)])],
            "claims": {"G": [[1, 2, 1] if H == 2 else [3, 4, 2]],
                       "free": {(0, 1): [], (0, 2): [h for h in range(H - 1) if h % 4 != 1]}}}


# ---- order --------------------------------------------------------------------------
_ORDER_IDS = {0: [0], 1: [0, 1], 2: [0, 63], 3: [1], 4: [62, 63], 5: [63], 6: list(range(64)),
              7: list(range(63)), 8: list(range(1, 64)), 59: [0, 63], 60: list(range(64))}
_ORDER_IDS.update({i: [i - 7] for i in range(9, 59)})  # singles {2} .. {51}
ORDER_MASKS = ([mask(0), mask(0, 1), mask(*range(63)), mask(*range(64)), mask(0, 63), mask(1),
                mask(*range(1, 64))] + [mask(k) for k in range(2, 52)] + [mask(62, 63), mask(63)])

# ---- the limit ----------------------------------------------------------------------
LIMIT_H = 2048
LIMIT_A = from_masks(11, {i: bits(i) for i in range(1, 2048)})               # id 0 free
LIMIT_B = from_masks(11, {i: bits(i if i else 5) for i in range(2048)})      # id 0 repeats id 5's mask
LIMIT_C = LIMIT_A + [[0]]                                                     # id 0 alone on a 12th record
FIVE = [list(range(k, LIMIT_H, 7 + k)) for k in range(5)]
FIVE_B = [list(range(3 * k + 1, LIMIT_H, 11 + 2 * k)) for k in range(5)]

# ---- probing ------------------------------------------------------------------------
_KINV = pow(R.HASH_K, -1, 1 << 64)
PROBE_MASKS = []
for _i in range(40):
    for _s in (8190, 8191):
        _t = (_s << 51) | (0x2545F4914F6CD * (2 * _i + 1) * (_s - 8188) & ((1 << 51) - 1))  # the product m * K
        PROBE_MASKS.append(_t * _KINV & R.M64)
PROBE_H = 200
_probe_ids, _next = {}, 0
for _j, _m in enumerate(PROBE_MASKS):
    for _ in range(1 + _j % 3):
        _probe_ids[_next] = bits(_m)
        _next += 1
assert _next <= PROBE_H
PROBE = from_masks(64, _probe_ids)


# ---- a sequence on one handle -------------------------------------------------------
def seq_region(H, r):
    return [list(range((r + k) % 5, H, 3 + k + r % 3)) for k in range(3 + r % 4)]


CASES = {
    "empty_first": {"calls": [(10, [[], some(10), full(10)])], "claims": {"G": [[0, 3, 4]]}},
    "empty_middle": {"calls": [(10, [some(10), [], full(10)])], "claims": {"G": [[3, 0, 4]]}},
    "empty_last": {"calls": [(10, [some(10), full(10), []])], "claims": {"G": [[3, 4, 0]]}},
    "empty_only": {"calls": [(6, [[], []])], "claims": {"G": [[0, 0]], "free": {(0, 0): list(range(6))}}},
    "order": {"calls": [(64, [from_masks(64, _ORDER_IDS)])],
              "claims": {"G": [[59]], "masks": {(0, 0): ORDER_MASKS}, "free": {(0, 0): [61, 62, 63]},
                         "count": {(0, 0, mask(0, 63)): 2, (0, 0, mask(*range(64))): 2, (0, 0, mask(63)): 1}}},
    "limit_a_2047_masks": {"calls": [(LIMIT_H, [LIMIT_A])], "claims": {"G": [[2047]], "free": {(0, 0): [0]}}},
    "limit_b_2047_masks_no_reference": {"calls": [(LIMIT_H, [LIMIT_B])],
                                        "claims": {"G": [[2047]], "free": {(0, 0): []}, "count": {(0, 0, 5): 2}}},
    "limit_c_2048_masks": {"calls": [(LIMIT_H, [LIMIT_C])], "claims": {"G": [[None]]}},
    "limit_d_overflow_between": {"calls": [(LIMIT_H, [LIMIT_A, LIMIT_C, FIVE])],
                                 "claims": {"G": [[2047, None, 25]], "free": {(0, 0): [0]}}},
    "limit_e_call_after_overflow": {"calls": [(LIMIT_H, [LIMIT_A, LIMIT_C, FIVE]), (LIMIT_H, [FIVE_B, FIVE, LIMIT_B])],
                                    "claims": {"G": [[2047, None, 25], [23, 25, 2047]]}},
    "probing": {"calls": [(PROBE_H, [PROBE])],
                "claims": {"G": [[80]], "slots": {8190: 40, 8191: 40}, "occupied": {8190, 8191} | set(range(78)),
                           "free": {(0, 0): list(range(159, 200))}}},
    "sequence": {"calls": [(2048, [seq_region(2048, r) for r in range(40)]), (10, [seq_region(10, 1)]),
                           (2048, [seq_region(2048, 100 + r) for r in range(80)])],
                 "claims": {"G": None, "regions": [40, 1, 80]}},
}
for _H in (2, 6, 10, 2046, 3002, 8, 16):
    CASES["rows_H%d" % _H] = _rows_case(_H)

# the constructions hold whatever the grouper does
assert len(set(PROBE_MASKS)) == 80 and all(PROBE_MASKS)
assert sorted(R.slot(m) for m in PROBE_MASKS) == [8190] * 40 + [8191] * 40, "the kernel's hash changed: rebuild PROBE_MASKS"
assert len(PROBE) == 64
assert all(len(r) == 1024 for r in LIMIT_A) and len(LIMIT_C) == 12


# ---- the same limits through a batch ------------------------------------------------
def snv_region(T, lmax, n_samples, j, records):
    """Carrier lists as one SNV-only region: record k an SNV at the k-th of ascending
    positions, so its rank in Vec<Diff> order is k."""
    base = T.SynthRegion(77, j, n_samples, lmax)
    s, e = base.merged
    es = s - lmax + 1
    recs = []
    for k, car in enumerate(records):
        rb = base.ref[2 + 2 * k]
        recs.append(("car", es + 2 + 2 * k, rb, "ACGT"[("ACGT".index(rb) + 1) % 4], car))
    return {"merged": (s, e), "ref": base.ref, "records": recs}


def fill(T, b, beds, regions):
    for reg in regions:
        s, e = reg["merged"]
        b.begin(s, e, reg["ref"])
        for (bi, a, z) in T.select_inner_peaks((s, e), beds):
            b.add_inner(bi, a, z)
        for rec in reg["records"]:
            if rec[0] == "car":
                b.add_record_carriers(rec[1], rec[2], rec[3], rec[4])
            else:
                b.add_record_gt(rec[1], rec[2], rec[3], rec[4], rec[5])
        b.end()


def batch_pair(T, ps, n_samples, regions, build_device, held=True):
    """(the plain host batch, the batch grouped on build_device) of the same regions; the
    second built held, in one release, unless held is False."""
    beds = [("synthetic.bed", [reg["merged"] for reg in regions])]
    out = []
    for dev in (None, build_device):
        b = T.RegionBatch(ps, n_samples, build_device=dev)
        for name, _ in beds:
            b.add_bed(name)
        if dev is not None and held:
            with b.hold():
                fill(T, b, beds, regions)
                assert b.num_regions == 0  # not part of the batch before the release
        else:
            fill(T, b, beds, regions)
        out.append(b)
    return out


def same_batches(host, dev):
    """Digests (haplotypes, packed bases, carrier counts, reference group, keys and
    membership), counts and stats of dev are the host batch's."""
    assert dev.num_regions == host.num_regions
    for r in range(host.num_regions):
        assert dev.input_digest(r) == host.input_digest(r), r
        assert dev.region_stats(r) == host.region_stats(r), r
        assert dev.membership(r) == host.membership(r), r
    assert dev.num_haplotypes == host.num_haplotypes
    assert dev.num_windows == host.num_windows
    assert dev.num_effective_windows == host.num_effective_windows
    assert dev.num_scan_windows == host.num_scan_windows
    assert dev.num_cell_ops == host.num_cell_ops
