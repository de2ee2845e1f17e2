"""Reference of the haplotype grouper (build_gpu.hip, group_host.cpp) in plain Python:
from a region's carrier lists (one per record, a record's rank its index) every
haplotype id's diff mask, the distinct non-zero masks in Vec<Diff> order -- their
ascending rank lists compared as Python lists, with no bit arithmetic on the masks --
the carriers per mask and the membership row.  slot() and probe_slots() restate the
kernel's LDS table only so that cases can be built to collide in it."""

G_MAX = 2047  # kGrpMax (batch.hpp): more distinct masks overflow
SLOTS = 8192  # kGrpSlots (build_gpu.hip)
HASH_K = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def ranks(mask):
    return [k for k in range(64) if mask >> k & 1]


def id_masks(H, records):
    m = [0] * H
    for k, rec in enumerate(records):
        for h in rec:
            m[h] |= 1 << k
    return m


def group(H, records):
    """-> (G, masks, counts, row); (None, [], [], None) for an overflowing region."""
    m = id_masks(H, records)
    distinct = sorted({x for x in m if x}, key=ranks)
    G = len(distinct)
    if G > G_MAX:
        return None, [], [], None
    index = {x: i for i, x in enumerate(distinct)}
    counts = [0] * G
    for x in m:
        if x:
            counts[index[x]] += 1
    return G, distinct, counts, [index.get(x, G) for x in m]


def slot(m):
    return ((m * HASH_K & M64) >> 51) & (SLOTS - 1)


def probe_slots(masks):
    """The slots that distinct masks occupy after linear probing from slot(m) (the same
    set in whatever order they are inserted), and the longest probe of an insertion in
    the given order."""
    used, longest = {}, 0
    for m in masks:
        s, n = slot(m), 0
        while s in used and used[s] != m:
            s, n = (s + 1) & (SLOTS - 1), n + 1
        used[s] = m
        longest = max(longest, n)
    return set(used), longest
