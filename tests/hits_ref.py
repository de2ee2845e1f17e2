"""The hit list and its TSV restated in plain Python (the yardstick of the hit list tests).

For a region, the hit list is every (distinct haplotype, pattern strand in creation order,
window i) with i + L <= len and score > min_score; score is the wrapping int32 column sum of a
mono PWM (an N column adds 0; dinuc_cases.mono_scores) or the wrapping int32 pair sum of a
dinucleotide PWM (dinuc_ref.scores); the match range is [pos[i], pos[i] + L - 1]; hits are
sorted by (region, haplotype, pattern, window).  The TSV is written from the issue's section 4.

Written from the specification, not from the library's code.  What a test expects comes from a
case's per-haplotype-id sequences (dinuc_cases "seqs"); the library's own haplotype order only
says which sequence an index stands for.
"""
import collections

import numpy as np

import dinuc_cases as K
import dinuc_ref as D
from helpers import T

HEADER = "#chrom\tregion\thaplotype\tcarriers\tkind\tname\tpattern_id\tstrand\tstart\tend\tscore\tcarrier_ids\n"


def pattern_scores(p, codes):
    """The wrapped score of every window of pattern p on base codes 0-4 ([] when none fits)."""
    if p.kind == T.KIND_DIPWM:
        return D.scores(p.weights, codes) if len(codes) >= len(p) else []
    if p.kind != T.KIND_PWM or len(p) == 0 or len(codes) < len(p):
        return []
    return [D.wrap32(v) for v in K.mono_scores([w.acgtn[:4] for w in p.weights], codes)]


_CACHE = {}


def sequence_hits(pats, codes, pos):
    """[(pattern index, window, start, end, score)] of one sequence, in (pattern, window) order."""
    key = (id(pats), codes, pos)
    if key not in _CACHE:
        out = []
        for pi, p in enumerate(pats):
            L = len(p)
            for i, s in enumerate(pattern_scores(p, codes)):
                if s > p.min_score:
                    out.append((pi, i, pos[i], pos[i] + L - 1, s))
        _CACHE[key] = (pats, out)  # (pats kept alive: its id stays its own)
    return _CACHE[key][1]


def carrier_ids(seqs):
    """{(codes, pos): ascending haplotype ids} of one region's per-id sequences."""
    out = collections.OrderedDict()
    for hid, sq in enumerate(seqs):
        out.setdefault(sq, []).append(hid)
    return out


def library_order(b, region):
    """[(codes, pos)] of the region's distinct haplotypes in the library's index order."""
    return [b.haplotype(region, h)[:2] for h in range(b.region_stats(region)[0])]


def expected_hits(pats, order_per_region):
    """The hit list of whole regions as tuples (region, haplotype, pattern, window, start, end,
    score), from the sequences alone; order_per_region[r] = [(codes, pos)] in index order."""
    out = []
    for r, order in enumerate(order_per_region):
        for h, (codes, pos) in enumerate(order):
            out += [(r, h) + x for x in sequence_hits(pats, codes, pos)]
    return out


def as_array(hits):
    a = np.zeros(len(hits), dtype=T.HIT_DTYPE)
    for k, name in enumerate(("region", "haplotype", "pattern", "window", "start", "end", "score")):
        a[name] = [x[k] for x in hits]
    return a


def as_tuples(a):
    return [tuple(int(x[k]) for k in ("region", "haplotype", "pattern", "window", "start", "end", "score")) for x in a]


def format_tsv(chrom, pats, regions, order_per_region, seqs_per_region, hits, mode):
    """Section 4 of the specification.  hits: tuples as expected_hits makes them."""
    per = collections.defaultdict(list)
    for x in hits:
        per[(x[0], x[1])].append(x)
    lines = []

    def pattern_fields(x):
        p = pats[x[2]]
        return [p.name, str(p.pattern_id), "-" if p.direction == T.DIR_N else "+", str(x[4]), str(x[5]), str(x[6])]

    for r, reg in enumerate(regions):
        rname = "%d-%d" % reg["merged"]
        ids = carrier_ids(seqs_per_region[r])
        order = order_per_region[r]
        if mode == "all":
            for h, sq in enumerate(order):
                for x in per[(r, h)]:
                    lines.append([chrom, rname, str(h), str(len(ids[sq])), "hit"] + pattern_fields(x) + ["."])
            continue
        # the baseline: most carrier ids, ties to the haplotype holding the lowest id
        base = min(range(len(order)), key=lambda h: (-len(ids[order[h]]), ids[order[h]][0])) if order else None
        for h, sq in enumerate(order):
            head = [chrom, rname, str(h), str(len(ids[sq]))]
            mine = per[(r, h)]
            if h == base:
                lines.append(head + ["hap"] + ["."] * 6 + ["*"])
                lines += [head + ["base"] + pattern_fields(x) + ["."] for x in mine]
                continue
            lines.append(head + ["hap"] + ["."] * 6 + [",".join(str(i) for i in ids[sq])])
            theirs = per[(r, base)]
            key = lambda x: (x[2], x[4], x[5])
            n_h = collections.Counter(key(x) for x in mine)
            n_b = collections.Counter(key(x) for x in theirs)
            for kind, own, other in (("gain", mine, n_b), ("loss", theirs, n_h)):
                seen = collections.Counter()
                for x in own:  # (pattern, window) order; the last n_own - n_other under a key
                    if seen[key(x)] >= other[key(x)]:
                        lines.append(head + [kind] + pattern_fields(x) + ["."])
                    seen[key(x)] += 1
    return "".join("\t".join(l) + "\n" for l in lines)


def diff_counts(hits, order, seqs, region=0):
    """(gains + losses, repeated (pattern, start, end) keys) of one region under the multiset rule."""
    ids = carrier_ids(seqs)
    per = collections.defaultdict(list)
    for x in hits:
        if x[0] == region:
            per[x[1]].append((x[2], x[4], x[5]))
    base = min(range(len(order)), key=lambda h: (-len(ids[order[h]]), ids[order[h]][0]))
    nb = collections.Counter(per[base])
    changed = repeated = 0
    for h in range(len(order)):
        nh = collections.Counter(per[h])
        repeated += sum(1 for v in nh.values() if v > 1)
        if h != base:
            changed += sum((nh - nb).values()) + sum((nb - nh).values())
    return changed, repeated


def fold_keys(pats, n_samples, beds, merged, hits, membership):
    """count_matches_by_sample from a region's hits: {(bed, range, pattern_id): (L, R)} through
    select_inner_peaks, range_overlaps(inner, match), the bed multiplicity (a range listed twice
    counts twice) and the membership (haplotype id -> distinct index)."""
    inner = T.select_inner_peaks(merged, beds)
    per_hap = collections.defaultdict(collections.Counter)  # distinct index -> {(inner index, pattern_id): count}
    for x in hits:
        pid = pats[x[2]].pattern_id
        for k, (_, a, z) in enumerate(inner):
            if T.range_overlaps((a, z), (x[4], x[5])):
                per_hap[x[1]][(k, pid)] += 1
    out = {}
    for hid, h in enumerate(membership):
        for (k, pid), c in per_hap[h].items():
            bi, a, z = inner[k]
            lr = out.setdefault((beds[bi][0], (a, z), pid), ([0] * n_samples, [0] * n_samples))
            lr[hid & 1][hid >> 1] += c
    return out
