"""The best sites and their TSV restated in plain Python (the yardstick of the best-site tests).

For a region, h one of its distinct haplotypes, p a pattern strand in creation order of L bases
and k one of the region's distinct non-empty inner ranges in ascending (start, end) order: window
i exists iff i + L <= len(h), its match range is [pos[i], pos[i] + L - 1], its score the hit
list's (hits_ref.pattern_scores); it belongs to k iff range_overlaps(inner_k, match).  The best
record of (h, p, k): n_windows = the windows that belong to k, score = the maximum of their
scores, window = the lowest i attaining it, start / end = that window's match range; without a
window score = INT32_MIN, window = UINT32_MAX, start = end = 0.  The list is dense and sorted by
(region, haplotype, pattern, range).  min_score and the bed multiplicity play no part.

Written from the specification, not from the library's code.  What a test expects comes from a
case's per-haplotype-id sequences (dinuc_cases "seqs"); the library's own haplotype order only
says which sequence an index stands for.
"""
import numpy as np

import hits_ref as H
from helpers import T

INT32_MIN, UINT32_MAX = -(1 << 31), (1 << 32) - 1
HEADER = ("#chrom\tregion\tbed\tinner_start\tinner_end\tname\tpattern_id\thaplotype\tcarriers\tkind\tstrand\tstart\tend\t"
          "score\tdelta\tcarrier_ids\n")
FIELDS = ("region", "haplotype", "pattern", "range", "window", "n_windows", "score", "start", "end")

_SCORES = {}


def scores_of(p, codes):
    key = (id(p), codes)
    if key not in _SCORES:
        _SCORES[key] = (p, H.pattern_scores(p, codes))  # (p kept alive: its id stays its own)
    return _SCORES[key][1]


def inner_of(reg, beds):
    """[(bed index, start, end)] of a region: select_inner_peaks, or the region's own "inner" list
    (a test that hands add_inner ranges no bed file would give, an empty one for instance)."""
    return reg["inner"] if "inner" in reg else T.select_inner_peaks(reg["merged"], beds)


def region_ranges(reg, beds):
    """The distinct non-empty inner ranges of a region, ascending (start, end)."""
    return sorted({(a, z) for _, a, z in inner_of(reg, beds) if z >= a})


def best_of(p, codes, pos, rng):
    """(window, n_windows, score, start, end) of one (sequence, strand, range)."""
    L = len(p)
    best = None
    n = 0
    for i, s in enumerate(scores_of(p, codes)):
        if T.range_overlaps(rng, (pos[i], pos[i] + L - 1)):
            n += 1
            if best is None or s > best[1]:  # (ascending i: a tie stays on the lowest window)
                best = (i, s)
    if best is None:
        return (UINT32_MAX, 0, INT32_MIN, 0, 0)
    return (best[0], n, best[1], pos[best[0]], pos[best[0]] + L - 1)


def expected_best(pats, regions, beds, order_per_region):
    """The dense best list of whole regions as tuples FIELDS, from the sequences alone;
    order_per_region[r] = [(codes, pos)] in index order."""
    out = []
    for r, (reg, order) in enumerate(zip(regions, order_per_region)):
        ranges = region_ranges(reg, beds)
        for h, (codes, pos) in enumerate(order):
            for pi, p in enumerate(pats):
                for k, rng in enumerate(ranges):
                    out.append((r, h, pi, k) + best_of(p, codes, pos, rng))
    return out


def as_array(recs):
    a = np.zeros(len(recs), dtype=T.BEST_DTYPE)
    for k, name in enumerate(FIELDS):
        a[name] = [x[k] for x in recs]
    return a


def as_tuples(a):
    return [tuple(int(x[k]) for k in FIELDS) for x in a]


def format_tsv(chrom, pats, regions, beds, order_per_region, seqs_per_region, recs, mode):
    """The issue's TSV section.  recs: tuples as expected_best makes them (any whole regions)."""
    per = {x[:4]: x for x in recs}
    pids = sorted({p.pattern_id for p in pats})
    lines = []
    for r, reg in enumerate(regions):
        if not any(x[0] == r for x in recs):
            continue
        rname = "%d-%d" % reg["merged"]
        ranges = region_ranges(reg, beds)
        ids = H.carrier_ids(seqs_per_region[r])
        order = order_per_region[r]
        keys = sorted({(a, z, bi) for bi, a, z in inner_of(reg, beds) if z >= a})

        def value(h, pid, k):
            """The best over the pattern_id's strands (creation order wins a tie), or None."""
            v = None
            for pi, p in enumerate(pats):
                x = per[(r, h, pi, k)]
                if p.pattern_id == pid and x[5] > 0 and (v is None or x[6] > v[6]):
                    v = x
            return v

        def line(a, z, bi, pid, h, kind, v, base=None):
            name = next(p.name for p in pats if p.pattern_id == pid)
            out = [chrom, rname, beds[bi][0], str(a), str(z), name, str(pid), str(h), str(len(ids[order[h]])), kind]
            if v is None:
                out += ["."] * 4
            else:
                out += ["-" if pats[v[2]].direction == T.DIR_N else "+", str(v[7]), str(v[8]), str(v[6])]
            out.append(str(v[6] - base[6]) if v is not None and base is not None else ".")
            lines.append(out + ["."])

        base = None
        if mode == "diff":
            base = min(range(len(order)), key=lambda h: (-len(ids[order[h]]), ids[order[h]][0]))
            for h, sq in enumerate(order):
                lines.append([chrom, rname] + ["."] * 5 + [str(h), str(len(ids[sq])), "hap"] + ["."] * 5 +
                             ["*" if h == base else ",".join(str(i) for i in ids[sq])])
        for a, z, bi in keys:
            k = ranges.index((a, z))
            for pid in pids:
                vals = [value(h, pid, k) for h in range(len(order))]
                if mode == "all":
                    for h, v in enumerate(vals):
                        line(a, z, bi, pid, h, "best", v)
                    continue
                vb = vals[base]
                alts = [h for h, v in enumerate(vals) if h != base and
                        ((v is None) != (vb is None) or (v is not None and v[6] != vb[6]))]
                if alts:
                    line(a, z, bi, pid, base, "base", vb)
                    for h in alts:
                        line(a, z, bi, pid, h, "alt", vals[h], vb)
    return "".join("\t".join(l) + "\n" for l in lines)
