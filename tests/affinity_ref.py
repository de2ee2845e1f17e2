"""The binding affinity and its TSV restated in plain Python (the yardstick of the affinity tests).

Weight: a(d) = floor(2^40 * exp(-d / 1000)) for an integer d >= 0, from decimal at 80 digits and
never from the committed tables.  Reference score: top(q) of a pattern_id q = the maximum over
q's PWM and dinucleotide strands of the sum over columns (rows) of max(0, the column's four (the
row's 16) weights).  Record of (distinct haplotype h, strand p, range k), with h, p, k, window
existence, match range and range membership the best sites' (best_ref.py): n_windows = the
windows that belong to k, n_nonzero = those with a(top - score) > 0, sum = the sum of a(top -
score) over them.  The value of (h, pattern_id, key): A = the sum of `sum`, N = the sum of
n_windows over the id's strands; N == 0 is "none".

Written from the specification, not from the library's code.  What a test expects comes from a
case's per-haplotype-id sequences; the library's own haplotype order only says which sequence an
index stands for.
"""
import functools
from decimal import ROUND_FLOOR, Context, Decimal

import numpy as np

import best_ref as R
import hits_ref as H
from helpers import T

INT32_MAX = (1 << 31) - 1
HEADER = ("#chrom\tregion\tbed\tinner_start\tinner_end\tname\tpattern_id\thaplotype\tcarriers\tkind\ttop\tn_windows\t"
          "affinity\tdelta\tcarrier_ids\n")
FIELDS = ("region", "haplotype", "pattern", "range", "n_windows", "n_nonzero", "sum")
_CTX = Context(prec=80)
_Q40 = Decimal(1 << 40)


@functools.lru_cache(None)
def weight_exact(d):
    """a(d) straight from the definition."""
    x = _CTX.multiply(_Q40, _CTX.exp(_CTX.divide(Decimal(-d), Decimal(1000))))
    return int(x.to_integral_value(ROUND_FLOOR, context=_CTX))


# 1000 ln 2^40 = 27725.89: the first d with 2^40 exp(-d / 1000) < 1.  exp falls, so a(d) = 0 from there on.
ZERO_FROM = 27726
assert weight_exact(ZERO_FROM - 1) == 1 and weight_exact(ZERO_FROM) == 0


def weight(d):
    assert d >= 0
    return 0 if d >= ZERO_FROM else weight_exact(d)


def strand_columns(p):
    """The strand's columns (rows) as lists of the weights a base (a pair) without N can take."""
    if p.kind == T.KIND_DIPWM:
        return [list(r) for r in p.weights]
    if p.kind == T.KIND_PWM:
        return [list(w.acgtn[:4]) for w in p.weights]
    return None


def tops(pats):
    """One value per strand: its pattern_id's top, 0 for an OtherPattern.  ValueError naming the
    strand when its sums can wrap int32 (sum over columns of max(|lo|, |hi|) > INT32_MAX)."""
    per = {}
    for p in pats:
        cols = strand_columns(p)
        if cols is None:
            continue
        if sum(max(abs(min(c)), abs(max(c))) for c in cols) > INT32_MAX:
            raise ValueError("the scores of strand '%s' (%s) can wrap int32" % (p.name, "-" if p.direction == T.DIR_N else "+"))
        per[p.pattern_id] = max(per.get(p.pattern_id, 0), sum(max(0, max(c)) for c in cols))
    return [per[p.pattern_id] if strand_columns(p) is not None else 0 for p in pats]


def record_of(p, top, codes, pos, rng):
    """(n_windows, n_nonzero, sum) of one (sequence, strand, range)."""
    L = len(p)
    n = nz = total = 0
    for i, s in enumerate(R.scores_of(p, codes)):
        if T.range_overlaps(rng, (pos[i], pos[i] + L - 1)):
            a = weight(top - s)
            n += 1
            nz += a > 0
            total += a
    return (n, nz, total)


def expected(pats, regions, beds, order_per_region):
    """The dense affinity list of whole regions as tuples FIELDS, from the sequences alone;
    order_per_region[r] = [(codes, pos)] in index order."""
    tp = tops(pats)
    out = []
    for r, (reg, order) in enumerate(zip(regions, order_per_region)):
        ranges = R.region_ranges(reg, beds)
        for h, (codes, pos) in enumerate(order):
            for pi, p in enumerate(pats):
                for k, rng in enumerate(ranges):
                    out.append((r, h, pi, k) + record_of(p, tp[pi], codes, pos, rng))
    return out


def as_array(recs):
    a = np.zeros(len(recs), dtype=T.AFFINITY_DTYPE)
    for k, name in enumerate(FIELDS):
        a[name] = [x[k] for x in recs]
    return a


def as_tuples(a):
    return [tuple(int(x[k]) for k in FIELDS) for x in a]


def format_tsv(chrom, pats, regions, beds, order_per_region, seqs_per_region, recs, mode):
    """The issue's TSV section.  recs: tuples as expected() makes them (any whole regions)."""
    per = {x[:4]: x for x in recs}
    tp = tops(pats)
    pids = sorted({p.pattern_id for p in pats})
    lines = []
    for r, reg in enumerate(regions):
        if not any(x[0] == r for x in recs):
            continue
        rname = "%d-%d" % reg["merged"]
        ranges = R.region_ranges(reg, beds)
        ids = H.carrier_ids(seqs_per_region[r])
        order = order_per_region[r]
        keys = sorted({(a, z, bi) for bi, a, z in R.inner_of(reg, beds) if z >= a})

        def value(h, pid, k):
            """(N, A) folded over the pattern_id's strands, or None when N == 0."""
            mine = [per[(r, h, pi, k)] for pi, p in enumerate(pats) if p.pattern_id == pid]
            n, a = sum(x[4] for x in mine), sum(x[6] for x in mine)
            return (n, a) if n else None

        def line(a, z, bi, pid, h, kind, v, base=None):
            first = next(pi for pi, p in enumerate(pats) if p.pattern_id == pid)
            out = [chrom, rname, beds[bi][0], str(a), str(z), pats[first].name, str(pid), str(h),
                   str(len(ids[order[h]])), kind, str(tp[first])]
            out += ["."] * 2 if v is None else [str(v[0]), str(v[1])]
            out.append(str(v[1] - base[1]) if v is not None and base is not None else ".")
            lines.append(out + ["."])

        base = None
        if mode == "diff":
            base = min(range(len(order)), key=lambda h: (-len(ids[order[h]]), ids[order[h]][0]))
            for h, sq in enumerate(order):
                lines.append([chrom, rname] + ["."] * 5 + [str(h), str(len(ids[sq])), "hap"] + ["."] * 4 +
                             ["*" if h == base else ",".join(str(i) for i in ids[sq])])
        for a, z, bi in keys:
            k = ranges.index((a, z))
            for pid in pids:
                vals = [value(h, pid, k) for h in range(len(order))]
                if mode == "all":
                    for h, v in enumerate(vals):
                        line(a, z, bi, pid, h, "aff", v)
                    continue
                vb = vals[base]
                alts = [h for h, v in enumerate(vals) if h != base and v != vb and
                        ((v is None) != (vb is None) or v[1] != vb[1])]
                if alts:
                    line(a, z, bi, pid, base, "base", vb)
                    for h in alts:
                        line(a, z, bi, pid, h, "alt", vals[h], vb)
    return "".join("\t".join(l) + "\n" for l in lines)
