"""The affinity rows restated in plain Python (the yardstick of the affinity-row tests).

mlog2(x) = floor(1000 * log2(x)) for x >= 1, as (x ** 1000).bit_length() - 1 in big integers (2^m <=
x^1000 < 2^(m + 1)  <=>  m <= 1000 log2 x < m + 1), and -1 for x = 0.  Never from the committed table.

A key is the score rows': a (bed, inner range) pair with a non-empty range, taken once, in the
order (inner start, inner end, bed as registered); under it pattern_id ascends.  The value of a
haplotype for pattern id q under a key is (A, N): the sums of `sum` and of n_windows over q's
strands (affinity_ref.record_of); N == 0 is "none".  A candidate row (key, q): a "none" of any
carried haplotype means no row; else x_s = A(2s) + A(2s + 1), y_s = mlog2(x_s), lo / hi / spread of
y; no row for no sample, spread 0 or spread < min_spread (0 counts as 1).  With d = y_s - lo the
field, the class counts and maf are the score rows' (score_ref.field, maf_of); the row is written
iff maf >= min_maf, numbered by a counter of written rows, its INFO
LOG2AFF=<lo>,<hi>;AFF=<min x>,<max x>;TOP=<top of q>;freqs=<zero>/<one>/<two>.

Written from the specification, not from the library's code.
"""
import functools

import affinity_ref as A
import best_ref as R
import score_ref as S


@functools.lru_cache(None)
def mlog2(x):
    assert 0 <= x < 1 << 64
    return -1 if x == 0 else (x ** 1000).bit_length() - 1


def genotypes(left, right, top, min_spread=1):
    """(maf, info, genotype text) of one candidate row's per-sample sums, or None."""
    xs = [a + b for a, b in zip(left, right)]
    if not xs:
        return None
    ys = [mlog2(x) for x in xs]
    lo, hi = min(ys), max(ys)
    spread = hi - lo
    if spread == 0 or spread < min_spread:
        return None
    cnt = [0, 0, 0]
    out = []
    for y in ys:
        text, cls = S.field(y - lo, spread)
        cnt[cls] += 1
        out.append(text)
    info = "LOG2AFF=%d,%d;AFF=%d,%d;TOP=%d;freqs=%d/%d/%d" % (lo, hi, min(xs), max(xs), top, cnt[0], cnt[1], cnt[2])
    return S.maf_of(*cnt), info, "".join(out)


def rows_of(pats, reg, beds, n, value, min_maf=0, min_spread=1):
    """[(bed name, pattern name, start, end, info, genotypes)] of one region's written rows;
    value(pid, (a, z), x) = (A, N) of haplotype id x for pattern id pid under the range."""
    tops = A.tops(pats)
    pids = sorted({p.pattern_id for p in pats})
    keys = sorted({(a, z, bi) for bi, a, z in R.inner_of(reg, beds) if z >= a})
    out = []
    for a, z, bi in keys:
        for pid in pids:
            vals = [value(pid, (a, z), x) for x in range(2 * n)]
            if n == 0 or any(v[1] == 0 for v in vals):
                continue
            first = next(i for i, p in enumerate(pats) if p.pattern_id == pid)
            g = genotypes([v[0] for v in vals[0::2]], [v[0] for v in vals[1::2]], tops[first], min_spread)
            if g is None or g[0] < min_maf:
                continue
            out.append((beds[bi][0], pats[first].name, a, z, g[1], g[2]))
    return out


def text_of(chrom, rows_per_region, pos=1):
    """(text, rows, next POS) of the regions' rows_of lists."""
    lines = []
    for rows in rows_per_region:
        for bed, name, a, z, info, gts in rows:
            lines.append("%s\t%d\t%s,%s,%d-%d\t.\t.\t.\tPASS\t%s\tGT:DS%s\n" %
                         (chrom.replace("chr", ""), pos, bed, name, a, z, info, gts))
            pos += 1
    return "".join(lines), len(lines), pos


def region_rows(pats, reg, beds, seqs, min_maf=0, min_spread=1):
    """rows_of from the sequences alone: seqs[x] = (codes, pos) of haplotype id x."""
    tops = A.tops(pats)

    @functools.lru_cache(None)
    def of_seq(pid, rng, sq):
        recs = [A.record_of(p, tops[i], sq[0], sq[1], rng) for i, p in enumerate(pats) if p.pattern_id == pid]
        return sum(r[2] for r in recs), sum(r[0] for r in recs)

    return rows_of(pats, reg, beds, len(seqs) // 2, lambda pid, rng, x: of_seq(pid, rng, seqs[x]), min_maf, min_spread)


def expected_text(chrom, pats, regions, beds, seqs_per_region, min_maf=0, min_spread=1, pos=1):
    """(text, rows, next POS) of whole regions, from the sequences alone."""
    return text_of(chrom, [region_rows(pats, reg, beds, seqs, min_maf, min_spread)
                           for reg, seqs in zip(regions, seqs_per_region)], pos)
