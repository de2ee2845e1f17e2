"""The score rows restated in plain Python (the yardstick of the score-row tests).

A key is a (bed, inner range) pair with a non-empty range, taken once, in the order (inner start,
inner end, bed as registered); under it pattern_id ascends.  B(x, q, key), the value of haplotype
id x for pattern id q: the best record (best_ref.best_of, brute force) over q's strands in creation
order, the highest score, a tie to the earlier strand, a strand with n_windows == 0 never; None
when every strand has n_windows == 0.  A candidate row (key, q): x_s = B(2s) + B(2s + 1); a None of
any carried haplotype means no row.  lo / hi / spread; no row for no sample, spread 0 or spread <
min_spread.  With d = x_s - lo the field is 0|0:0.0 (d == 0), 1|1:2.0 (d == spread), else the class
by 4 d against spread and 3 spread with DS = t / 10000, t = round_half_even(20000 d / spread), on
four decimals.  maf is counts_as_genotypes' rule on the class counts; the row is written iff maf >=
min_maf, numbered by a counter of written rows.

Written from the specification with fractions and plain ints, not from the library's code.  What a
test expects comes from a case's per-haplotype-id sequences (dinuc_cases "seqs").
"""
from fractions import Fraction

import best_ref as R


def field(d, spread):
    """(text, class 0 / 1 / 2) of one sample."""
    assert 0 <= d <= spread and spread > 0
    if d == 0:
        return "\t0|0:0.0", 0
    if d == spread:
        return "\t1|1:2.0", 2
    if 4 * d < spread:
        gt, cls = "0|0", 0
    elif 4 * d < 3 * spread:
        gt, cls = "0|1", 1
    else:
        gt, cls = "1|1", 2
    t = round(Fraction(20000 * d, spread))  # (a Fraction rounds half to even)
    assert 0 <= t <= 20000
    return "\t%s:%d.%04d" % (gt, t // 10000, t % 10000), cls


def maf_of(zero, one, two):
    if zero >= one and zero >= two:
        return one + two
    if two >= zero and two >= one:
        return zero + one
    return zero + two


def genotypes(left, right, min_spread=1):
    """(maf, info, genotype text) of one candidate row's per-sample values, or None."""
    xs = [a + b for a, b in zip(left, right)]
    if not xs:
        return None
    lo, hi = min(xs), max(xs)
    spread = hi - lo
    if spread == 0 or spread < min_spread:
        return None
    cnt = [0, 0, 0]
    out = []
    for x in xs:
        text, cls = field(x - lo, spread)
        cnt[cls] += 1
        out.append(text)
    return maf_of(*cnt), "SCORES=%d,%d;freqs=%d/%d/%d" % (lo, hi, cnt[0], cnt[1], cnt[2]), "".join(out)


def value(pats, pid, codes, pos, rng):
    """B of one haplotype sequence: the best score over pid's strands, or None."""
    v = None
    for p in pats:
        if p.pattern_id != pid:
            continue
        _, n, s, _, _ = R.best_of(p, codes, pos, rng)
        if n > 0 and (v is None or s > v):
            v = s
    return v


def region_rows(pats, reg, beds, seqs, min_maf=0, min_spread=1):
    """[(bed name, pattern name, start, end, info, genotypes)] of one region's written rows;
    seqs[x] = (codes, pos) of haplotype id x."""
    pids = sorted({p.pattern_id for p in pats})
    keys = sorted({(a, z, bi) for bi, a, z in R.inner_of(reg, beds) if z >= a})
    n = len(seqs) // 2
    distinct = sorted(set(seqs))
    out = []
    for a, z, bi in keys:
        for pid in pids:
            per = {sq: value(pats, pid, sq[0], sq[1], (a, z)) for sq in distinct}
            if n == 0 or any(per[sq] is None for sq in seqs):
                continue
            g = genotypes([per[seqs[2 * s]] for s in range(n)], [per[seqs[2 * s + 1]] for s in range(n)], min_spread)
            if g is None or g[0] < min_maf:
                continue
            name = next(p.name for p in pats if p.pattern_id == pid)
            out.append((beds[bi][0], name, a, z, g[1], g[2]))
    return out


def expected_text(chrom, pats, regions, beds, seqs_per_region, min_maf=0, min_spread=1, pos=1):
    """(text, rows, next POS) of whole regions."""
    lines = []
    for reg, seqs in zip(regions, seqs_per_region):
        for bed, name, a, z, info, gts in region_rows(pats, reg, beds, seqs, min_maf, min_spread):
            lines.append("%s\t%d\t%s,%s,%d-%d\t.\t.\t.\tPASS\t%s\tGT:DS%s\n" %
                         (chrom.replace("chr", ""), pos, bed, name, a, z, info, gts))
            pos += 1
    return "".join(lines), len(lines), pos
