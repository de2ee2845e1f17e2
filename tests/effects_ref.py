"""The variant effects and their TSV restated in plain Python (the yardstick of the effects tests).

For a region of a batch that keeps its variants, records are numbered v = 0 .. in the order they
were added.  A record's status, tested in this order: 1 multi-allelic (n_alleles != 2), 2 no
carrier id, 3 patching it alone is refused, else 0 scored.  For a scored record
R = patch_haplotype((es, ee), [], ref) and A = patch_haplotype((es, ee), [v], ref) are sequences of
(code, pos) columns; a = their longest common prefix, z = their longest common suffix with
z <= min(len R, len A) - a.  Window i of a strand of L bases on side X of n columns is affected iff
i + L <= n, i + L > a and i < n - z.  Per side: the number of affected windows, the maximum of
their scores (hits_ref.pattern_scores: wrapped int32, an N adds 0), the lowest window attaining it
and that window's range [pos[i], pos[i] + L - 1]; a side without one holds (0, INT32_MIN,
UINT32_MAX, 0, 0).  The result is dense and sorted by (region, variant, pattern).

Written from the specification, not from the library's code: the sequences come from the oracle's
patch_haplotype.
"""
import numpy as np

import hits_ref as H
import oracle_py as O
from helpers import T

NUC = "ACGTN"
INT32_MIN, UINT32_MAX = -(1 << 31), (1 << 32) - 1
SCORED, MULTIALLELIC, NO_CARRIER, UNPATCHED = 0, 1, 2, 3
STATUS_TEXT = ["scored", "multiallelic", "no_carrier", "unpatched"]
FIELDS = ("region", "variant", "pattern", "status", "n_ref", "ref_score", "ref_window", "n_alt", "alt_score",
          "alt_window", "ref_start", "ref_end", "alt_start", "alt_end")
HEADER = ("#chrom\tregion\tvariant\tpos\tref\talt\tcarriers\tkind\tname\tpattern_id\tstrand\tref_start\tref_end\t"
          "ref_score\talt_start\talt_end\talt_score\tdelta\n")
EMPTY_SIDE = (0, INT32_MIN, UINT32_MAX)


def build_batch(pset, n_samples, beds, regions, **kw):
    """helpers.build_batch with the variants kept."""
    b = T.RegionBatch(pset, n_samples, keep_variants=True, **kw)
    for name, _ in beds:
        b.add_bed(name)
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
    return b


def record_fields(rec):
    """(pos, ref, alt, n_alleles, carrier ids) of a case's record."""
    if rec[0] == "car":
        return rec[1], rec[2], rec[3], 2, list(rec[4])
    _, pos, n_alleles, ref, alt, gt = rec
    car = []
    if n_alleles == 2:  # load_diffs: Left = Unphased(1) = raw 4, Right = Phased(1) = raw 5
        for s, g in enumerate(gt):  # one (left, right) pair of raw ints per sample
            if len(g) > 0 and g[0] == 4:
                car.append(2 * s)
            if len(g) > 1 and g[1] == 5:
                car.append(2 * s + 1)
    return pos, ref, alt, n_alleles, car


def ref_columns(reg):
    return [(c, reg["es"] + i) for i, c in enumerate(reg["ref"])]


def patched(reg, diffs):
    """(codes, positions) or a negative error."""
    hp = O.patch_haplotype((reg["es"], reg["ee"]), diffs, ref_columns(reg))
    if isinstance(hp, int):
        return hp
    return tuple(NUC.index(c) for c, _ in hp), tuple(p for _, p in hp)


def variants(reg):
    """[(pos, ref, alt, n_alleles, carriers, status)] of a region: what RegionBatch.variants gives."""
    out = []
    for rec in reg["records"]:
        pos, ref, alt, n_alleles, car = record_fields(rec)
        if n_alleles != 2:
            st = MULTIALLELIC
        elif not car:
            st = NO_CARRIER
        elif isinstance(patched(reg, [(pos, ref, alt)]), int):
            st = UNPATCHED
        else:
            st = SCORED
        out.append((pos, ref, alt, n_alleles, len(car), st))
    return out


def prefix_suffix(R, A):
    cr, ca = list(zip(*R)), list(zip(*A))
    lim = min(len(cr), len(ca))
    a = 0
    while a < lim and cr[a] == ca[a]:
        a += 1
    z = 0
    while z < lim - a and cr[len(cr) - 1 - z] == ca[len(ca) - 1 - z]:
        z += 1
    return a, z


def affected(n, L, a, z):
    """The affected windows of a side of n columns: a range."""
    return [i for i in range(max(0, n - L + 1)) if i + L > a and i < n - z]


def side(p, X, a, z):
    """(n, score, window, start, end) of pattern p on side X = (codes, positions)."""
    codes, pos = X
    L = len(p)
    if p.kind not in (T.KIND_PWM, T.KIND_DIPWM) or L == 0:
        return EMPTY_SIDE + (0, 0)
    win = affected(len(codes), L, a, z)
    if not win:
        return EMPTY_SIDE + (0, 0)
    lo, hi = win[0], win[-1]
    assert win == list(range(lo, hi + 1))
    sc = H.pattern_scores(p, codes[lo:hi + L])  # the windows lo .. hi alone
    assert len(sc) == len(win)
    top = max(sc)
    i = lo + sc.index(top)
    return len(win), top, i, pos[i], pos[i] + L - 1


def region_effects(pats, reg, r):
    """The region's block as tuples in FIELDS order, and per scored record its (R, A, a, z)."""
    out, geo = [], {}
    R = None
    for v, (pos, ref, alt, _, _, st) in enumerate(variants(reg)):
        if st == SCORED:
            if R is None:
                R = patched(reg, [])
            A = patched(reg, [(pos, ref, alt)])
            a, z = prefix_suffix(R, A)
            geo[v] = (R, A, a, z)
        for pi, p in enumerate(pats):
            if st != SCORED:
                out.append((r, v, pi, st) + EMPTY_SIDE + EMPTY_SIDE + (0, 0, 0, 0))
                continue
            sr, sa = side(p, R, a, z), side(p, A, a, z)
            out.append((r, v, pi, st) + sr[:3] + sa[:3] + sr[3:] + sa[3:])
    return out, geo


def expected_effects(pats, regions):
    out, geo = [], []
    for r, reg in enumerate(regions):
        o, g = region_effects(pats, reg, r)
        out += o
        geo.append(g)
    return out, geo


def as_tuples(a):
    return [tuple(int(x[k]) for k in FIELDS) for x in a]


def as_array(rows):
    a = np.zeros(len(rows), dtype=T.EFFECT_DTYPE)
    for k, name in enumerate(FIELDS):
        a[name] = [x[k] for x in rows]
    return a


def kind_of(p, x):
    """gain | loss | change | same | none of a record tuple under pattern p's threshold."""
    _, _, _, _, n_ref, ref_score, _, n_alt, alt_score = x[:9]
    pr = n_ref > 0 and ref_score > p.min_score
    pa = n_alt > 0 and alt_score > p.min_score
    if pa and not pr:
        return "gain"
    if pr and not pa:
        return "loss"
    if not pr:
        return "none"
    return "change" if ref_score != alt_score else "same"


def format_tsv(chrom, pats, regions, rows, mode):
    """The TSV of whole regions' record tuples (region index r = index in `regions`)."""
    lines = []
    at = 0
    while at < len(rows):
        r = rows[at][0]
        reg = regions[r]
        rname = "%d-%d" % reg["merged"]
        for v, (pos, ref, alt, _, ncar, st) in enumerate(variants(reg)):
            head = [chrom, rname, str(v), str(pos), ref or ".", alt or ".", str(ncar)]
            lines.append(head + ["var", STATUS_TEXT[st]] + ["."] * 9)
            for pi, p in enumerate(pats):
                x = rows[at]
                at += 1
                assert x[:4] == (r, v, pi, st)
                n_ref, ref_score, _, n_alt, alt_score, _, rs, re_, as_, ae = x[4:]
                if st != SCORED or n_ref + n_alt == 0:
                    continue
                kind = kind_of(p, x)
                if mode == "sites" and kind in ("same", "none"):
                    continue
                f = head + [kind, p.name, str(p.pattern_id), "-" if p.direction == T.DIR_N else "+"]
                f += [str(rs), str(re_), str(ref_score)] if n_ref else ["."] * 3
                f += [str(as_), str(ae), str(alt_score)] if n_alt else ["."] * 3
                f.append(str(alt_score - ref_score) if n_ref and n_alt else ".")
                lines.append(f)
    return "".join("\t".join(l) + "\n" for l in lines)
