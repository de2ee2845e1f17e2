"""The mutation scan and its TSV restated in plain Python (the yardstick of the mutation-scan tests).

For a region let R = patch_haplotype((es, ee), [], ref): n columns of (code, pos).  A substitution
is (c, b): a column c with R[c] in ACGT and a base b in ACGT, b != R[c]; an N column has none.  The
mutation record of (region, pattern strand p of L bases, c, b) holds what the effect record of the
SNV (pos[c], REF = R[c], ALT = b) holds: the affected windows are i with i + L <= n and
c - L + 1 <= i <= c; ref_score / ref_window are the maximum of their scores on R (signed int32) and
the lowest window attaining it, alt_score / alt_window the same on R with column c set to b; the
four positions are pos[window] and that plus L - 1; kind is the effects TSV's under the strand's
min_score.  A record exists iff the strand is a PWM or a dinucleotide PWM, it has an affected window
and its kind is in the mask.  Sorted by (region, pattern, column, alt base).

Written from the specification, not from the library's code: R comes from the oracle's
patch_haplotype, and every alt window is rescored from the substituted sequence with
hits_ref.pattern_scores, never by a delta.
"""
import numpy as np

import effects_ref as E
import hits_ref as H
from helpers import T

NUC = "ACGT"
KINDS = ("gain", "loss", "change", "same", "none")
GAIN, LOSS, CHANGE, SAME, NONE = 1, 2, 4, 8, 16
SITES, ALL = 7, 31
FIELDS = ("region", "column", "pattern", "ref", "alt", "kind", "pos", "n_windows", "ref_score", "ref_window",
          "alt_score", "alt_window", "ref_start", "ref_end", "alt_start", "alt_end")
HEADER = ("#chrom\tregion\tpos\tref\talt\tkind\tname\tpattern_id\tstrand\tref_start\tref_end\tref_score\talt_start\t"
          "alt_end\talt_score\tdelta\n")


def kind_of(p, ref_score, alt_score):
    pr, pa = ref_score > p.min_score, alt_score > p.min_score
    if pa and not pr:
        return 0
    if pr and not pa:
        return 1
    if not pr:
        return 4
    return 2 if ref_score != alt_score else 3


def best(scores, lo):
    """(maximum, lowest window attaining it) of the scores of windows lo, lo + 1, ..."""
    top = max(scores)
    return top, lo + scores.index(top)


def region_mutations(pats, reg, r, kinds=ALL):
    """The region's records as tuples in FIELDS order, sorted by (pattern, column, alt)."""
    codes, pos = E.patched(reg, [])
    n = len(codes)
    out = []
    for pi, p in enumerate(pats):
        L = len(p)
        if p.kind not in (T.KIND_PWM, T.KIND_DIPWM) or L == 0 or n < L:
            continue
        for c in range(n):
            if codes[c] == 4:
                continue
            lo, hi = max(0, c - L + 1), min(c, n - L)
            assert lo <= hi
            ref_score, ref_window = best(H.pattern_scores(p, codes[lo:hi + L]), lo)
            for b in range(4):
                if b == codes[c]:
                    continue
                alt = codes[:c] + (b,) + codes[c + 1:]
                alt_score, alt_window = best(H.pattern_scores(p, alt[lo:hi + L]), lo)  # rescored, no delta
                k = kind_of(p, ref_score, alt_score)
                if not (kinds >> k) & 1:
                    continue
                out.append((r, c, pi, codes[c], b, k, pos[c], hi - lo + 1, ref_score, ref_window, alt_score,
                            alt_window, pos[ref_window], pos[ref_window] + L - 1, pos[alt_window],
                            pos[alt_window] + L - 1))
    return out


_CACHE = {}


def expected(pats, regions, kinds=ALL, key=None):
    """The records of whole regions (region index = index in `regions`); key: a hashable name under
    which the TFBS_MUT_ALL list is computed once per process."""
    if key is not None and key in _CACHE:
        full = _CACHE[key]
    else:
        full = []
        for r, reg in enumerate(regions):
            full += region_mutations(pats, reg, r)
        if key is not None:
            _CACHE[key] = full
    return [x for x in full if (kinds >> x[5]) & 1]


def as_tuples(a):
    return [tuple(int(x[k]) for k in FIELDS) for x in a]


def as_array(rows):
    a = np.zeros(len(rows), dtype=T.MUTATION_DTYPE)
    for k, name in enumerate(FIELDS):
        a[name] = [x[k] for x in rows]
    return a


def format_tsv(chrom, pats, regions, rows):
    """One line per record tuple, in list order."""
    lines = []
    for x in rows:
        (r, _, pi, ref, alt, k, pos, _, ref_score, _, alt_score, _, rs, re_, as_, ae) = x
        p = pats[pi]
        lines.append([chrom, "%d-%d" % regions[r]["merged"], str(pos), NUC[ref], NUC[alt], KINDS[k], p.name,
                      str(p.pattern_id), "-" if p.direction == T.DIR_N else "+", str(rs), str(re_), str(ref_score),
                      str(as_), str(ae), str(alt_score), str(alt_score - ref_score)])
    return "".join("\t".join(l) + "\n" for l in lines)
