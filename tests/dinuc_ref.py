"""Dinucleotide PWM semantics restated in plain Python (the yardstick of the dinucleotide tests).

A dinucleotide PWM covers L >= 2 bases with R = L - 1 rows of 16 int32 milli-log-odds,
row entry 4 * a + b for the pair (base a, next base b), A=0 C=1 G=2 T=3.  The window
starting at base i scores sum_{j<R} W[j][4 s[i+j] + s[i+j+1]] as a wrapping int32; a pair
in which either base is N (code 4) contributes 0; it matches iff score > min_score
(strict) and the match range is [pos[i], pos[i] + L - 1]; windows exist for i <= len - L.
The reverse strand is W'[i][4a + b] = W[R-1-i][4(3-b) + (3-a)].  Counting per inner range
uses the reference's asymmetric overlap (T.range_overlaps(inner, match)).

Written from the feature's specification, not from the library's code; never compared
with itself.
"""
import tfbs_pkg

T = tfbs_pkg.load()


def wrap32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def score(rows, codes, i):
    s = 0
    for j, row in enumerate(rows):
        a, b = codes[i + j], codes[i + j + 1]
        if a == 4 or b == 4:
            continue
        s += row[4 * a + b]
    return wrap32(s)


def scores(rows, codes):
    """The score of every window (i <= len - L)."""
    L = len(rows) + 1
    return [score(rows, codes, i) for i in range(len(codes) - L + 1)]


def matches(rows, min_score, codes, pos):
    """[(start, end)] of the matching windows, in window order."""
    L = len(rows) + 1
    return [(pos[i], pos[i] + L - 1) for i, s in enumerate(scores(rows, codes)) if s > min_score]


def reverse_rows(rows):
    R = len(rows)
    return [[rows[R - 1 - i][4 * (3 - b) + (3 - a)] for a in range(4) for b in range(4)] for i in range(R)]


def embed_mono(mono):
    """The dinucleotide rows that score every N-free window as the mono PWM `mono`
    (rows of [A, C, G, T]) does: W[j][4a+b] = m[j][a], the last row adding m[last][b]."""
    R = len(mono) - 1
    rows = [[mono[j][a] for a in range(4) for _ in range(4)] for j in range(R)]
    rows[R - 1] = [mono[R - 1][a] + mono[R][b] for a in range(4) for b in range(4)]
    return rows


def count_overlaps(ms, inner):
    """Matches `ms` counted for the inner range: those whose start or end lies inside it."""
    return sum(1 for m in ms if T.range_overlaps(inner, m))
