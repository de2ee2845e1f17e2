"""Reference-window reuse across indels, restated without segments (the yardstick of
test_reuse_cases_cpu.py and test_gpu_reuse_indels.py).

A region's reference is `ref` (codes 0-4), `m` columns from position `es`; a distinct haplotype is
what RegionBatch.haplotype gives: codes 0-4 and positions, `n` columns.  A haplotype window may
take the reference's hit (or none) exactly when it *is* a reference window: the same bases at the
same consecutive positions (equal_window).  A run list says which windows are not claimed to be
one (meets: run_meets of tfbs_internal.hpp).  Nothing here knows of segments, shifts or of how
the lists are built; `patch` restates the patcher's rules (haplotype.rs:94-156) only to say which
records a haplotype applied and which columns they wrote, for the footprint bound.
"""
END = 0xFFFFFFFF  # a run's end past the sequence's end


def equal_window(ref, es, nuc, pos, w, L):
    """q, the reference window that window w of length L of the haplotype equals (its bases and
    its positions, N compared as a code), or None."""
    m = len(ref)
    q = pos[w] - es
    if not 0 <= q <= m - L:
        return None
    for j in range(L):
        if pos[w + j] != es + q + j or nuc[w + j] != ref[q + j]:
            return None
    return q


def meets(runs, w, S):
    """Some run (a, b) meets the columns [w, w + S - 1] (b = a - 1: the windows spanning a - 1 and a)."""
    return any(a <= w + S - 1 and b >= w for a, b in runs)


def census(nuc, pos, L, rng):
    """The windows of length L with their first or their last position inside rng = (s, e) (the
    overlap rule of the count path) that hold a base other than N: the exact count of a strand
    whose weights are all 1 with min_score 0 (an N column adds 0; a hit is score > min_score)."""
    s, e = rng
    return sum(1 for w in range(len(nuc) - L + 1)
               if (s <= pos[w] <= e or s <= pos[w] + L - 1 <= e) and any(c != 4 for c in nuc[w:w + L]))


def census_ranges(nuc, pos, L, ranges):
    """[census(nuc, pos, L, rng) for rng in ranges] with the windows listed once: positions never
    decrease along a haplotype, so both ends are sorted, and first or last inside = first inside
    + last inside - both inside (both: the first position in [s, e - L + 1])."""
    import bisect
    first = [pos[w] for w in range(len(nuc) - L + 1) if any(c != 4 for c in nuc[w:w + L])]
    assert first == sorted(first)
    between = lambda lo, hi: max(0, bisect.bisect_right(first, hi) - bisect.bisect_left(first, lo))
    return [between(s, e) + between(s - L + 1, e - L + 1) - between(s, e - L + 1) for s, e in ranges]


def patch(ref, es, records):
    """The patcher's rules on a window of consecutive positions [es, es + m - 1]: records =
    [(pos, REF codes, ALT codes)] of one haplotype.  Returns (nuc, pos, applied, truncated):
    applied = [(q, len(REF), first column written, columns written)] of the records that took
    effect, q their reference column; truncated: an overlapping record ended the sequence early."""
    m = len(ref)
    ee = es + m - 1
    diffs = sorted(d for d in records if es <= d[0] <= ee)
    nuc, pos, applied = [], [], []
    at = es

    def copy(lo, hi):  # the reference's bases with positions in [lo, hi]
        for p in range(max(lo, es), min(hi, ee) + 1):
            nuc.append(ref[p - es])
            pos.append(p)

    for p, r, a in diffs:
        if p > at:
            copy(at, p - 1)
            at = p
        if p == at and len(r) == 1:  # SNV or insertion: every ALT base at the anchor's position
            assert r[0] == ref[at - es]
            applied.append((at - es, 1, len(nuc), len(a)))
            nuc.extend(a)
            pos.extend([at] * len(a))
            at += 1
        elif p == at and len(a) == 1:  # deletion: its one ALT base, then the position past REF
            applied.append((at - es, len(r), len(nuc), 1))
            nuc.append(a[0])
            pos.append(at)
            at += len(r)
        elif p == at:
            raise ValueError("neither REF nor ALT of one base")
        elif at >= ee:  # an overlapping record at the window's end: the last base, and done
            copy(at, at)
            return tuple(nuc), tuple(pos), applied, False
        else:  # an overlapping record truncates the haplotype
            return tuple(nuc), tuple(pos), applied, True
    copy(at, ee)
    return tuple(nuc), tuple(pos), applied, False


def _merged(intervals):
    out = []
    for lo, hi in sorted(intervals):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def footprints(applied, truncated, m, n):
    """The bound on either run list from the records alone: (reference-column intervals, a run
    to the end allowed there; own-column intervals, a run to the end allowed there).

    Reference columns: a record at column q with REF of r bases leaves [q, q + r - 1] and may
    separate what precedes it from what follows it at q + r, so [q, q + r].  Own columns: the
    columns the record wrote, [c, c + k - 1], and the boundary towards the next column, so
    [c, c + k].  The list builder merges runs that touch (a <= previous b + 1), so intervals that
    touch or overlap bound a run together.  A run to the end: in the reference's columns when a
    record's REF reaches the last column or past it, or when an overlapping record truncated the
    haplotype (it ends with the last applied record's columns: the reference past that record's
    REF has no counterpart); in the haplotype's own columns when a record wrote its last column."""
    rq = _merged((q, q + r) for q, r, _, _ in applied)
    own = _merged((c, c + k) for _, _, c, k in applied)
    rq_end = truncated or any(q + r >= m for q, r, _, _ in applied)
    own_end = any(c + k >= n for _, _, c, k in applied)
    return rq, rq_end, own, own_end


def inside(run, intervals, end_ok):
    """Run (a, b) lies inside one of the intervals (a boundary run (a, a - 1) as the columns
    a - 1 and a; a run to the end from its first column on, where end_ok allows one)."""
    a, b = run
    if b == END:
        return end_ok and any(lo <= a <= hi for lo, hi in intervals)
    lo_col, hi_col = min(a, b), max(a, b)
    return any(lo <= lo_col and hi_col <= hi for lo, hi in intervals)
