"""The cases of the mutation-scan tests that no other test has: case_edges(), the smallest shapes at
which the kernel (scan_mutscan.hip) can go wrong.  What is expected comes from mutscan_ref.py; a
case is built once per process and never modified.
"""
import functools
import random

import dinuc_cases as K
import dinuc_ref as D
from helpers import T

EDGE_COLUMNS = (1, 2, 8, 63, 64, 65, 127, 128, 129, 193)
# N per region (columns of R): column 0, the chunk boundary 62-65, the last column, a run of 3, and
# an N on each side of a scored column (20 / 22, 30 / 32)
EDGE_N = {1: (), 2: (1,), 8: (0,), 63: (62,), 64: (0, 62, 63), 65: (30, 32, 64), 127: (63, 64), 128: (62, 63, 64, 65),
          129: (0, 64, 128), 193: (20, 22, 62, 65, 100, 101, 102, 127, 128)}


def edge_region(rnd, probe, lmax, k, cols, n_samples):
    """A region whose reference window has `cols` columns: the merged range as long as the extended
    one allows, the reference cut short to cols bases, as at a contig end (case_geometry's way)."""
    merged_len = max(1, cols - 2 * (lmax - 1))
    reg = K.make_region(rnd, probe, n_samples, 10000 + 3000 * k, merged_len, 2, ref_len=cols, n_at=EDGE_N[cols], max_car=2)
    assert len(reg["ref"]) == cols <= reg["ee"] - reg["es"] + 1
    return reg


def mono(rnd, L, name, pid, calib, frac=0.7, direction=None, lo=-2000, hi=2000):
    w = [[rnd.randint(lo, hi) for _ in range(4)] for _ in range(L)]
    sc = K.mono_scores(w, calib) if len(calib) >= L else [0]
    return T.Pattern.PWM([T.Weight(*x) for x in w], name, pid, K.attained_threshold(sc, frac),
                         (T.DIR_N if pid & 1 else T.DIR_P) if direction is None else direction)


def mono_probe(lmax, n_samples):
    """A batch of a set whose longest strand has lmax columns: RegionBatch.ext sizes the regions."""
    return T.RegionBatch(T.PatternSet.from_patterns([T.Pattern.PWM([T.Weight(0, 0, 0, 0)] * lmax, "p", 0, 0)]), n_samples)


def ring_max():
    return T.mutscan_ring_max_length()


@functools.lru_cache(None)
def case_edges():
    """Two parts, each a case of its own pattern set (the long strands stay with the regions that
    need them, so that the Python model takes seconds):
      short  every region of EDGE_COLUMNS; mono strands of 1, 2, 8, 32 and 33 columns; dinucleotide
             strands of 2, 3 and 32 bases on both directions; an OtherPattern; an all-zero mono strand
             under min_score -1 (every window ties and passes: `same`, both windows max(0, c - L + 1))
             and an all-zero dinucleotide strand under min_score 0 (`none`); a strand whose min_score
             equals an attained reference best (the strict >); case_wrap's wrapping strands and a
             mono strand of wrapping weights.  The 32- and 33-base strands are longer than the
             regions of 1 to 8 columns.
      long   regions of 65, 129 and 193 columns; mono strands of 64, Lr, Lr + 1 and 2 Lr + 3 columns
             (Lr = tfbs_mutscan_ring_max_length()): both sides of the ring's limit, the slow path
             over more than one 64-window chunk, strands longer than the region of 65 columns."""
    rnd = random.Random(1717)
    n = 2
    Lr = ring_max()
    parts = {}
    # ---- short
    lmax = 33
    probe = mono_probe(lmax, n)
    regions = [edge_region(rnd, probe, lmax, k, cols, n) for k, cols in enumerate(EDGE_COLUMNS)]
    calib = [c for c in K.codes_of(regions[-1]["ref"]) if c != 4]
    pats = [mono(rnd, L, "m%d" % L, pid, calib) for pid, L in enumerate((1, 2, 8, 32, 33))]
    pid = len(pats)
    for L in (2, 3, 32):
        pats += K.both_strands(rnd, pid, L, calib, frac=0.7)
        pid += 1
    pats.append(T.Pattern.OtherPattern("other", pid))
    pats.append(T.Pattern.PWM([T.Weight(0, 0, 0, 0)] * 5, "zero_mono", pid + 1, -1))
    pats.append(T.Pattern.DiPWM([[0] * 16] * 3, "zero_di", pid + 2, 0))
    # min_score = the best score a window of the 63-column region attains: its columns' reference
    # side does not pass (strict >), a substitution scoring higher does
    w8 = [w.acgtn[:4] for w in pats[2].weights]
    top = max(K.mono_scores(w8, K.codes_of(regions[3]["ref"])))
    pats.append(T.Pattern.PWM(pats[2].weights, "m8_at_best", pid + 3, top))
    wrap = K.wrap_strands(rnd, calib, lengths=(2, 13, 32))
    for p in wrap:
        p.pattern_id += pid + 4
    pats += wrap
    pid += 4 + len(wrap)
    big = [[rnd.choice(K.BIG) if rnd.random() < 0.35 else rnd.randint(-3, 3) for _ in range(4)] for _ in range(8)]
    pats.append(T.Pattern.PWM([T.Weight(*x) for x in big], "wrap_mono", pid,
                              K.attained_threshold([D.wrap32(v) for v in K.mono_scores(big, calib)], 0.6)))
    parts["short"] = {"pats": pats, "n": n, "regions": regions, "beds": [("a.bed", [r["merged"] for r in regions])]}
    # ---- long
    lengths = (64, Lr, Lr + 1, 2 * Lr + 3)
    lmax = max(lengths)
    probe = mono_probe(lmax, n)
    regions = [edge_region(rnd, probe, lmax, 20 + k, cols, n) for k, cols in enumerate((65, 129, 193))]
    calib = [c for c in K.codes_of(regions[-1]["ref"]) if c != 4]
    pats = [mono(rnd, L, "m%d" % L, pid, calib, frac=0.5) for pid, L in enumerate(lengths)]
    parts["long"] = {"pats": pats, "n": n, "regions": regions, "beds": [("a.bed", [r["merged"] for r in regions])]}
    return parts


@functools.lru_cache(None)
def case_special_region():
    """test_gpu_effects' `special` region of 124 columns (an N inside, no indel in R) under that
    case's strands, each with a threshold that about two thirds of its reference windows pass: more
    substitutions leave both sides passing, so `same` occurs often enough."""
    import hits_ref as H
    import test_gpu_effects as TE
    case = TE.case_special()
    codes = K.codes_of(case["regions"][0]["ref"])
    pats = [T.Pattern(p.name, p.pattern_id, p.weights, K.attained_threshold(H.pattern_scores(p, codes), 0.33),
                      p.direction, p.kind) for p in case["pats"]]
    return {"pats": pats, "n": case["n"], "regions": case["regions"], "beds": case["beds"]}
