"""The mono PWM count path restated in plain Python, and the decoder of the LUT plan (the
yardstick of the LUT and generic scan path tests).

Spec.  A PWM strand of L columns scores the window at base i as the sum of its column weights
(an N adds 0), kept here as an unwrapped Python int; the reference's score is its int32 wrap.
The window matches iff score > min_score (strict), its range is [pos[i], pos[i] + L - 1], and
windows exist for i <= len - L.  Counts per inner range use T.range_overlaps(inner, match), per
haplotype id.

Octet rule (plan.cpp's header comment).  With (bmin, bmax) the lowest and highest sum of each
block of 4 columns, a strand is OCTET16 iff every bmax - bmin <= 32767, the sum over blocks of
max(|bmax|, |bmin|) is below 2^30, and min_score - sum(bmax) >= -32768; otherwise QUAD32.  A
pattern_id is generic iff one of its strands has more than 32 columns.

LutPlan knows the layout of PatternSet.lut_plan()'s copied words: block b of unit U of tile t is
block t.lut_begin + U.lut_off + b of 1024 ints, code c's 16 bytes at ints 4 c .. 4 c + 3; an
octet unit's strand s is half s & 1 (low first) of int s >> 1, a quad unit's strand s is int s.
decode() walks the kernel's lookup loop over them.  Written from the specification and the
layout's description, not from the planner's code; never compared with itself.
"""
import dinuc_cases as K
import dinuc_ref as D
import hits_ref as H
from helpers import T

OCTET, QUAD = 0, 1
NO_STRAND = 0xFFFFFFFF
FAST_MAX_LEN = 32


def columns(p):
    return [w.acgtn[:4] for w in p.weights]


def exact_scores(p, codes):
    """The unwrapped score of every window of PWM strand p on base codes 0-4."""
    return K.mono_scores(columns(p), codes)


def matches(p, codes, pos):
    """[(start, end)] of the matching windows, in window order."""
    L = len(p)
    return [(pos[i], pos[i] + L - 1) for i, s in enumerate(H.pattern_scores(p, codes)) if s > p.min_score]


def expected_keys(pats, n_samples, beds, reg, seqs):
    """count_matches_by_sample per haplotype id: {(bed, range, pattern_id): (L, R)} of the keys
    that some haplotype counts for; a range that a bed lists twice is counted twice."""
    inner = T.select_inner_peaks(reg["merged"], beds)
    out = {}
    for p in pats:
        per_seq = {}
        for h, seq in enumerate(seqs):
            if seq not in per_seq:
                ms = matches(p, seq[0], seq[1])
                per_seq[seq] = [D.count_overlaps(ms, (a, z)) for _, a, z in inner]
            for (bi, a, z), c in zip(inner, per_seq[seq]):
                if c:
                    lr = out.setdefault((beds[bi][0], (a, z), p.pattern_id), ([0] * n_samples, [0] * n_samples))
                    lr[h & 1][h >> 1] += c
    return out


def finish(case):
    """Adds the haplotype sequences and the model's keys of every region."""
    case["seqs"] = [K.hap_sequences(reg, case["n"]) for reg in case["regions"]]
    case["want"] = [expected_keys(case["pats"], case["n"], case["beds"], reg, sq)
                    for reg, sq in zip(case["regions"], case["seqs"])]
    return case


# ---------------------------------------------------------------------------------------
# the octet rule
# ---------------------------------------------------------------------------------------
def block_ranges(p):
    """[(bmin, bmax)] per block of 4 columns: the columns are independent, so a block's lowest
    sum is the sum of its columns' lowest weights."""
    cols = columns(p)
    return [(sum(min(c) for c in cols[b:b + 4]), sum(max(c) for c in cols[b:b + 4])) for b in range(0, len(cols), 4)]


def is_octet(p):
    br = block_ranges(p)
    return (all(hi - lo <= 32767 for lo, hi in br) and sum(max(abs(lo), abs(hi)) for lo, hi in br) < (1 << 30)
            and p.min_score - sum(hi for _, hi in br) >= -32768)


def generic_ids(pats):
    return {p.pattern_id for p in pats if p.kind == T.KIND_PWM and len(p) > FAST_MAX_LEN}


def extreme_window(p, highest):
    """The bases (codes 0-3) of the window that takes every column's highest (or lowest) weight."""
    pick = max if highest else min
    return [c.index(pick(c)) for c in columns(p)]


# ---------------------------------------------------------------------------------------
# the copied plan
# ---------------------------------------------------------------------------------------
def s16(x):
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def sat16(x):
    return max(-32768, min(32767, x))


def image_of(window, tail):
    """A 32-base image: the window's bases (codes 0-3), then `tail` repeated."""
    img = list(window)
    k = 0
    while len(img) < 32:
        img.append(tail[k % len(tail)])
        k += 1
    return img


class LutPlan:
    def __init__(self, plan):
        self.plan = plan
        self.tiles, self.units, self.lut = plan["tiles"], plan["units"], plan["lut"]
        self.fast = {}  # strand (creation order) -> [(tile, unit, s)]
        for ti, t in enumerate(self.tiles):
            for ui in range(t["first"], t["last"]):
                U = self.units[ui]
                for s in range(self.width(U)):
                    if U["orig_index"][s] != NO_STRAND:
                        self.fast.setdefault(U["orig_index"][s], []).append((ti, ui, s))
        self.gen = {}  # strand -> [(generic tile, index into gen_pats)]
        for gi, t in enumerate(plan["gen_tiles"]):
            for k in range(t["first"], t["last"]):
                self.gen.setdefault(plan["gen_pats"][k]["orig_index"], []).append((gi, k))

    @staticmethod
    def width(U):
        return 8 if U["kind"] == OCTET else 4

    def entry(self, ti, ui, s, b, code):
        """Strand s's entry for 4-mer `code` in block b of unit ui (of tile ti)."""
        U = self.units[ui]
        at = (self.tiles[ti]["lut_begin"] + U["lut_off"] + b) * 1024 + 4 * code
        if U["kind"] == OCTET:
            return s16(self.lut[at + (s >> 1)] >> (16 * (s & 1)))
        return self.lut[at + s]

    def init_half(self, ui, s):
        return s16(self.units[ui]["init"][s >> 1] >> (16 * (s & 1)))

    def decode_at(self, ti, ui, s, image):
        """The kernel's decision for strand s of unit ui on a 32-base image (codes 0-3): every
        block of the *unit* is looked up, whatever the strand's own length."""
        U = self.units[ui]
        codes = [sum(image[4 * b + j] << (2 * j) for j in range(4)) for b in range(8)]
        if U["kind"] == OCTET:
            acc = self.init_half(ui, s)
            for b in range(min(8, U["nblk"])):
                acc = sat16(acc + self.entry(ti, ui, s, b, codes[b]))
            return acc >= 0
        acc = 0
        for b in range(min(8, U["nblk"])):
            acc = D.wrap32(acc + self.entry(ti, ui, s, b, codes[b]))
        return acc > U["thr"][s]

    def decode(self, strand, image):
        (ti, ui, s), = self.fast[strand]
        return self.decode_at(ti, ui, s, image)

    def gen_columns(self, k):
        """The generic kernel's weights of gen_pats[k]: per column [A, C, G, T, N]."""
        g = self.plan["gen_pats"][k]
        w = self.plan["gen_w"]
        return [list(w[5 * (g["col_off"] + j):5 * (g["col_off"] + j) + 5]) for j in range(g["len"])]
