"""The matrix-core filter restated in plain Python, from the layout comments of mfma.cpp,
scan_mfma.hip and DESIGN.md section 3 -- never from the library's own bound.

Input: PatternSet.mfma_plan() -- the bytes of the FP6 image, the super tiles' fields and
the tiles' rescoring fields, exactly what a Scanner uploads.  Output: the digits decoded
from those bytes, the bound U of every (window, tile, strand place) of a haplotype, the
candidates "U > t0" counted as the scan kernel counts them (tfbs_ctx_scan_counters'
out[2]), and the packed two-strand output word.

Layout (mfma.cpp): a tile of depth D is D chunks of 1536 bytes; chunk kc holds columns
8 kc .. 8 kc + 7.  Lane l (0-63) holds strand place 2 (l & 31) + (l >> 5); its 192 bits are
dwords 0-3 at kc * 1536 + l * 16 and dwords 4-5 at kc * 1536 + 1024 + l * 8; element
e = 4 t + c (column 8 kc + t, base c) is the 6 bits at bit 6 e.  A code is FP6 e2m3: sign at
bit 5, two exponent bits, three mantissa bits."""
import struct

import numpy as np

STRANDS = 64          # strand places per tile
WINDOWS = 32          # windows per window tile
CHUNK_COLS = 8
CHUNK_BYTES = 1536
META_INTS = 384       # per tile: 4 ints per strand place, the pattern index at 256 + place, the depth class at 320
FIELD_BITS = 11
FIELD_BIAS = 1023
INT32_MAX = 2**31 - 1


def e2m3_times8(code5):
    """8 x the magnitude of an e2m3 value from its 5 low bits (exponent bias 1, subnormals
    at exponent 0): 0..7, 8..15, 16..30 step 2, 32..60 step 4."""
    e, m = code5 >> 3, code5 & 7
    return m if e == 0 else (8 + m) << (e - 1)


GRID8 = [e2m3_times8(c) for c in range(32)]


def _lane_bits(image, base, kc, lane):
    lo = image[base + kc * CHUNK_BYTES + lane * 16: base + kc * CHUNK_BYTES + lane * 16 + 16]
    hi = image[base + kc * CHUNK_BYTES + 1024 + lane * 8: base + kc * CHUNK_BYTES + 1024 + lane * 8 + 8]
    return int.from_bytes(lo, "little") | (int.from_bytes(hi, "little") << 128)


def seg_ends(seg):
    """Byte d - 1 of seg: the first tile deeper than d (= the tiles of depth <= d)."""
    return [(seg >> (8 * d)) & 255 for d in range(4)]


class Tile:
    """codes[place][column][base]: the 6-bit code; d8[place, column, base]: 8 x the digit
    (<= 0 when the sign is set).  The tile's rescoring fields: min_score, length, slot and
    pattern index per place (index -1: a padding place)."""

    def __init__(self, sup, index, depth, off):
        self.sup, self.index, self.depth, self.off = sup, index, depth, off


class FilterPlan:
    def __init__(self, plan):
        self.image = plan["image"]
        self.supers = plan["supers"]
        meta = plan["meta"]
        self.tiles = []
        for k, S in enumerate(self.supers):
            ends = seg_ends(S["seg"])
            off = S["img_off"]
            for t in range(S["tile_count"]):
                depth = 1 + sum(1 for d in range(4) if t >= ends[d])
                tile = Tile(k, S["tile0"] + t, depth, off)
                codes = np.zeros((STRANDS, CHUNK_COLS * depth, 4), dtype=np.int64)
                for kc in range(depth):
                    for lane in range(64):
                        place = 2 * (lane & 31) + (lane >> 5)
                        bits = _lane_bits(self.image, off, kc, lane)
                        for e in range(32):
                            codes[place, CHUNK_COLS * kc + (e >> 2), e & 3] = (bits >> (6 * e)) & 63
                tile.codes = codes
                mag = np.array(GRID8, dtype=np.int64)[codes & 31]
                tile.d8 = np.where(codes & 32, -mag, mag)
                m = meta[tile.index * META_INTS:(tile.index + 1) * META_INTS]
                tile.min_score = [m[4 * s + 0] for s in range(STRANDS)]
                tile.woff = [m[4 * s + 1] for s in range(STRANDS)]
                tile.length = [m[4 * s + 2] for s in range(STRANDS)]
                tile.slot = [m[4 * s + 3] for s in range(STRANDS)]
                tile.orig = [m[256 + s] for s in range(STRANDS)]
                tile.depth_class = m[320]
                self.tiles.append(tile)
                off += CHUNK_BYTES * depth

    def class_lmin(self):
        """Per depth class (0: nk 2, 1: nk 4) its shortest strand over all its super tiles, or 0."""
        out = [0, 0]
        for S in self.supers:
            c = 1 if S["nk"] > 2 else 0
            out[c] = min(out[c], S["lmin"]) if out[c] else S["lmin"]
        return out

    def t0(self, tile):
        return self.supers[tile.sup]["t0"]

    def place_of(self, orig):
        """(tile, place) of pattern index orig, or None (not a matrix-core strand)."""
        for tile in self.tiles:
            if orig in tile.orig:
                return tile, tile.orig.index(orig)
        return None


def acc0_value(bits):
    """The accumulator's start value (f32 bits) as an integer; it must be one."""
    f = struct.unpack("<f", struct.pack("<I", bits))[0]
    assert f == int(f)
    return int(f)


def packed(acc0_bits, u_even, u_odd):
    """The output word of a strand pair, an integer: acc0 + U_even + 2^11 U_odd."""
    return acc0_value(acc0_bits) + u_even + (u_odd << FIELD_BITS)


def fields(value):
    """(V_even, V_odd) of an output in [2^23, 2^24): mantissa bits 0-10 and 11-21."""
    assert 2**23 <= value < 2**24, value
    m = value - 2**23
    return m & 2047, (m >> FIELD_BITS) & 2047


def fires(value):
    """The kernel's test: the fields' top bits (10 and 21) of the f32's bits."""
    bits = struct.unpack("<I", struct.pack("<f", float(value)))[0]
    return bool(bits & (1 << 10)), bool(bits & (1 << 21))


def base_codes(hap):
    """'ACGTN' string -> codes 0-4."""
    return np.array(["ACGTN".index(ch) for ch in hap], dtype=np.int64)


def n_windows(n, lmin):
    return max(0, n - lmin + 1) if lmin else 0


def tile_bounds(tile, codes, nw):
    """U[w, place] of windows 0 .. nw - 1 of the haplotype `codes`: - the sum of the grid
    magnitudes over the tile's columns whose base is not N; bases past the end read as A."""
    n = len(codes)
    ncol = tile.d8.shape[1]
    idx = np.arange(nw)[:, None] + np.arange(ncol)[None, :]
    b = np.where(idx < n, codes[np.minimum(idx, max(n - 1, 0))] if n else 0, 0)
    live = b < 4
    b = np.where(live, b, 0)
    g = tile.d8[:, np.arange(ncol)[None, :], b]  # [place, window, column]
    return (g * live[None, :, :]).sum(axis=2).T


def candidates(fp, hap):
    """The candidates of one haplotype, as tfbs_matches lists and the kernel counts them:
    (count, {(pattern index, window)} of the real strands' candidates, count per class)."""
    codes = base_codes(hap)
    lmin = fp.class_lmin()
    total, real, per_class = 0, set(), [0, 0]
    for tile in fp.tiles:
        c = 1 if fp.supers[tile.sup]["nk"] > 2 else 0
        nw = n_windows(len(codes), lmin[c])
        if not nw:
            continue
        fire = tile_bounds(tile, codes, nw) > fp.t0(tile)
        total += int(fire.sum())
        per_class[c] += int(fire.sum())
        for w, s in zip(*np.nonzero(fire)):
            if tile.orig[s] >= 0:
                real.add((tile.orig[s], int(w)))
    return total, real, per_class
