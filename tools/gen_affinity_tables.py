#!/usr/bin/env python3
"""Generates the binding affinity's constant tables.

find-tfbs_amd/csrc/affinity_tables.hpp: the 1 028 constants of the binding affinity's fixed-point
exponential (include/tfbs_amd.h, "Binding affinity"),

    T1[r] = floor(2^63 * exp(-r / 1000))   r = 0 .. 999
    T2[q] = floor(2^63 * exp(-q))          q = 0 .. 27

from Python's decimal at 80 digits.  With them a(d) = floor(2^40 * exp(-d / 1000)) is
umul64hi(T1[d % 1000], T2[d / 1000]) >> 22 for d <= 27725 and 0 beyond.

find-tfbs_amd/csrc/affinity_log_table.hpp: the 1 000 constants of the affinity rows' exact
logarithm (include/tfbs_amd.h, "Affinity rows"),

    P[j] = ceil(2^63 * 2^(j / 1000))           j = 0 .. 999

by an exact integer 1000th root, no decimals: P[j] is the least p with p^1000 >= 2^(63000 + j).
With x normalised to xn = x << (63 - e), e = bitlen(x) - 1, floor(1000 log2 x) is
1000 e + max{j : P[j] <= xn}.

    python tools/gen_affinity_tables.py            rewrites the headers
    python tools/gen_affinity_tables.py --check    exit status 1 when a header differs
"""
import os
import sys
from decimal import Decimal, ROUND_FLOOR, getcontext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "find-tfbs_amd", "csrc", "affinity_tables.hpp")
LOG_HEADER = os.path.join(ROOT, "find-tfbs_amd", "csrc", "affinity_log_table.hpp")
DIGITS = 80
LAST = 27725  # the last d with a(d) > 0: 1000 ln 2^40 = 27725.89


def tables():
    """(T1, T2) as lists of Python ints."""
    getcontext().prec = DIGITS
    one = Decimal(1 << 63)
    t1 = [int((one * (Decimal(-r) / 1000).exp()).to_integral_value(ROUND_FLOOR)) for r in range(1000)]
    t2 = [int((one * Decimal(-q).exp()).to_integral_value(ROUND_FLOOR)) for q in range(28)]
    return t1, t2


def weight(d, t1, t2):
    """a(d) from the tables, as the library computes it."""
    if d > LAST:
        return 0
    return ((t1[d % 1000] * t2[d // 1000]) >> 64) >> 22


def log_table():
    """P as a list of Python ints: P[j] the least p with p^1000 >= 2^(63000 + j), by bisection."""
    out = []
    for j in range(1000):
        target = 1 << (63000 + j)
        lo, hi = (1 << 63) - 1, 1 << 64  # lo^1000 < target <= hi^1000
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if mid ** 1000 >= target:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return out


def array(name, v):
    rows = ["    " + ", ".join("0x%016Xull" % x for x in v[k:k + 4]) + "," for k in range(0, len(v), 4)]
    return "inline constexpr uint64_t %s[%d] = {\n%s\n};\n" % (name, len(v), "\n".join(rows))


def render_log():
    return ("// The table of the affinity rows' exact logarithm mlog2(x) = floor(1000 * log2(x)):\n"
            "// kAffLogP[j] = ceil(2^63 * 2^(j / 1000)), the least p with p^1000 >= 2^(63000 + j), so that\n"
            "// mlog2(x) = 1000 e + max{j : kAffLogP[j] <= x << (63 - e)} with e = bitlen(x) - 1.\n"
            "// Data, written by tools/gen_affinity_tables.py (exact integer 1000th roots): do not edit.\n"
            "#pragma once\n\n#include <cstdint>\n\nnamespace tfbs {\n\n"
            "constexpr uint32_t kAffLogLen = 1000;\n\n" + array("kAffLogP", log_table()) + "\n}  // namespace tfbs\n")


def render():
    t1, t2 = tables()

    return ("// The tables of the binding affinity's weight a(d) = floor(2^40 * exp(-d / 1000)):\n"
            "// kAffT1[r] = floor(2^63 * exp(-r / 1000)), kAffT2[q] = floor(2^63 * exp(-q)), so that\n"
            "// a(d) = umul64hi(kAffT1[d %% 1000], kAffT2[d / 1000]) >> 22 for d <= kAffLast and 0 beyond.\n"
            "// Data, written by tools/gen_affinity_tables.py (decimal at %d digits): do not edit.\n"
            "#pragma once\n\n#include <cstdint>\n\nnamespace tfbs {\n\n"
            "constexpr uint32_t kAffLast = %d;  // the last d with a(d) > 0\n"
            "constexpr uint32_t kAffT1Len = 1000, kAffT2Len = 28;\n\n" % (DIGITS, LAST) +
            array("kAffT1", t1) + "\n" + array("kAffT2", t2) + "\n}  // namespace tfbs\n")


if __name__ == "__main__":
    files = ((HEADER, render()), (LOG_HEADER, render_log()))
    if "--check" in sys.argv[1:]:
        sys.exit(0 if all(os.path.exists(p) and open(p).read() == text for p, text in files) else 1)
    for p, text in files:
        with open(p, "w") as f:
            f.write(text)
