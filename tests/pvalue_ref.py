"""The model of "Thresholds from a p-value" (include/tfbs_amd.h): exact score distributions
of a strand under a uniform background in Python integers and dictionaries, by enumeration
(small L) and by a dynamic programme, and the threshold rule with fractions.Fraction.
A strand is (kind, weights): kind "mono" with L columns of 4 weights [A, C, G, T], or "di"
with L - 1 rows of 16 weights indexed 4 a + b."""
import bisect
import itertools
from fractions import Fraction


def length(kind, weights):
    return len(weights) if kind == "mono" else len(weights) + 1


def score(kind, weights, x):
    if kind == "mono":
        return sum(weights[j][x[j]] for j in range(len(weights)))
    return sum(weights[j][4 * x[j] + x[j + 1]] for j in range(len(weights)))


def counts_enum(kind, weights):
    """cnt by scoring every sequence of {A,C,G,T}^L."""
    cnt = {}
    for x in itertools.product(range(4), repeat=length(kind, weights)):
        s = score(kind, weights, x)
        cnt[s] = cnt.get(s, 0) + 1
    return cnt


def counts_dp(kind, weights):
    """cnt by one pass per column (row), scattering: not the gather the product runs."""
    if kind == "mono":
        cur = {0: 1}
        for col in weights:
            nxt = {}
            for s, c in cur.items():
                for b in range(4):
                    nxt[s + col[b]] = nxt.get(s + col[b], 0) + c
            cur = nxt
        return cur
    tabs = [{0: 1} for _ in range(4)]  # per last base
    for row in weights:
        nxt = [{} for _ in range(4)]
        for a in range(4):
            for s, c in tabs[a].items():
                for b in range(4):
                    t = s + row[4 * a + b]
                    nxt[b][t] = nxt[b].get(t, 0) + c
        tabs = nxt
    cnt = {}
    for tab in tabs:
        for s, c in tab.items():
            cnt[s] = cnt.get(s, 0) + c
    return cnt


class Dist:
    """tail(m) = #{x : S(x) >= m} from a cnt dictionary."""

    def __init__(self, cnt, L):
        self.L = L
        self.scores = sorted(cnt)
        self.tails = [0] * len(self.scores)
        run = 0
        for k in range(len(self.scores) - 1, -1, -1):
            run += cnt[self.scores[k]]
            self.tails[k] = run
        assert run == 4 ** L
        self.smin, self.smax = self.scores[0], self.scores[-1]

    def tail(self, m):
        k = bisect.bisect_left(self.scores, m)
        return self.tails[k] if k < len(self.scores) else 0

    def threshold(self, p):
        """max{m : tail(m) > floor(p 4^L)}: p is taken as the exact rational a double holds."""
        x = (Fraction(p) * 4 ** self.L).__floor__()
        for k in range(len(self.scores) - 1, -1, -1):
            if self.tails[k] > x:
                return self.scores[k]
        raise AssertionError("p >= 1")


def reverse_mono(cols):
    return [[c[3], c[2], c[1], c[0]] for c in reversed(cols)]


def reverse_di(rows):
    R = len(rows)
    return [[rows[R - 1 - i][4 * (3 - b) + (3 - a)] for a in range(4) for b in range(4)] for i in range(R)]
