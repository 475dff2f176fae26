"""High-precision reference for the six aligned-sequence distance types (test infrastructure).

Written from the formulas of the original program, not from the oracle: types 1-2 from its all-pairs kernel (counts: a site is
useful when either code is a base, a match when the column's code is a base equal to the row's; epilogue 1 - match / useful and
-0.75 log(1 - uncor / 0.75)), types 3-6 from its divide-and-conquer kernels (only sites valid in both sequences count; Tajima-Nei,
K2P, Tamura and Jin-Nei epilogues as written there, the integer pair counts included where they enter as counts).

Counts are plain integers: useful, match and the 4 x 4 table of (row base, column base) over sites valid in both sequences.  The
epilogues run on exact rationals (`fractions`); `log` and `sqrt` use `decimal` at 50 digits.  Every cell falls into one class:

  regular        every denominator and every log / sqrt argument is at least 1e-6 in magnitude: compare at a relative 1e-12;
  special        an exact denominator is 0, or a log argument is 0 or negative: IEEE decides (0/0 and log or sqrt of a negative
                 number -> NaN, x/0 -> +-inf, log 0 -> -inf).  Only when every rational leading to the singular value is exactly a
                 binary64 number, so that the fp64 computation meets the same exact zero;
  near-singular  everything else (skipped by the comparisons, counted).
"""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _c, _v in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"U", 3)):
    _CODE[_c[0]] = _v
DIGITS = 50
TINY = Fraction(1, 10 ** 6)
REGULAR, SPECIAL, NEAR = "regular", "special", "near"


def codes(seq):
    """A, C, G, T/U -> 0..3, anything else (gaps, N, lower case, IUPAC) -> 4"""
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


class Counts:
    """one ordered pair (row a, column b)"""

    def __init__(self, a, b):
        va, vb = a < 4, b < 4
        self.useful = int(np.count_nonzero(va | vb))
        self.match = int(np.count_nonzero(vb & (a == b)))
        both = va & vb
        t = np.zeros((4, 4), dtype=np.int64)
        np.add.at(t, (a[both].astype(np.intp), b[both].astype(np.intp)), 1)
        self.table = t                                              # [row base][column base]
        self.tot = int(t.sum())
        self.match_v = int(np.trace(t))
        self.frac = [int(t[i, :].sum() + t[:, i].sum()) for i in range(4)]
        self.pr = [int(t[0, 2] + t[2, 0]), int(t[0, 3] + t[3, 0]), int(t[1, 2] + t[2, 1]), int(t[1, 3] + t[3, 1])]
        off = ~np.eye(4, dtype=bool)
        same = np.array([[(i % 2) == (j % 2) for j in range(4)] for i in range(4)])
        self.p = int(t[off & same].sum())                           # transitions A<->G, C<->T
        self.q = int(t[off & ~same].sum())                          # transversions
        self.gc1 = int(sum(t[i, j] for i in (1, 2) for j in range(4) if j != i))     # row base C or G at a mismatch
        self.gc2 = int(sum(t[i, j] for j in (1, 2) for i in range(4) if i != j))     # column base C or G at a mismatch


class _NearSingular(Exception):
    pass


class X:
    """a value of the epilogue: an exact rational ('q', with `fp`: it and everything it came from are binary64 numbers), a
    50-digit decimal after a transcendental step ('d'), or an IEEE special ('f': NaN / +-inf, or a zero a special produced)."""

    def __init__(self, kind, v, fp=True):
        self.kind, self.v, self.fp = kind, v, fp

    @staticmethod
    def q(v, fp=True):
        v = Fraction(v)
        return X("q", v, fp and Fraction(float(v)) == v)

    def _f(self):
        if self.kind == "f":
            return self.v
        return np.float64(float(self.v))

    def _d(self):
        return self.v if self.kind == "d" else Decimal(self.v.numerator) / Decimal(self.v.denominator)

    def _bin(self, o, op):
        o = o if isinstance(o, X) else X.q(o)
        if self.kind == "f" or o.kind == "f":
            with np.errstate(all="ignore"):
                r = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide}[op](self._f(), o._f())
            return X("f", np.float64(r))
        if op == "/":
            if o.kind == "q" and o.v == 0:
                if not o.fp:
                    raise _NearSingular()
                if self.kind == "q" and self.v == 0:
                    return X("f", np.float64(np.nan))
                return X("f", np.float64(math.copysign(math.inf, float(self.v))))
            if abs(o.v) < (TINY if o.kind == "q" else Decimal(1) / Decimal(10 ** 6)):
                raise _NearSingular()
        zero = [z for z in (self, o) if z.kind == "q" and z.v == 0]
        if op == "*" and zero:          # an exact zero times a finite value is an exact zero in fp64 too
            return X.q(0, all(z.fp for z in zero))
        if self.kind == "q" and o.kind == "q":
            a, b = self.v, o.v
            r = {"+": a + b, "-": a - b, "*": a * b, "/": a / b if op == "/" else None}[op]
            return X.q(r, self.fp and o.fp)
        with localcontext() as ctx:
            ctx.prec = DIGITS
            a, b = self._d(), o._d()
            return X("d", {"+": a + b, "-": a - b, "*": a * b, "/": a / b if op == "/" else None}[op])

    def __add__(self, o): return self._bin(o, "+")
    def __sub__(self, o): return self._bin(o, "-")
    def __mul__(self, o): return self._bin(o, "*")
    def __truediv__(self, o): return self._bin(o, "/")
    def __radd__(self, o): return X.q(o)._bin(self, "+")
    def __rsub__(self, o): return X.q(o)._bin(self, "-")
    def __rmul__(self, o): return X.q(o)._bin(self, "*")
    def __rtruediv__(self, o): return X.q(o)._bin(self, "/")
    def __neg__(self): return X.q(0)._bin(self, "-") if self.kind != "f" else X("f", -self.v)

    def _sign0(self):
        """-1, 0, +1 of an exact or decimal value; raises for a zero that fp64 may not meet exactly"""
        if self.kind == "q":
            if self.v == 0 and not self.fp:
                raise _NearSingular()
            return (self.v > 0) - (self.v < 0)
        return (self.v > 0) - (self.v < 0)

    def log(self):
        if self.kind == "f":
            with np.errstate(all="ignore"):
                return X("f", np.log(self.v))
        s = self._sign0()
        if s < 0:
            return X("f", np.float64(np.nan))
        if s == 0:
            return X("f", np.float64(-np.inf))
        if self.kind == "q" and self.v == 1:
            return X.q(0, self.fp)
        if self._d() < Decimal(1) / Decimal(10 ** 6):
            raise _NearSingular()
        with localcontext() as ctx:
            ctx.prec = DIGITS
            return X("d", self._d().ln())

    def sqrt(self):
        if self.kind == "f":
            with np.errstate(all="ignore"):
                return X("f", np.sqrt(self.v))
        s = self._sign0()
        if s < 0:
            return X("f", np.float64(np.nan))
        if s == 0:
            return X.q(0, self.fp)
        if self.kind == "q":
            r = math.isqrt(self.v.numerator * self.v.denominator)
            if r * r == self.v.numerator * self.v.denominator:      # an exact square root (1, 1/4, ...)
                return X.q(Fraction(r, self.v.denominator), self.fp)
        if self._d() < Decimal(1) / Decimal(10 ** 6):
            raise _NearSingular()
        with localcontext() as ctx:
            ctx.prec = DIGITS
            return X("d", self._d().sqrt())


def _epilogue(c, t):
    if t in (1, 2):
        uncor = 1 - X.q(c.match) / c.useful
        if t == 1:
            return uncor
        return X.q(Fraction(-3, 4)) * (1 - uncor / Fraction(3, 4)).log()
    tot = X.q(c.tot)
    if t == 3:
        fr = [X.q(f) / tot / 2 for f in c.frac]
        h = (Fraction(1, 2) * X.q(c.pr[0]) * fr[0] * fr[2] + Fraction(1, 2) * X.q(c.pr[1]) * fr[0] * fr[3]
             + Fraction(1, 2) * X.q(c.pr[2]) * fr[1] * fr[2] + Fraction(1, 2) * X.q(c.pr[3]) * fr[1] * fr[3])
        D = X.q(c.tot - c.match_v) / tot
        b = Fraction(1, 2) * (1 - fr[0] * fr[0] - fr[2] * fr[2] + D * D / h)
        return -b * (1 - D / b).log()
    pp, qq = X.q(c.p) / tot, X.q(c.q) / tot
    if t == 4:
        return Fraction(-1, 2) * ((1 - 2 * pp - qq) * (1 - 2 * qq).sqrt()).log()
    if t == 6:
        return Fraction(1, 2) * (1 / (1 - 2 * pp - qq) + Fraction(1, 2) / (1 - qq * 2) - Fraction(3, 2))
    if t == 5:
        g1, g2 = X.q(c.gc1), X.q(c.gc2)
        cc = g1 / tot + g2 / tot - 2 * g1 * g2 / tot / tot
        return -cc * (1 - pp / cc - qq).log() - Fraction(1, 2) * (1 - cc) * (1 - 2 * qq).log()
    raise ValueError(t)


def distance(c, t):
    """(class, value): value a float (regular: the correctly rounded exact value; special: NaN / +-inf); None when near-singular"""
    try:
        r = _epilogue(c, t)
    except _NearSingular:
        return NEAR, None
    if r.kind == "f":
        v = float(r.v)
        if math.isfinite(v):           # a finite result out of a special intermediate (x / inf): not IEEE-stable in general
            return NEAR, None
        return SPECIAL, v
    return REGULAR, float(r.v) if r.kind == "q" else float(r.v)


def dist_lower(seqs, t):
    """classes and values of the strict lower triangle (row r > column c), as the oracle and the kernels orient the pair"""
    cs = [codes(s) for s in seqs]
    n = len(cs)
    cls = np.full((n, n), "", dtype=object)
    val = np.full((n, n), np.nan)
    for r in range(1, n):
        for c in range(r):
            k, v = distance(Counts(cs[r], cs[c]), t)
            cls[r, c] = k
            if v is not None:
                val[r, c] = v
    return cls, val
