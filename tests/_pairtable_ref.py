"""High-precision reference for the pair-table distance types 9 (TN93), 10 (LogDet) and 11 (paralinear) -- test infrastructure.

Written from the definitions in include/dipper_hip.h.  For the ordered pair (row a, column b) the 4 x 4 table F[row base][column
base] over the sites valid in both sequences comes from tests/_msa_ref.Counts; the determinant is exact (Python ints); the
epilogues run on exact rationals (`fractions`) with `ln` and `sqrt` in `decimal` at 50 digits.  Every cell falls into one class:

  regular   the value is the correctly rounded exact one; compare with `close` (|gpu - ref| <= 1e-11 |ref| + 1e-14: the project's
            relative bound for distances through log, DESIGN.md section 3, plus an absolute part for ln of an argument near 1 --
            15 times the worst absolute error, 6e-16, of a plain binary64 evaluation of these formulas; -0.0 equals 0.0);
  special   types 10 and 11: NaN or +inf, exactly as the sign of the integer determinant and of the products decides (value = that
            NaN / +inf).  Type 9: NaN when N = 0 or a frequency product a_A a_G, a_C a_T is 0 (value NaN); not finite when a log
            argument is <= 0 (value None: NaN or an infinity, the cell must not be finite);
  near      type 9 only: a log argument with 0 < |arg| < 1e-5.  Skipped by the comparisons, counted (at most 0.1 % of a case).
"""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

from tests import _msa_ref

TYPES = (9, 10, 11)
REGULAR, SPECIAL, NEAR = "regular", "special", "near"
DIGITS = 50
RTOL, ATOL = 1e-11, 1e-14
NEAR_ARG = Fraction(1, 10 ** 5)
A, C, G, T = 0, 1, 2, 3


def det4(F):
    """exact determinant of a 4 x 4 table of Python ints (cofactor expansion along the first row)"""
    def det3(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    return sum((-1) ** j * F[0][j] * det3([[F[i][k] for k in range(4) if k != j] for i in (1, 2, 3)]) for j in range(4))


def _dec(q):
    return Decimal(q.numerator) / Decimal(q.denominator)


def _ln(q):
    return _dec(q).ln()


def table(a_codes, b_codes):
    """F as nested Python ints, from the Counts of tests/_msa_ref.py"""
    return [[int(v) for v in row] for row in _msa_ref.Counts(a_codes, b_codes).table]


def margins(F):
    r = [sum(F[i]) for i in range(4)]
    c = [sum(F[i][j] for i in range(4)) for j in range(4)]
    return sum(r), r, c


def tn93_args(F):
    """the three log arguments and k1, k2, k3 as exact rationals (None when N = 0 or a frequency product is 0)"""
    N, r, c = margins(F)
    a = [r[i] + c[i] for i in range(4)]
    if N == 0 or a[A] * a[G] == 0 or a[C] * a[T] == 0:
        return None
    g = [Fraction(a[i], 2 * N) for i in range(4)]
    gR, gY = g[A] + g[G], g[C] + g[T]
    P1 = Fraction(F[A][G] + F[G][A], N)
    P2 = Fraction(F[C][T] + F[T][C], N)
    Q = Fraction(N - sum(F[i][i] for i in range(4)), N) - P1 - P2
    k1 = 2 * g[A] * g[G] / gR
    k2 = 2 * g[C] * g[T] / gY
    k3 = 2 * (gR * gY - g[A] * g[G] * gY / gR - g[C] * g[T] * gR / gY)
    return (1 - P1 / k1 - Q / (2 * gR), 1 - P2 / k2 - Q / (2 * gY), 1 - Q / (2 * gR * gY)), (k1, k2, k3)


def distance(F, t):
    """(class, value) of one table; value: a float, or None (near; type 9 with a log argument <= 0: any non-finite value)"""
    N, r, c = margins(F)
    with localcontext() as ctx:
        ctx.prec = DIGITS
        if t == 9:
            ak = tn93_args(F)
            if ak is None:
                return SPECIAL, math.nan
            args, ks = ak
            if any(x <= 0 for x in args):
                return SPECIAL, None
            if any(abs(x) < NEAR_ARG for x in args):
                return NEAR, None
            return REGULAR, float(-sum(_dec(k) * _ln(x) for k, x in zip(ks, args)))
        d = det4(F)
        if t == 10:
            if N == 0 or d < 0:
                return SPECIAL, math.nan
            if d == 0:
                return SPECIAL, math.inf
            return REGULAR, float(-_ln(Fraction(d, N ** 4)) / 4 - Decimal(4).ln())
        if t == 11:
            prod = 1
            for i in range(4):
                prod *= r[i] * c[i]
            if d < 0 or (d == 0 and prod == 0):
                return SPECIAL, math.nan
            if d == 0:
                return SPECIAL, math.inf
            return REGULAR, float(-(Decimal(d).ln() - Decimal(prod).ln() / 2) / 4)
    raise ValueError(t)


def reference(seqs):
    """{"F": {(r, c): table}, t: (classes, values)} over the strict lower triangle (row r > column c) of an alignment; cells
    whose value is None hold NaN in `values` and are told apart by their class and by `anyinf` (type 9, argument <= 0)"""
    cs = [_msa_ref.codes(s) for s in seqs]
    n = len(cs)
    out = {"F": {}, "n": n}
    for t in TYPES:
        out[t] = (np.full((n, n), "", dtype=object), np.full((n, n), np.nan), np.zeros((n, n), dtype=bool))
    memo = {}
    for r in range(1, n):
        for c in range(r):
            F = table(cs[r], cs[c])
            out["F"][(r, c)] = F
            key = tuple(map(tuple, F))
            if key not in memo:
                memo[key] = [distance(F, t) for t in TYPES]
            for t, (k, v) in zip(TYPES, memo[key]):
                cls, val, loose = out[t]
                cls[r, c] = k
                if v is None:
                    loose[r, c] = k == SPECIAL
                else:
                    val[r, c] = v
    for t in TYPES:
        for arr in out[t]:
            arr.setflags(write=False)
    return out


def close(got, want):
    """the rule for regular cells, element-wise"""
    return np.abs(got - want) <= RTOL * np.abs(want) + ATOL


def check_matrix(got, ref, t, what=""):
    """the lower triangle of `got` against reference(seqs)[t]; returns (largest excess-free error figures) for printing"""
    cls, val, loose = ref[t]
    n = cls.shape[0]
    lo = np.tril_indices(n, -1)
    g, k, v, any_nonfinite = got[lo], cls[lo], val[lo], loose[lo]
    reg = k == REGULAR
    spec = (k == SPECIAL) & ~any_nonfinite
    near = k == NEAR
    assert near.sum() <= 0.001 * max(g.size, 1), (what, t, int(near.sum()), "near-singular cells")
    assert np.all(~np.isfinite(g[any_nonfinite])), (what, t, "finite where a log argument is <= 0")
    nan = spec & np.isnan(v)
    assert np.all(np.isnan(g[nan])), (what, t, "NaN expected", g[nan][~np.isnan(g[nan])][:4])
    inf = spec & np.isposinf(v)
    assert np.all(np.isposinf(g[inf])), (what, t, "+inf expected", g[inf][~np.isposinf(g[inf])][:4])
    assert np.all(np.isfinite(g[reg])), (what, t, "not finite where the reference is", np.flatnonzero(~np.isfinite(g[reg]))[:4])
    err = np.abs(g[reg] - v[reg])
    worst_abs = float(err.max()) if err.size else 0.0
    worst_rel = float(np.max(err / np.maximum(np.abs(v[reg]), 1e-300))) if err.size else 0.0
    ok = close(g[reg], v[reg])
    print(f"{what} type {t}: {int(reg.sum())} regular, {int((k == SPECIAL).sum())} special, {int(near.sum())} near; "
          f"largest absolute difference {worst_abs:.3e}, relative {worst_rel:.3e}")
    assert np.all(ok), (what, t, g[reg][~ok][:4], v[reg][~ok][:4])
    return worst_abs, worst_rel


_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def msa_drift(L=2080, n=40, seed=0):
    """two groups of n / 2 sequences evolved from one root: in the first group substitutions draw the new base towards G and C,
    in the second towards A and T, so the composition drifts apart and the table of a cross-group pair is not symmetric"""
    rng = np.random.default_rng(6000 + L + n + seed)
    root = rng.integers(0, 4, size=L).astype(np.uint8)
    towards = (np.array([0.08, 0.42, 0.42, 0.08]), np.array([0.42, 0.08, 0.08, 0.42]))
    out = []
    for i in range(n):
        grp = 0 if i < n // 2 else 1
        s = root.copy()
        rate = 0.1 + 0.4 * ((i % (n // 2)) / max(n // 2 - 1, 1))
        hit = np.flatnonzero(rng.random(L) < rate)
        s[hit] = rng.choice(4, size=hit.size, p=towards[grp]).astype(np.uint8)
        out.append(_BASES[s].tobytes())
    return out
