"""Reference and inputs of each sequence's K nearest neighbours (-o n, dpr_nearest_*): np.lexsort on (column, distance) per row after
masking the diagonal and the non-finite entries; the symmetric matrices the CPU and the GPU tests share (computed once per size, never
changed)."""
import functools

import numpy as np

from tests import _pairs_ref as P

PAD_BITS = np.uint64(0x7FF8000000000000)


def nearest(D, K):
    """dict(j [n, K], d [n, K], cnt [n]) as capi.nearest_host returns them, from NumPy"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    j = np.full((n, K), -1, dtype=np.int32)
    d = np.full((n, K), 0, dtype=np.uint64)
    d[:] = PAD_BITS
    d = d.view(np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    for i in range(n):
        row = D[i]
        cols = np.array([c for c in range(n) if c != i and np.isfinite(row[c])], dtype=np.int64)
        vals = row[cols] + 0.0      # (-0.0 + 0.0 is +0.0: the two zeros sort as one value; every other value is unchanged)
        order = cols[np.lexsort((cols, vals))][:K]
        m = len(order)
        j[i, :m] = order
        d[i, :m] = row[order]       # (the entry's own bits)
        cnt[i] = m
    return dict(j=j, d=d, cnt=cnt)


def same(got, ref):
    """the library's answer equals the reference's: j and cnt as integers, d as bits"""
    assert got["j"].shape == ref["j"].shape and got["d"].shape == ref["d"].shape
    assert np.array_equal(got["cnt"], ref["cnt"]), (got["cnt"][:8], ref["cnt"][:8])
    assert np.array_equal(got["j"], ref["j"]), np.argwhere(got["j"] != ref["j"])[:4]
    assert np.array_equal(np.ascontiguousarray(got["d"]).view(np.uint64), np.ascontiguousarray(ref["d"]).view(np.uint64))


def _frozen(D):
    assert np.array_equal(D, D.T, equal_nan=True)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def noisy(n):
    """distinct values: a random permutation of 1 .. n (n - 1) / 2 over the pairs, scaled"""
    rng = np.random.default_rng(11000 + n)
    L = np.zeros((n, n))
    L[np.tril_indices(n, -1)] = (rng.permutation(n * (n - 1) // 2) + 1) * (1.0 / 1024.0)
    D = L + L.T
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def constant(n):
    """every off-diagonal entry equal: row i's neighbours are the K smallest columns other than i"""
    D = np.full((n, n), 0.375)
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def three_values(n):
    """entries drawn from three values: the K-th place falls inside a run of ties"""
    rng = np.random.default_rng(12000 + n)
    D = P.symmetric(rng.choice(np.array([0.125, 0.25, 0.5]), size=(n, n)))
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def descending(n):
    """D[i][j] = (2 n - i - j) / 64: along a row every later column is nearer than all before it"""
    i, j = np.indices((n, n))
    D = (2.0 * n - i - j) / 64.0
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def ascending(n):
    """D[i][j] = (i + j + 1) / 64: nothing behind a row's first K columns is a neighbour"""
    i, j = np.indices((n, n))
    D = (i + j + 1.0) / 64.0
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def nonfinite(n, K=3):
    """the generator of the pairs tests (NaN, +inf, -inf strewn in), plus -- from n = 8 on -- row 1 without a finite entry, row 2 with
    exactly K - 1 and row 3 with exactly K finite entries (K clipped to what a row can hold)"""
    D = P.nonfinite(n).copy()
    if n >= 8:
        bad = (np.nan, np.inf, -np.inf)
        for c in range(n):
            if c != 1:
                D[1, c] = D[c, 1] = bad[c % 3]
        for r, keep in ((2, min(K - 1, n - 4)), (3, min(K, n - 4))):
            kept = 0
            for c in range(n - 1, -1, -1):      # (the finite entries at the far end of the row)
                if c in (1, 2, 3) or c == r:
                    continue
                if kept < keep:
                    D[r, c] = D[c, r] = 0.5 + c / 1024.0
                    kept += 1
                else:
                    D[r, c] = D[c, r] = bad[c % 3]
            D[2, 3] = D[3, 2] = np.nan
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def signed_zero(n):
    """three_values with a few -0.0 beside +0.0 entries (they tie: the column decides; the sign bit stays in d) and a few negative
    entries (they sort below zero)"""
    rng = np.random.default_rng(13000 + n)
    D = three_values(n).copy()
    cells = [(int(a), int(b)) for a, b in zip(rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)) if a != b]
    for k, (a, b) in enumerate(cells):
        D[a, b] = D[b, a] = (-0.0, 0.0, -0.0, 0.0, -0.25, -1.5)[k % 6]
    if n >= 3:
        D[0, 1] = D[1, 0] = 0.0
        D[0, 2] = D[2, 0] = -0.0
        D[n - 1, 0] = D[0, n - 1] = -0.0
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


MATRICES = dict(noisy=noisy, constant=constant, three_values=three_values, descending=descending, ascending=ascending,
                nonfinite=nonfinite, signed_zero=signed_zero)


def matrix(name, n, K=3):
    return nonfinite(n, K) if name == "nonfinite" else MATRICES[name](n)
