"""Reference and inputs of the pairs within a distance threshold (-o p, dpr_pairs_*): np.nonzero on the strict lower triangle with `<=`
plus a dict union-find; the matrices the CPU and the GPU tests share (computed once per size, never changed)."""
import functools

import numpy as np

from tests import _nonfinite

DBL_MAX = float(np.finfo(np.float64).max)


def within(D, T):
    """dict(i, j, d, label, stats) as capi.pairs_within_host returns them, from NumPy and a dict union-find"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    with np.errstate(invalid="ignore"):
        keep = np.tril(D <= T, -1)      # (NaN <= T is False, +inf <= T is False for every finite T)
    i, j = np.nonzero(keep)             # row-major: by i, then by j
    parent = {v: v for v in range(n)}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(v) for v in range(n)], dtype=np.int32)
    # the label of a component is its smallest member: by construction, and checked independently of the union order
    members = {}
    for v in range(n):
        members.setdefault(int(label[v]), []).append(v)
    assert all(min(m) == r for r, m in members.items())
    sizes = [len(m) for m in members.values()]
    stats = dict(pairs=len(i), components=len(sizes), largest=max(sizes), singletons=sum(s == 1 for s in sizes))
    return dict(i=i.astype(np.int32), j=j.astype(np.int32), d=D[i, j], label=label, stats=stats)


def ranks(label):
    """1-based rank of every tip's component, components ordered by their smallest member"""
    order = {r: k + 1 for k, r in enumerate(sorted(set(int(v) for v in label)))}
    return np.array([order[int(v)] for v in label], dtype=np.int32)


def same(got, ref):
    """the library's answer equals the reference's as bits: i, j, d as uint64, label, the counts"""
    assert np.array_equal(got["i"], ref["i"]) and np.array_equal(got["j"], ref["j"]), (len(got["i"]), len(ref["i"]))
    assert np.array_equal(np.ascontiguousarray(got["d"]).view(np.uint64), np.ascontiguousarray(ref["d"]).view(np.uint64))
    assert np.array_equal(got["label"], ref["label"])
    for k in ("pairs", "components", "largest", "singletons"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])


def symmetric(L):
    L = np.tril(L, -1)
    return L + L.T


@functools.lru_cache(maxsize=None)
def noisy(n, seed=0):
    """distances ~ U(0.05, 1) rounded to two places (many exact ties, so a threshold can equal entries), symmetric, zero diagonal"""
    rng = np.random.default_rng(7000 + 13 * n + seed)
    D = symmetric(np.round(rng.random((n, n)) * 0.95 + 0.05, 2))
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def nonfinite(n, seed=0):
    """noisy with NaN, +inf and -inf entries strewn in, the last row and the first column included"""
    rng = np.random.default_rng(9000 + 17 * n + seed)
    D = noisy(n, seed).copy()
    if n >= 3:
        cells = [(int(a), int(b)) for a, b in zip(rng.integers(1, n, 3 * n), rng.integers(0, n, 3 * n)) if b < a]
        for k, (a, b) in enumerate(cells[: max(3, n // 2)] + [(n - 1, 0), (n - 1, n - 2), (1, 0)]):
            D[a, b] = D[b, a] = (np.nan, np.inf, -np.inf)[k % 3]
    D.setflags(write=False)
    return D


def nonfinite_named(n):
    """the four matrices of tests/_nonfinite.py (n >= 80)"""
    return _nonfinite.matrices(n, 5)


def relabel(D, perm):
    """tip v of D becomes tip perm[v]"""
    n = D.shape[0]
    out = np.empty_like(D)
    out[np.ix_(perm, perm)] = D
    assert out.shape == (n, n)
    return out


@functools.lru_cache(maxsize=None)
def shapes(n):
    """name -> (D, T): graphs whose components are known, built as matrices (edges 0.25, everything else 0.75, T = 0.5).
    path: 0-1-...-(n-1) under a random relabelling (long parent chains); star: everybody joined to one tip; cliques: two cliques
    joined by one pair whose row is the last; singletons: no pair at all"""
    rng = np.random.default_rng(500 + n)
    far, near, T = 0.75, 0.25, 0.5
    out = {}
    P = np.full((n, n), far)
    for v in range(n - 1):
        P[v, v + 1] = P[v + 1, v] = near
    np.fill_diagonal(P, 0.0)
    out["path"] = (relabel(P, rng.permutation(n)), T)
    S = np.full((n, n), far)
    hub = n // 3
    S[hub, :] = S[:, hub] = near
    np.fill_diagonal(S, 0.0)
    out["star"] = (S, T)
    if n >= 5:
        C = np.full((n, n), far)
        h = n // 2
        C[:h, :h] = near                # clique 0 .. h-1
        C[h:, h:] = near                # clique h .. n-1
        C[n - 1, 0] = C[0, n - 1] = near      # the one pair that joins the two, in the last row
        np.fill_diagonal(C, 0.0)
        out["cliques"] = (C, T)
    Z = np.full((n, n), far)
    np.fill_diagonal(Z, 0.0)
    out["singletons"] = (Z, T)
    for D, _ in out.values():
        D.setflags(write=False)
    return out
