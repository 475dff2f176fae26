"""References and inputs of the minimum spanning forest of the distances (-o s, dpr_mst_*): a NumPy Kruskal (np.lexsort on (j, i, key)
and a dict union-find) and a NumPy Boruvka that follows the device's round structure (row minimum, component minimum, emit, join) and
also returns the number of rounds; the minimax path distances by a direct closure; the symmetric matrices the CPU and the GPU tests
share (computed once per size, never changed)."""
import functools

import numpy as np

from tests import _nearest_ref as N

ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN = np.uint64(0x8000000000000000)


def key(D):
    """the contract's key of every entry: the bits of D (of +0.0 for either zero), the sign bit flipped for D >= 0 and all bits flipped
    for D < 0; all ones where D is not finite"""
    D = np.ascontiguousarray(np.asarray(D, dtype=np.float64))
    b = (D + 0.0).view(np.uint64)      # (-0.0 + 0.0 is +0.0; every other value is unchanged)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | SIGN)
    return np.where(np.isfinite(D), k, ALL_ONES)


class _Forest:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, v):
        while self.parent[v] != v:
            self.parent[v] = self.parent[self.parent[v]]
            v = self.parent[v]
        return v

    def join(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra == rb:
            return False
        self.parent[max(ra, rb)] = min(ra, rb)      # (the root of a component is its smallest member)
        return True

    def labels(self):
        return np.array([self.find(v) for v in range(len(self.parent))], dtype=np.int32)


def _result(D, edges, label):
    e = np.array(edges, dtype=np.int64).reshape(-1, 2)
    return dict(i=e[:, 0].astype(np.int32), j=e[:, 1].astype(np.int32), d=np.asarray(D)[e[:, 0], e[:, 1]], label=label)


def kruskal(D):
    """dict(i, j, d, label) as capi.mst_host returns them: every finite entry below the diagonal in the order (key, i, j), taken when its
    ends are not joined yet"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    i, j = np.tril_indices(n, -1)
    k = key(D[i, j])
    keep = k != ALL_ONES
    i, j, k = i[keep], j[keep], k[keep]
    order = np.lexsort((j, i, k))
    f, edges = _Forest(n), []
    for a, b in zip(i[order].tolist(), j[order].tolist()):
        if f.join(a, b):
            edges.append((a, b))
            if len(edges) == n - 1:
                break
    return _result(D, edges, f.labels())


def boruvka(D):
    """(dict as kruskal gives it, rounds): per round every row's smallest (key, column) over the finite entries whose column lies in
    another component, per component the smallest (key, max(r, c), min(r, c)) of its rows, every component's edge once, the join; the
    rounds end when nothing was emitted or one component is left.  The edges sorted once at the end"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    K = key(D)
    np.fill_diagonal(K, ALL_ONES)
    f, label, edges, rounds = _Forest(n), np.arange(n), set(), 0
    rows = np.arange(n)
    while True:
        rounds += 1
        Km = np.where(label[None, :] != label[:, None], K, ALL_ONES)
        rcol = np.argmin(Km, axis=1)          # (the first of equal keys: the smaller column)
        rkey = Km[rows, rcol]
        best = {}
        for r in np.nonzero(rkey != ALL_ONES)[0].tolist():
            c = int(rcol[r])
            cand = (int(rkey[r]), max(r, c), min(r, c))
            if cand < best.get(int(label[r]), (1 << 64, 0, 0)):
                best[int(label[r])] = cand
        emitted = {(i, j) for _, i, j in best.values()} - edges
        for i, j in sorted(emitted):
            assert f.join(i, j)                # (the edges of a round close no cycle)
        edges |= emitted
        label = f.labels().astype(np.int64)
        if not emitted or len(set(label.tolist())) == 1:
            break
    ordered = sorted(edges, key=lambda e: (int(K[e[0], e[1]]), e[0], e[1]))
    return _result(D, ordered, label.astype(np.int32)), rounds


def same(got, ref):
    """the library's answer equals the reference's as bits: i, j, label as integers, d as uint64"""
    assert np.array_equal(got["i"], ref["i"]) and np.array_equal(got["j"], ref["j"]), (len(got["i"]), len(ref["i"]))
    assert np.array_equal(np.ascontiguousarray(got["d"]).view(np.uint64), np.ascontiguousarray(ref["d"]).view(np.uint64))
    assert np.array_equal(got["label"], ref["label"])


def summary(label):
    """dict(components, largest, singletons) of labels"""
    _, sizes = np.unique(np.asarray(label), return_counts=True)
    return dict(components=len(sizes), largest=int(sizes.max()), singletons=int((sizes == 1).sum()))


def minimax(D):
    """the minimax path distance of every pair -- the smallest, over the paths between the two, of the path's largest finite entry -- by
    the direct closure M = min(M, max(M[:, k], M[k, :])) over every k; +inf where no path of finite entries joins the pair"""
    M = np.where(np.isfinite(D), np.asarray(D, dtype=np.float64), np.inf)
    np.fill_diagonal(M, -np.inf)
    for k in range(M.shape[0]):
        M = np.minimum(M, np.maximum(M[:, k : k + 1], M[k : k + 1, :]))
    return M


def tree_paths(n, parent, length):
    """the path length of every pair of tips in the tree (parent, length) of 2 n - 1 nodes, a parent behind its children"""
    m = len(parent)
    depth = np.zeros(m)
    for v in range(m - 2, -1, -1):
        assert parent[v] > v
        depth[v] = depth[parent[v]] + length[v]
    tips = {v: [v] for v in range(n)}
    P = np.zeros((n, n))
    kids = {}
    for v in range(m - 1):
        kids.setdefault(int(parent[v]), []).append(v)
    for u in range(n, m):
        a, b = kids[u]
        A, B = np.array(tips.pop(a)), np.array(tips.pop(b))
        P[np.ix_(A, B)] = (depth[A] - depth[u])[:, None] + (depth[B] - depth[u])[None, :]
        P[np.ix_(B, A)] = P[np.ix_(A, B)].T
        tips[u] = A.tolist() + B.tolist()
    return P, depth[:n]


def _frozen(D):
    assert np.array_equal(D, D.T, equal_nan=True)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def chain(n):
    """D = |i - j|: every tip's nearest other component is its neighbour; the forest is (i, i - 1), found in one round, and the join
    walks a chain of hooks n deep"""
    i, j = np.indices((n, n))
    return _frozen(np.abs(i - j).astype(np.float64))


@functools.lru_cache(maxsize=None)
def hierarchy(n):
    """D = the bit length of i xor j: a balanced hierarchy, level by level -- a round joins the pairs (2 t, 2 t + 1), the next the
    quadruples: floor(log2 n) rounds, and the columns of a row's own component lie everywhere in the row"""
    i, j = np.indices((n, n))
    x = (i ^ j).astype(np.float64)
    D = np.where(x > 0, np.floor(np.log2(np.maximum(x, 1.0))) + 1.0, 0.0)
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def nonfinite(n):
    """distinct finite values with NaN, +inf and -inf strewn in at random; the tips below n // 2 and the others are two groups with
    nothing finite between them; tip 1 has nothing finite against anyone: several components, a singleton, a last round that emits
    nothing"""
    rng = np.random.default_rng(21000 + n)
    D = N.noisy(n).copy()
    bad = np.array([np.nan, np.inf, -np.inf])
    hit = np.tril(rng.random((n, n)) < 0.2, -1)
    fill = bad[rng.integers(0, 3, size=(n, n))]
    D[hit] = fill[hit]
    D[hit.T] = fill.T[hit.T]
    h = n // 2
    D[h:, :h] = np.nan
    D[:h, h:] = np.nan
    D[1, :] = D[:, 1] = np.inf
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def negative(n):
    """the distinct values of noisy shifted so that half of them are negative: ordinary values, ordered below zero"""
    D = N.noisy(n) - (n * (n - 1) // 4) / 1024.0
    np.fill_diagonal(D, 0.0)
    return _frozen(D)


MATRICES = dict(noisy=N.noisy, three_values=N.three_values, constant=N.constant, chain=chain, hierarchy=hierarchy, nonfinite=nonfinite,
                signed_zero=N.signed_zero, negative=negative)
EXACT = ("noisy", "three_values", "constant", "chain", "hierarchy", "negative")      # every entry k / 1024: sums of branches are exact


def matrix(name, n):
    return MATRICES[name](n)


def closed_form(name, n):
    """the forest of `constant` (the star (i, 0)) and of `chain` ((i, i - 1)), i = 1 .. n - 1, as (i, j) arrays"""
    i = np.arange(1, n, dtype=np.int32)
    return (i, np.zeros(n - 1, dtype=np.int32)) if name == "constant" else (i, i - 1)
