"""NumPy reference of UPGMA / WPGMA, independent of the library (tests/test_upgma.py holds dpr_upgma_host to it).

UPGMA is computed FROM THE DEFINITION: the distance of two clusters is the mean of the ORIGINAL distances over their member pairs
-- there is no recurrence, so an error in the library's weighted update cannot hide in a reference that repeats it.  WPGMA has no
such closed form (its weights depend on the merge order) and is computed by its recurrence.  The pair of every step is chosen by
the contract's order of values on the definition's numbers, and the slots move as the contract moves them, so that logs can be
compared entry by entry.  Per step the reference also returns the relative gap between its best and its second-best candidate: a
comparison of logs means something only where no step is a near-tie that rounding could decide either way."""
import struct

import numpy as np

ALL = (1 << 64) - 1


def key(v):
    """the contract's order of values: negative < zero (-0.0 as +0.0) < positive finite < +inf < NaN, as an integer"""
    v = float(v)
    if v != v:
        return ALL
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    if b == 1 << 63:
        b = 0
    return (~b) & ALL if b >> 63 else b | (1 << 63)


def symmetric(lower):
    """(n, n) symmetric matrix with a zero diagonal from the strict lower triangle of `lower`"""
    L = np.tril(np.asarray(lower, dtype=np.float64), -1)
    return L + L.T


def noisy_matrix(rng, n):
    return symmetric(rng.random((n, n)) + 0.05)


def run(D, linkage):
    """dict(merge_x, merge_y, height, gap (n-1 relative gaps, inf where a step has one candidate), members (tips of node n+it))"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    members = [[i] for i in range(n)]            # by slot
    W = D.copy()                                 # WPGMA: the recurrence's matrix, by slot
    mx, my, hs, gaps, made = [], [], [], [], []
    for it in range(n - 1):
        m = n - it
        cand = []
        for i in range(m):
            for j in range(i + 1, m):
                v = float(np.mean(D[np.ix_(members[i], members[j])])) if linkage == 0 else float(W[j, i])
                cand.append((key(v), i, j, v))
        cand.sort(key=lambda c: c[:3])
        _, x, y, d = cand[0]
        if len(cand) > 1:
            d2 = cand[1][3]
            gaps.append(abs(d2 - d) / max(abs(d), 1e-300) if np.isfinite(d) and np.isfinite(d2) else np.inf)
        else:
            gaps.append(np.inf)
        mx.append(x); my.append(y); hs.append(0.5 * d)
        for k in range(m):
            if k != x and k != y:
                W[x, k] = W[k, x] = 0.5 * (W[x, k] + W[y, k])
        members[x] = members[x] + members[y]
        made.append(sorted(members[x]))
        last = m - 1
        if y != last:
            members[y] = members[last]
            W[y, :] = W[last, :]
            W[:, y] = W[:, last]
    return dict(merge_x=np.array(mx, dtype=np.int32), merge_y=np.array(my, dtype=np.int32), height=np.array(hs), gap=np.array(gaps), members=made)


def clades_of_log(n, mx, my):
    """tips under node n+it of a log, by the slot bookkeeping of the contract"""
    members = [[i] for i in range(n)]
    out = []
    for it in range(len(mx)):
        x, y, last = int(mx[it]), int(my[it]), n - it - 1
        members[x] = members[x] + members[y]
        out.append(sorted(members[x]))
        members[y] = members[last]
    return out


def children_of_log(n, mx, my):
    """(node of slot x, node of slot y) joined by every merge: tips < n, node n+it made by merge it"""
    real = list(range(n))
    out = []
    for it in range(len(mx)):
        x, y, last = int(mx[it]), int(my[it]), n - it - 1
        out.append((real[x], real[y]))
        real[x] = n + it
        real[y] = real[last]
    return out


def contract_loop(D, linkage):
    """the contract, literally, in Python floats (IEEE doubles, the same order of operations): what the library must give bit for bit"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    M = [[float(D[i, j]) for j in range(n)] for i in range(n)]
    s = [1.0] * n
    mx, my, hs = [], [], []
    for it in range(n - 1):
        m = n - it
        best = None
        for i in range(m):
            for j in range(i + 1, m):
                c = (key(M[j][i]), i, j)
                if best is None or c < best:
                    best = c
        _, x, y = best
        d = M[y][x]
        mx.append(x); my.append(y); hs.append(0.5 * d)
        for k in range(m):
            if k == x or k == y:
                continue
            a, b = M[x][k], M[y][k]
            val = (s[x] * a + s[y] * b) / (s[x] + s[y]) if linkage == 0 else 0.5 * (a + b)
            M[x][k] = M[k][x] = val
        s[x] = s[x] + s[y]
        last = m - 1
        if y != last:
            for k in range(m):
                M[y][k] = M[last][k]
            for k in range(m):
                M[k][y] = M[k][last]
            s[y] = s[last]
    return dict(merge_x=np.array(mx, dtype=np.int32), merge_y=np.array(my, dtype=np.int32), height=np.array(hs, dtype=np.float64))


def ultrametric_tree(rng, n, whole=True):
    """a random rooted binary tree over n tips whose internal nodes have distinct heights (whole numbers 1, 2, .. in a random
    order of joining, or those times a random factor): (D with D[a][b] = 2 height(lca), {frozenset(clade): height})"""
    clusters = [[i] for i in range(n)]
    D = np.zeros((n, n))
    clades = {}
    scale = 1.0 if whole else float(rng.random() + 0.5)
    for step in range(n - 1):
        a, b = sorted(rng.choice(len(clusters), 2, replace=False))
        h = (step + 1) * scale
        for u in clusters[a]:
            for v in clusters[b]:
                D[u, v] = D[v, u] = 2.0 * h
        merged = clusters[a] + clusters[b]
        clades[frozenset(merged)] = h
        clusters[a] = merged
        clusters.pop(b)
    return D, clades


def newick(names, mx, my, height, labels=None, fmt=lambda v: "%g" % v):
    """the rooted text `dipper --upgma` writes for a log: node n+it joins the nodes of slots x and y, each on a branch of its own
    height minus the child's; labels[k] (an int, or None) goes after the `)` of node n+k, the root carries none"""
    n = len(names)
    real, h = list(range(n)), [0.0] * n
    kids = {}
    for it in range(n - 1):
        x, y, last = int(mx[it]), int(my[it]), n - it - 1
        hn = float(height[it])
        kids[n + it] = [(real[x], hn - h[x]), (real[y], hn - h[y])]
        real[x], h[x] = n + it, hn
        real[y], h[y] = real[last], h[last]
    root = 2 * n - 2

    def text(v):
        if v < n:
            return names[v]
        lab = "" if labels is None or v == root or labels[v - n] is None else str(labels[v - n])
        return "(" + ",".join(text(c) + ":" + fmt(l) for c, l in kids[v]) + ")" + lab

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 100))
    return text(root) + ";\n"
