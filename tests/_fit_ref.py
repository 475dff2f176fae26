"""NumPy / Python reference of the tree fit, independent of the library (tests/test_fit_tree.py holds dpr_tree_fit_host to it).

A tree is (parent, length): m entries each, tips 0 .. n-1, parent -1 for the root.  The children are derived from `parent`.  The
path length of two tips is computed twice: by the contract's depth formula, P = (depth[i] - depth[a]) + (depth[j] - depth[a]) with
depth[v] = depth[parent[v]] + length[v] -- the same IEEE operations in the same order, so equal bit for bit to the library's -- and by
ADDING THE EDGES of the path from each tip up to a, one at a time.  The sums are accumulated with math.fsum (exactly rounded)."""
import math

import numpy as np


class Tree:
    def __init__(self, n, parent, length):
        self.n = n
        self.parent = np.asarray(parent, dtype=np.int64)
        self.length = np.asarray(length, dtype=np.float64)
        self.m = m = len(self.parent)
        self.kids = [[] for _ in range(m)]
        roots = [v for v in range(m) if self.parent[v] < 0]
        assert len(roots) == 1
        self.root = roots[0]
        for v in range(m):
            if v != self.root:
                self.kids[int(self.parent[v])].append(v)
        assert all(not self.kids[v] for v in range(n)) and all(len(self.kids[v]) >= 2 for v in range(n, m))
        # pre-order from the root: depth and level of every node
        self.depth = np.zeros(m)
        self.level = np.zeros(m, dtype=np.int64)
        order, stack = [], [self.root]
        while stack:
            v = stack.pop()
            order.append(v)
            for c in self.kids[v]:
                self.depth[c] = self.depth[v] + self.length[c]
                self.level[c] = self.level[v] + 1
                stack.append(c)
        assert len(order) == m
        self.height = int(self.level.max())
        # lca of every pair of tips: two tips in different child clades of a meet in a
        tips = [None] * m
        self.lca = np.full((n, n), -1, dtype=np.int64)
        for v in reversed(order):
            if v < n:
                tips[v] = np.array([v])
                self.lca[v, v] = v
                continue
            parts = [tips[c] for c in self.kids[v]]
            for a in range(len(parts)):
                for b in range(len(parts)):
                    if a != b:
                        self.lca[np.ix_(parts[a], parts[b])] = v
            tips[v] = np.concatenate(parts)
            for c in self.kids[v]:
                tips[c] = None
        assert (self.lca >= 0).all()

    def patristic_depth(self):
        """(n, n) by the contract's formula, the diagonal with a = i"""
        d = self.depth[: self.n]
        da = self.depth[self.lca]
        with np.errstate(invalid="ignore"):
            return (d[:, None] - da) + (d[None, :] - da)

    def patristic_paths(self):
        """((n, n) by adding the edges of each path, (n,) sum of |length| from every tip to the root)"""
        n, m = self.n, self.m
        up = np.zeros((n, m))          # up[i][a]: the edges from tip i to its ancestor a, added one at a time from the tip
        absroot = np.zeros(n)
        for i in range(n):
            v, acc, ab = i, 0.0, 0.0
            while v != self.root:
                acc = acc + float(self.length[v])
                ab = ab + abs(float(self.length[v]))
                v = int(self.parent[v])
                up[i, v] = acc
            absroot[i] = ab
        rows = np.arange(n)
        with np.errstate(invalid="ignore"):
            P = up[rows[:, None], self.lca] + up[rows[None, :], self.lca]
        P[rows, rows] = 0.0
        return P, absroot


def fit(D, tree):
    """dict of the fit from the depth-formula P with math.fsum: n, skipped, the seven sums and the sums of their terms' magnitudes
    (`abs_...`, for the summation bound), n_w, max_e, worst, taxon_ss, taxon_pairs"""
    n = tree.n
    D = np.asarray(D, dtype=np.float64)
    P = tree.patristic_depth()
    ii, jj = np.tril_indices(n, -1)
    d, p = D[ii, jj], P[ii, jj]
    ok = np.isfinite(d) & np.isfinite(p)
    ii, jj, d, p = ii[ok], jj[ok], d[ok], p[ok]
    e = d - p
    ee = e * e
    w = d > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = dict(sum_d=d, sum_p=p, sum_dd=d * d, sum_pp=p * p, sum_dp=d * p, ss=ee, wss=ee[w] / (d[w] * d[w]))
    out = dict(n=int(ok.sum()), skipped=int((~ok).sum()), n_w=int(w.sum()))
    for k, v in terms.items():
        out[k] = math.fsum(v.tolist())
        out["abs_" + k] = math.fsum(np.abs(v).tolist())
        out["terms_" + k] = len(v)
    if len(e):
        ae = np.abs(e)
        best = int(np.lexsort((jj, ii, -ae))[0])       # largest |e|, then the smaller i, then the smaller j
        out["max_e"], out["worst"] = float(ae[best]), (int(ii[best]), int(jj[best]))
    else:
        out["max_e"], out["worst"] = 0.0, (-1, -1)
    out["taxon_ss"] = np.array([math.fsum(ee[(ii == t) | (jj == t)].tolist()) for t in range(n)])
    out["taxon_terms"] = np.array([int(((ii == t) | (jj == t)).sum()) for t in range(n)])
    out["taxon_pairs"] = out["taxon_terms"]
    return out


def derived(s):
    """rms, relative rms, explained variance, cophenetic correlation from a dict of sums (Python floats)"""
    nan = float("nan")
    N, Nw = s["n"], s["n_w"]
    rms = math.sqrt(s["ss"] / N) if N else nan
    rel = math.sqrt(s["wss"] / Nw) if Nw else nan
    vd = s["sum_dd"] - s["sum_d"] * s["sum_d"] / N if N else 0.0
    ev = 1.0 - s["ss"] / vd if vd != 0 else nan
    cd, cp = N * s["sum_dd"] - s["sum_d"] ** 2, N * s["sum_pp"] - s["sum_p"] ** 2
    den = math.sqrt(cd * cp) if cd * cp > 0 else 0.0
    cc = (N * s["sum_dp"] - s["sum_d"] * s["sum_p"]) / den if den else nan
    return rms, rel, ev, cc


# ---- trees ------------------------------------------------------------------------------------------------------------------------
def caterpillar(n, rng):
    """tips 0 and 1 under node n, then one tip more per node: n - 1 edges between the root and tip 0"""
    parent = np.full(2 * n - 1, -1, dtype=np.int32)
    parent[0] = parent[1] = n
    for k in range(1, n - 1):
        parent[n + k - 1] = n + k
        parent[k + 1] = n + k
    return parent, lengths(rng, 2 * n - 1)


def balanced(n, rng):
    """nodes joined two by two, level by level"""
    parent = np.full(2 * n - 1, -1, dtype=np.int32)
    live, nxt = list(range(n)), n
    while len(live) > 1:
        up = []
        for a in range(0, len(live) - 1, 2):
            parent[live[a]] = parent[live[a + 1]] = nxt
            up.append(nxt)
            nxt += 1
        if len(live) % 2:
            up.append(live[-1])
        live = up
    assert nxt == 2 * n - 1
    return parent, lengths(rng, 2 * n - 1)


def multifurcating(n, rng):
    """a root with three or more children, one of them a node with up to four tips, the rest of the tips in cherries or alone"""
    assert n >= 3
    groups, at = [], 0
    sizes = [4, 1, 2, 3]
    while at < n:
        g = min(sizes[len(groups) % 4], n - at)
        groups.append(list(range(at, at + g)))
        at += g
    if len(groups) == 1:                    # n = 3 or 4: the star
        return np.array([n] * n + [-1], dtype=np.int32), lengths(rng, n + 1)
    inner = [g for g in groups if len(g) > 1]
    m = n + len(inner) + 1
    root = m - 1
    parent = np.full(m, root, dtype=np.int32)
    for k, g in enumerate(inner):
        parent[g] = n + k
    parent[root] = -1
    return parent, lengths(rng, m)


def lengths(rng, m, kind="positive"):
    v = 0.01 + rng.random(m)
    if kind == "zero_negative":
        v[rng.random(m) < 0.2] = 0.0
        v[rng.random(m) < 0.2] *= -0.1
    return v


def noisy_matrix(rng, n):
    D = 0.05 + rng.random((n, n))
    D = np.tril(D, -1)
    return D + D.T


# ---- Newick text of the command: patristic distances between named tips -----------------------------------------------------------
def newick_patristic(text):
    """(names in order of appearance, (n, n) path lengths by adding the printed lengths, (n, n) edges on each path)"""
    text = text.strip()
    assert text.endswith(";")
    names, stack = [], []
    nodes = []      # [parent, length above, name or None]
    i, last = 0, None
    while i < len(text):
        ch = text[i]
        if ch == "(":
            nodes.append([stack[-1] if stack else -1, 0.0, None])
            stack.append(len(nodes) - 1)
            i += 1
        elif ch == ")":
            last = stack.pop()
            i += 1
            while i < len(text) and text[i] not in ":,);":      # an internal label
                i += 1
        elif ch == ",":
            i += 1
        elif ch == ":":
            j = i + 1
            while text[j] not in ",);":
                j += 1
            nodes[last][1] = float(text[i + 1:j])
            i = j
        elif ch == ";":
            break
        else:
            j = i
            while text[j] not in ":,);":
                j += 1
            nodes.append([stack[-1], 0.0, text[i:j]])
            last = len(nodes) - 1
            names.append(text[i:j])
            i = j
    tips = [k for k, nd in enumerate(nodes) if nd[2] is not None]
    n = len(tips)
    P, E = np.zeros((n, n)), np.zeros((n, n), dtype=np.int64)
    paths = []
    for t in tips:
        path, v, acc, k = {}, t, 0.0, 0
        while v != -1:
            path[v] = (acc, k)
            acc, k, v = acc + nodes[v][1], k + 1, nodes[v][0]
        paths.append(path)
    for a in range(n):
        for b in range(a):
            v = tips[b]
            while v not in paths[a]:
                v = nodes[v][0]
            P[a, b] = P[b, a] = paths[a][v][0] + paths[b][v][0]
            E[a, b] = E[b, a] = paths[a][v][1] + paths[b][v][1]
    return names, P, E
