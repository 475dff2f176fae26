"""Textbook balanced minimum evolution in NumPy (Desper & Gascuel 2002; Pauplin 2000), written without the recursions of the
library: the reference of tests/test_bme_nni.py.

A tree is (kids, top): kids[k] = the two children of internal node n + k when the tree hangs from tip t0 = n - 1, top = the node
next to t0.  Everything below works on the unrooted tree behind that table:
  path lengths      edges between every pair of tips, by BFS;
  L                 Pauplin's closed form, sum over i < j of 2^(1 - p_ij) D_ij;
  edge lengths      the balanced formulas over subtree averages, each average a direct sum over tip pairs with weights
                    2^-(depth in its subtree): delta(X, Y) = sum 2^-(d(x, i) + d(y, j)) D_ij;
  gain of a move    L(T) - L(T after the move), two closed forms;
  the search        the contract of include/dipper_hip.h (candidates, selection by shared endpoints, fallback) run on those gains."""
import numpy as np


def random_matrix(rng, n, noise=0.3):
    """additive distances of a random tree times log-normal noise; symmetric, zero diagonal"""
    from tests import _util
    D = _util.random_additive_matrix(rng, n)
    E = np.tril(rng.normal(size=(n, n)), -1)
    D = D * np.exp(noise * (E + E.T))
    np.fill_diagonal(D, 0.0)
    return D


def tree_from_merges(n, mx, my):
    """(kids, top) of a merge log hung from tip n - 1 (internal node n + k = merge k; the last two nodes share an edge)"""
    adj = {v: [] for v in range(2 * n - 2)}
    real = list(range(n))
    for it in range(n - 2):
        x, y = int(mx[it]), int(my[it])
        node = n + it
        for w in (real[x], real[y]):
            adj[node].append(w)
            adj[w].append(node)
        real[x] = node
        real[y] = real[n - it - 1]
    adj[real[0]].append(real[1])
    adj[real[1]].append(real[0])
    return root_at(n, adj)


def root_at(n, adj):
    t0 = n - 1
    top = adj[t0][0]
    kids = np.zeros((n - 2, 2), dtype=np.int32)
    stack = [(top, t0)]
    while stack:
        v, p = stack.pop()
        if v < n:
            continue
        ch = sorted(w for w in adj[v] if w != p)
        kids[v - n] = ch
        stack += [(c, v) for c in ch]
    return kids, top


def adjacency(n, kids, top):
    adj = {v: [] for v in range(2 * n - 2)}
    for k in range(n - 2):
        for c in kids[k]:
            adj[n + k].append(int(c))
            adj[int(c)].append(n + k)
    adj[n - 1].append(int(top))
    adj[int(top)].append(n - 1)
    return adj


def parents(n, kids, top):
    par = {n - 1: int(top), int(top): n - 1}
    for k in range(n - 2):
        for c in kids[k]:
            par[int(c)] = n + k
    return par


def depths(adj, root, banned, n):
    """{tip: edges from root} over the subtree behind `root` as seen from `banned`"""
    out, stack = {}, [(root, banned, 0)]
    while stack:
        v, p, d = stack.pop()
        if v < n:
            out[v] = d
        stack += [(w, v, d + 1) for w in adj[v] if w != p]
    return out


def pauplin(n, kids, top, D):
    adj = adjacency(n, kids, top)
    L = 0.0
    for i in range(n):
        d = depths(adj, adj[i][0], i, n)
        for j, p in d.items():
            if j > i:
                L += 2.0 ** (1 - (p + 1)) * D[i, j]
    return L


def delta(D, da, db):
    return sum(2.0 ** -(pa + pb) * D[i, j] for i, pa in da.items() for j, pb in db.items())


def edge_lengths(n, kids, top, D):
    """balanced length of the edge above every node (index t0 = n - 1: 0)"""
    adj, par = adjacency(n, kids, top), parents(n, kids, top)
    out = np.zeros(2 * n - 2)
    for v in range(2 * n - 2):
        if v == n - 1:
            continue
        p = par[v]
        if p == n - 1:                       # the pendant edge of t0, seen from the other end
            v, p = n - 1, v
        sub = lambda x, frm: depths(adj, x, frm, n)
        if v < n:
            a, b = (w for w in adj[p] if w != v)
            me = {v: 0}
            val = 0.5 * (delta(D, me, sub(a, p)) + delta(D, me, sub(b, p)) - delta(D, sub(a, p), sub(b, p)))
        else:
            a, b = (w for w in adj[v] if w != p)
            c, d = (w for w in adj[p] if w != v)
            A, B, C, Dd = sub(a, v), sub(b, v), sub(c, p), sub(d, p)
            val = 0.25 * (delta(D, A, C) + delta(D, B, C) + delta(D, A, Dd) + delta(D, B, Dd)) - 0.5 * (delta(D, A, B) + delta(D, C, Dd))
        out[par[n - 1] if v == n - 1 else v] = val
    return out


def moved(n, kids, top, v, move):
    """the tree after move 1 (the larger child of v changes place with v's sibling) or 2 (the smaller child) of node v"""
    par = parents(n, kids, top)
    p = par[v]
    A, B = sorted(int(c) for c in kids[v - n])
    C = [int(c) for c in kids[p - n] if c != v][0]
    X, keep = (B, A) if move == 1 else (A, B)
    out = kids.copy()
    out[v - n] = sorted((keep, C))
    out[p - n] = sorted((v, X))
    return out


def gains(n, kids, top, D):
    """{v: (g1, g2)} for every internal v whose parent is not t0, each the difference of two Pauplin lengths"""
    par = parents(n, kids, top)
    L = pauplin(n, kids, top, D)
    return {v: tuple(L - pauplin(n, moved(n, kids, top, v, m), top, D) for m in (1, 2))
            for v in range(n, 2 * n - 2) if par[v] != n - 1}


def candidates(n, kids, top, D):
    """{v: (move, gain)} and the smallest distance of any decision from a tie: a gain from 0, g1 from g2, a candidate's gain from a
    competing one at a shared endpoint"""
    par = parents(n, kids, top)
    cand, gap = {}, np.inf
    for v, (g1, g2) in gains(n, kids, top, D).items():
        m, g = (1, g1) if g1 >= g2 else (2, g2)
        gap = min(gap, abs(g), abs(g1 - g2) if max(g1, g2) > 0 else np.inf)
        if g > 0:
            cand[v] = (m, g)
    for v in cand:
        for f in cand:
            if f != v and {f, par[f]} & {v, par[v]}:
                gap = min(gap, abs(cand[f][1] - cand[v][1]))
    return cand, gap


def select(n, kids, top, cand):
    par = parents(n, kids, top)
    better = lambda f, v: cand[f][1] > cand[v][1] or (cand[f][1] == cand[v][1] and f < v)
    return [v for v in sorted(cand) if not any(f != v and ({f, par[f]} & {v, par[v]}) and better(f, v) for f in cand)]


def search(n, kids, top, D, max_rounds):
    """the contract's loop on textbook gains and Pauplin lengths.  dict(trees: (kids, top) after 0, 1, .. accepted rounds; L: the
    same for the length; picked: per accepted round the [(v, move)] applied; fallbacks; gap: smallest distance from a tie met)"""
    L = pauplin(n, kids, top, D)
    res = dict(trees=[(kids.copy(), top)], L=[L], picked=[], fallbacks=0, gap=np.inf)
    while len(res["picked"]) < max_rounds:
        cand, gap = candidates(n, kids, top, D)
        res["gap"] = min(res["gap"], gap)
        if not cand:
            break
        picked = [(v, cand[v][0]) for v in select(n, kids, top, cand)]
        new = kids
        for v, m in picked:
            new = moved(n, new, top, v, m)
        Ln = pauplin(n, new, top, D)
        if not Ln < L:
            res["fallbacks"] += 1
            best = max(cand, key=lambda v: (cand[v][1], -v))
            picked = [(best, cand[best][0])]
            new = moved(n, kids, top, *picked[0])
            Ln = pauplin(n, new, top, D)
            if not Ln < L:
                break
        res["gap"] = min(res["gap"], abs(L - Ln))
        kids, L = new, Ln
        res["trees"].append((kids.copy(), top))
        res["L"].append(L)
        res["picked"].append(picked)
    return res


def caterpillar_log(n):
    """merge log of the caterpillar (((0,1),2),3).. : depth n"""
    # (slot 0 holds the growing clade; after a merge the last slot moves into slot 1)
    return np.zeros(n - 2, dtype=np.int32), np.ones(n - 2, dtype=np.int32)


def balanced_log(n):
    """merge log that always joins the two shallowest slots: depth about log2 n"""
    mx, my, h = [], [], [0] * n
    for _ in range(n - 2):
        x, y = sorted(sorted(range(len(h)), key=lambda i: (h[i], i))[:2])
        mx.append(x)
        my.append(y)
        h[x] = max(h[x], h[y]) + 1
        h[y] = h[-1]
        h.pop()
    return np.array(mx, dtype=np.int32), np.array(my, dtype=np.int32)


def newick(names, kids, top, length, fmt=None):
    """the command's text for a (kids, top, len) result: the root joins name[n-1] and top, each with half of len[top]"""
    from tests import _util
    fmt = fmt or _util.fmt
    n = len(names)

    def sub(v):                               # (iterative: a caterpillar is as deep as it has tips)
        out, stack = [], [v]
        while stack:
            w = stack.pop()
            if isinstance(w, str):
                out.append(w)
            elif w < n:
                out.append(names[w])
            else:
                a, b = (int(c) for c in kids[w - n])
                stack += [")", ":" + fmt(length[b]), b, ",", ":" + fmt(length[a]), a, "("]
        return "".join(out)

    h = fmt(length[top] * 0.5)
    return "(" + names[n - 1] + ":" + h + "," + sub(int(top)) + ":" + h + ");\n"
