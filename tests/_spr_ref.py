"""Textbook SPR moves for balanced minimum evolution, without any table of subtree averages: the reference of
tests/test_bme_spr.py.  A move is carried out on the adjacency list of the unrooted tree and its gain is the difference of two
Pauplin lengths, each a sum over tip pairs of 2^(1 - edges between them) D_ij with the path lengths found by BFS.

Numbering as in include/dipper_hip.h above dpr_bme_spr: the tree hangs from t0 = n - 1; directed subtree d = v is the clade of v,
d = (2n - 2) + v everything outside the clade of v; a target is named by w, the lower node of its edge."""
import numpy as np

from tests import _bme_ref as R


def pauplin_adj(n, adj, D):
    L = 0.0
    for i in range(n):
        for j, p in R.depths(adj, adj[i][0], i, n).items():
            if j > i:
                L += 2.0 ** (1 - (p + 1)) * D[i, j]
    return L


def apply_nodes(adj, nodes):
    """a copy of adj after the move with the node set [x0, a0, q, p_1 .. p_k, b0]: q leaves between a0 and p_1 and enters
    between p_k and b0"""
    new = {v: list(ws) for v, ws in adj.items()}
    a0, q, p1, pk, b0 = nodes[1], nodes[2], nodes[3], nodes[-2], nodes[-1]

    def cut(a, b):
        new[a].remove(b)
        new[b].remove(a)

    def join(a, b):
        new[a].append(b)
        new[b].append(a)

    cut(q, a0)
    cut(q, p1)
    join(a0, p1)
    cut(pk, b0)
    join(pk, q)
    join(q, b0)
    return new


def all_moves(n, kids, top):
    """{(d, w): node set [x0, a0, q, p_1 .. p_k, b0]} of every SPR move of the tree"""
    adj, par = R.adjacency(n, kids, top), R.parents(n, kids, top)
    M, t0 = 2 * n - 2, n - 1
    out = {}
    for q in range(n, M):
        for x0 in adj[q]:
            d = M + top if x0 == t0 else x0 if par[x0] == q else M + q
            for p1 in adj[q]:
                if p1 == x0 or p1 < n:
                    continue
                a0 = [v for v in adj[q] if v not in (x0, p1)][0]
                stack = [[q, p1]]
                while stack:
                    path = stack.pop()
                    pk = path[-1]
                    for b0 in adj[pk]:
                        if b0 == path[-2]:
                            continue
                        w = pk if par[pk] == b0 else b0          # the lower node; the edge at t0 is the one above top
                        assert (d, w) not in out and w != t0
                        out[(d, w)] = [x0, a0] + path + [b0]
                        if b0 >= n:
                            stack.append(path + [b0])
    return out


def gains(n, kids, top, D):
    """{(d, w): (L(T) - L(T after the move), k)}"""
    adj = R.adjacency(n, kids, top)
    L = pauplin_adj(n, adj, D)
    return {dw: (L - pauplin_adj(n, apply_nodes(adj, nodes), D), len(nodes) - 4) for dw, nodes in all_moves(n, kids, top).items()}


def select(cands, moves):
    """the contract's selection: cands {d: (gain, w)} in the order (gain descending, d ascending), each taken iff its node set is
    free; [(d, w)]"""
    used, picked = set(), []
    for d in sorted(cands, key=lambda d: (-cands[d][0], d)):
        nodes = set(moves[(d, cands[d][1])])
        if not nodes & used:
            used |= nodes
            picked.append((d, cands[d][1]))
    return picked


def moved(n, kids, top, moves, picked):
    """(kids, top) after the picked moves, hung from t0 again"""
    adj = R.adjacency(n, kids, top)
    for dw in picked:
        adj = apply_nodes(adj, moves[dw])
    return R.root_at(n, adj)


def integer_matrix(rng, n, hi=4):
    """symmetric, zero diagonal, whole numbers 1 .. hi: gains of small trees are exact, and tie"""
    D = np.triu(rng.integers(1, hi + 1, size=(n, n)).astype(np.float64), 1)
    return D + D.T
