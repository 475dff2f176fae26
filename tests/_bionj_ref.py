"""Textbook BIONJ (Gascuel 1997, Mol. Biol. Evol. 14:685-695) in plain Python over NumPy arrays: the reference of
tests/test_bionj.py.  Nothing of the library's canonical summation orders, slot moves or tie-break keys is restated here: nodes
live in a list, sums are Python's sum(), the best pair is the smallest Q.

    Q_ij   = d_ij - S_i / (m - 2) - S_j / (m - 2)                    S_i = sum_k d_ik, m active nodes
    b_i    = (d_ij + S_i / (m - 2) - S_j / (m - 2)) / 2,  b_j = d_ij - b_i
    lambda = 1/2 + sum_{k != i,j} (v_jk - v_ik) / (2 (m - 2) v_ij), clamped to [0, 1]; 1/2 where v_ij = 0
    d_uk   = lambda (d_ik - b_i) + (1 - lambda) (d_jk - b_j)
    v_uk   = lambda v_ik + (1 - lambda) v_jk - lambda (1 - lambda) v_ij,  v = d at the start

The lengths a merge reports are clamped the way the library's merge log defines them (a negative length becomes 0 and is
taken off its sibling); the update uses the unclamped ones, as the formulas above say."""
import numpy as np


def bionj(D0, variant=1, follow=None):
    """variant 1: BIONJ, 0: NJ (lambda = 1/2 throughout, no variances).
    Returns dict(merges=[(node_a, node_b, len_a, len_b, lambda)], last=(node_a, node_b, d), splits=set of frozensets (the side
    without tip 0), min_gap=smallest difference between the best and the second-best unordered pair's Q over the run).
    Tips are nodes 0 .. n-1, merge t creates node n + t.

    Two ties are identities of the criterion, whatever the distances, and are left out of min_gap:
      m = 4: Q_ij = Q_kl = -(d_ik + d_il + d_jk + d_jl) / 2 for the complementary pair kl (both name the same split);
             the gap of that step is taken to the best pair that is neither the winner nor its complement;
      m = 3: all three Q equal -(d_ij + d_ik + d_jk) (one tree).
    Which of the tied pairs is joined does not change the tree, but it does change which two nodes a log entry names and
    (on a matrix that is no tree metric) the lengths.  follow = [(node_a, node_b)] * (n - 2), the pairs of another run:
    at m <= 4 this run joins the pair named there, after checking that its Q is within 1e-12 of the smallest."""
    n = D0.shape[0]
    D = np.array(D0, dtype=np.float64)
    V = D.copy()
    ids = list(range(n))
    clade = {i: frozenset([i]) for i in range(n)}
    merges, min_gap = [], float("inf")
    while len(ids) > 2:
        m = len(ids)
        S = [sum(float(D[i, k]) for k in range(m) if k != i) for i in range(m)]
        qs = sorted((float(D[i, j]) - S[i] / (m - 2) - S[j] / (m - 2), i, j) for i in range(m) for j in range(i + 1, m))
        _, i, j = qs[0]
        if m >= 5:
            min_gap = min(min_gap, qs[1][0] - qs[0][0])
        elif m == 4:
            min_gap = min(min_gap, min(q for q, a, b in qs if len({a, b} & {i, j}) == 1) - qs[0][0])
        if m <= 4 and follow is not None:
            want = set(follow[len(merges)])
            q, i, j = next(t for t in qs if {ids[t[1]], ids[t[2]]} == want)
            assert q - qs[0][0] <= 1e-12, (m, q, qs[0])
        d = float(D[i, j])
        bi = (d + S[i] / (m - 2) - S[j] / (m - 2)) / 2
        bj = d - bi
        lam = 0.5
        if variant == 1 and V[i, j] != 0.0:
            lam = 0.5 + sum(float(V[j, k] - V[i, k]) for k in range(m) if k not in (i, j)) / (2 * (m - 2) * float(V[i, j]))
            lam = min(1.0, max(0.0, lam))
        li, lj = bi, bj
        if li < 0:
            lj += li
            li = 0.0
        if lj < 0:
            li += lj
            lj = 0.0
        new = n + len(merges)
        merges.append((ids[i], ids[j], li, lj, lam))
        clade[new] = clade[ids[i]] | clade[ids[j]]
        du = lam * (D[i] - bi) + (1 - lam) * (D[j] - bj)
        vu = lam * V[i] + (1 - lam) * V[j] - lam * (1 - lam) * V[i, j]
        D[i, :] = du
        D[:, i] = du
        V[i, :] = vu
        V[:, i] = vu
        D[i, i] = V[i, i] = 0.0
        keep = [k for k in range(m) if k != j]
        D = D[np.ix_(keep, keep)]
        V = V[np.ix_(keep, keep)]
        ids[i] = new
        del ids[j]
    full = frozenset(range(n))
    splits = {c if 0 not in c else full - c for c in clade.values() if 1 < len(c) < n - 1}
    return dict(merges=merges, last=(ids[0], ids[1], float(D[0, 1])), splits=splits, min_gap=min_gap)


def log_nodes(n, mx, my):
    """node ids (tips 0 .. n-1, merge t creates n + t) of the two slots every entry of a merge log joins, and of the last pair"""
    real = list(range(n))
    out = []
    for it in range(len(mx)):
        x, y = int(mx[it]), int(my[it])
        out.append((real[x], real[y]))
        real[x] = n + it
        real[y] = real[n - it - 1]
    return out, (real[0], real[1])


def random_matrix(rng, n):
    """symmetric, zero diagonal, off-diagonal U(0.1, 1): far from a tree metric"""
    D = rng.uniform(0.1, 1.0, size=(n, n))
    D = np.tril(D, -1)
    return D + D.T


def additive_with_tree(rng, n):
    """(patristic distance matrix of a random binary tree with branch lengths U(0.05, 1), its non-trivial splits as the side
    without tip 0): a random cherry-joining history, so no restated tree code of the tests' other helpers"""
    nodes = [frozenset([i]) for i in range(n)]
    depth = {i: 0.0 for i in range(n)}        # tip -> distance to the root of its current clade
    D = np.zeros((n, n))
    splits = set()
    full = frozenset(range(n))
    while len(nodes) > 2:
        a, b = (int(v) for v in rng.choice(len(nodes), size=2, replace=False))
        A, B = nodes[a], nodes[b]
        la, lb = (float(v) for v in rng.uniform(0.05, 1.0, size=2))
        for i in A:
            depth[i] += la
        for i in B:
            depth[i] += lb
        for i in A:
            for j in B:
                D[i, j] = D[j, i] = depth[i] + depth[j]
        C = A | B
        nodes = [c for k, c in enumerate(nodes) if k not in (a, b)] + [C]
        if 1 < len(C) < n - 1:
            splits.add(C if 0 not in C else full - C)
    A, B = nodes
    lab = float(rng.uniform(0.05, 1.0))
    for i in A:
        for j in B:
            D[i, j] = D[j, i] = depth[i] + depth[j] + lab
    return D, splits
