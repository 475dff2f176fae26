"""Helpers of the transfer bootstrap expectation (TBE) tests: merge-log tree shapes, phi by Python sets straight from the
definition, and TBE labels recomputed from Newick text."""
import heapq

import numpy as np

from tests import _util

U64 = np.uint64


# ---- merge logs (slots as dpr_nj_run writes them: 0 <= x < y < n - it) ------------------------------------------------------
def random_log(rng, n):
    k = max(n - 2, 1)
    it = np.arange(n - 2)
    y = 1 + np.floor(rng.random(n - 2) * (n - it - 1)).astype(np.int64)
    x = np.floor(rng.random(n - 2) * y).astype(np.int64)
    mx, my = np.zeros(k, np.int32), np.zeros(k, np.int32)
    mx[: n - 2], my[: n - 2] = x, y
    return mx, my


def caterpillar_log(n):
    """every merge joins the last node made with the next tip: depth n"""
    k = max(n - 2, 1)
    return np.zeros(k, np.int32), np.ones(k, np.int32)


def balanced_log(n):
    """the two smallest clades merge first (Huffman order): depth ~ log2 n"""
    k = max(n - 2, 1)
    mx, my = np.zeros(k, np.int32), np.zeros(k, np.int32)
    slot_of = list(range(n))                    # node -> slot
    at = list(range(n))                         # slot -> node
    heap = [(1, t) for t in range(n)]
    heapq.heapify(heap)
    for it in range(n - 2):
        sa, a = heapq.heappop(heap)
        sb, b = heapq.heappop(heap)
        x, y = sorted((slot_of[a], slot_of[b]))
        mx[it], my[it] = x, y
        last = n - it - 1
        v = n + it
        slot_of.append(0)
        at[x] = v
        slot_of[v] = x
        moved = at[last]
        if y != last:
            at[y] = moved
            slot_of[moved] = y
        heapq.heappush(heap, (sa + sb, v))
    return mx, my


def shared_prefix(rng, n, mx, my):
    """a replicate whose first merges are the main tree's: most clades close, some exact"""
    rx, ry = random_log(rng, n)
    cut = int(rng.integers(0, max(n - 1, 1)))
    rx[:cut], ry[:cut] = mx[:cut], my[:cut]
    return rx, ry


def clades(n, mx, my):
    """tips below every node 0 .. 2n-3 (realID bookkeeping of writeNewickFromMerges)"""
    real = list(range(n))
    below = [frozenset([t]) for t in range(n)]
    for it in range(n - 2):
        x, y = int(mx[it]), int(my[it])
        below.append(below[real[x]] | below[real[y]])
        real[x] = n + it
        real[y] = real[n - it - 1]
    return below


def phi_brute(n, mx, my, rx, ry):
    """{k: phi} for the main nodes n+k with p >= 2, from the definition with sets"""
    A, L = clades(n, mx, my), clades(n, rx, ry)
    out = {}
    for k in range(n - 2):
        a = A[n + k]
        if min(len(a), n - len(a)) < 2:
            continue
        best = n
        for lv in L:
            h = len(a) + len(lv) - 2 * len(a & lv)
            best = min(best, h, n - h)
        out[k] = best
    return out


def p_of(n, mx, my):
    """p = min(|A|, n - |A|) of every main internal node n+k"""
    A = clades(n, mx, my)
    return [min(len(A[n + k]), n - len(A[n + k])) for k in range(n - 2)]


# ---- labels from Newick text ------------------------------------------------------------------------------------------------
def tree_nodes(text, names):
    """DFS leaf order of a Newick tree: (rank of every name index, [(start, end, label, is_leaf)] of every node below the root)"""
    kids, _, name, root = _util.parse_newick(text)
    idx = {nm: i for i, nm in enumerate(names)}
    rank = np.zeros(len(names), np.int64)
    nodes, pos = [], 0
    st = [(root, 0)]
    start = {}
    while st:
        v, state = st.pop()
        if state == 0:
            start[v] = pos
            if not kids[v]:
                rank[idx[name[v]]] = pos
                pos += 1
                if v != root:
                    nodes.append((start[v], pos, None, True))
                continue
            st.append((v, 1))
            for c in reversed(kids[v]):
                st.append((c, 0))
        elif v != root:
            nodes.append((start[v], pos, name.get(v), False))
    assert pos == len(names)
    return rank, nodes


def tbe_expected(main_text, rep_texts, names):
    """[(clade as a frozenset of name indices, label in main_text, expected TBE label or None)] of every internal node below the
    root of main_text; phi of every replicate from its Newick text (numpy prefix counts over the replicate's DFS order)"""
    n, R = len(names), len(rep_texts)
    mrank, mnodes = tree_nodes(main_text, names)
    leaf_at = np.argsort(mrank)
    internal = [(s, e, lab) for s, e, lab, leaf in mnodes if not leaf]
    S = np.zeros(len(internal), np.int64)
    reps = []
    for text in rep_texts:
        rrank, rnodes = tree_nodes(text, names)
        m_at = np.empty(n, np.int64)
        m_at[rrank] = mrank                      # main rank of the leaf at every replicate position
        iv = np.array([(s, e) for s, e, _, _ in rnodes], np.int64)
        reps.append((m_at, iv[:, 0], iv[:, 1]))
    out = []
    for j, (s0, e0, lab) in enumerate(internal):
        a = e0 - s0
        p = min(a, n - a)
        clade = frozenset(int(t) for t in leaf_at[s0:e0])
        if p < 2:
            out.append((clade, lab, None))
            continue
        total = 0
        for m_at, rs, re_ in reps:
            pre = np.concatenate([[0], np.cumsum((m_at >= s0) & (m_at < e0))])
            h = a + (re_ - rs) - 2 * (pre[re_] - pre[rs])
            total += int(np.minimum(h, n - h).min())
        den = R * (p - 1)
        out.append((clade, lab, (200 * (den - total) + den) // (2 * den)))
    return out


# ---- replicate alignments (the column sample of dpr_msa_boot_weights, restated) -----------------------------------------------
def _mix64(z):
    z = z + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def boot_weights(seed, r, L):
    with np.errstate(over="ignore"):
        key = _mix64(np.array([seed], dtype=U64) ^ _mix64(np.array([r], dtype=U64)))[0]
        col = ((_mix64(np.arange(L, dtype=U64) ^ key) >> U64(32)) * U64(L)) >> U64(32)
    return np.bincount(col.astype(np.int64), minlength=L)


def replicate_seqs(seqs, seed, r):
    L = len(seqs[0])
    idx = np.repeat(np.arange(L), boot_weights(seed, r, L))
    return [np.frombuffer(s, dtype=np.uint8)[idx].tobytes() for s in seqs]


def read_fasta(path):
    names, seqs, cur = [], [], []
    for line in open(path, "rb"):
        line = line.strip()
        if line.startswith(b">"):
            if names:
                seqs.append(b"".join(cur))
            names.append(line[1:].split()[0].decode())
            cur = []
        elif line:
            cur.append(line)
    seqs.append(b"".join(cur))
    return names, seqs
