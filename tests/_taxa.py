"""Helpers of the per-taxon transfer index tests (`dpr_transfer_taxa`, `dipper --bootstrap-taxa`): the definition of DESIGN
§10.2 restated with Python sets straight from `_tbe.clades`, merge logs from lists of node merges, and the report recomputed
from Newick text."""
import numpy as np

from tests import _tbe


# ---- merge logs from node merges --------------------------------------------------------------------------------------------
def log_from_merges(n, pairs):
    """slot merge log of the tree whose it-th merge joins nodes pairs[it] = (a, b) into node n+it (n - 2 merges; the two nodes
    left over meet at the root); the slot bookkeeping of _tbe.balanced_log"""
    assert len(pairs) == n - 2
    k = max(n - 2, 1)
    mx, my = np.zeros(k, np.int32), np.zeros(k, np.int32)
    slot_of = list(range(n))                    # node -> slot
    at = list(range(n))                         # slot -> node
    for it, (a, b) in enumerate(pairs):
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
    return mx, my


def caterpillar_of(order):
    """merge log of the caterpillar that joins the tips in `order`: ((o0, o1), o2), ... ; the last tip meets the rest at the root"""
    n = len(order)
    pairs, prev = [], order[0]
    for i in range(1, n - 1):
        pairs.append((prev, order[i]))
        prev = n + i - 1
    return log_from_merges(n, pairs)


def prune_regraft(rng, n, mx, my, tip):
    """node merges of the tree of (mx, my) with `tip` pruned and regrafted on a random other branch, as a merge log of n tips"""
    real = list(range(n))
    kids = {}
    for it in range(n - 2):
        x, y = int(mx[it]), int(my[it])
        kids[n + it] = [real[x], real[y]]
        real[x] = n + it
        real[y] = real[n - it - 1]
    root = 2 * n - 2
    kids[root] = [real[0], real[1]]
    parent = {c: v for v, cs in kids.items() for c in cs}
    # prune: the tip's parent goes, its sibling takes the parent's place
    par = parent[tip]
    sib = [c for c in kids[par] if c != tip][0]
    if par == root:
        assert sib >= n
        kids[root] = list(kids[sib])
        del kids[sib]
    else:
        g = parent[par]
        kids[g] = [sib if c == par else c for c in kids[g]]
        del kids[par]
    # regraft above a random node below the root
    parent = {c: v for v, cs in kids.items() for c in cs}
    targets = sorted(parent)
    at = targets[int(rng.integers(0, len(targets)))]
    new = max(kids) + 1
    g = parent[at]
    kids[g] = [new if c == at else c for c in kids[g]]
    kids[new] = [at, tip]
    # node merges in post-order, the root's children last and not merged
    name, pairs = {}, []
    st = [(c, 0) for c in kids[root]]
    while st:
        v, state = st.pop()
        if v < n:
            name[v] = v
        elif state == 0:
            st.append((v, 1))
            st.extend((c, 0) for c in kids[v])
        else:
            name[v] = n + len(pairs)
            pairs.append((name[kids[v][0]], name[kids[v][1]]))
    return log_from_merges(n, pairs)


# ---- the definition with sets -----------------------------------------------------------------------------------------------
def root_children(n, mx, my):
    real = list(range(n))
    for it in range(n - 2):
        real[int(mx[it])] = n + it
        real[int(my[it])] = real[n - it - 1]
    return real[0], real[1]


def branches(n, mx, my):
    """k of the main nodes n+k that are branches: p >= 2, and of two such root children the smaller node number only"""
    A = _tbe.clades(n, mx, my)
    ks = [k for k in range(n - 2) if min(len(A[n + k]), n - len(A[n + k])) >= 2]
    a, b = root_children(n, mx, my)
    if a >= n and b >= n and a - n in ks and b - n in ks:
        ks.remove(max(a, b) - n)
    return ks


def canonical_key(lv, n):
    s = lv if 0 not in lv else frozenset(range(n)) - lv
    return (min(s), len(s))


def transfer_sets(n, mx, my, rx, ry, cutoff):
    """{k: (phi, T)} of the counted branches, T a frozenset of tips"""
    A, L = _tbe.clades(n, mx, my), _tbe.clades(n, rx, ry)
    everything = frozenset(range(n))
    out = {}
    for k in branches(n, mx, my):
        a = A[n + k]
        p = min(len(a), n - len(a))
        delta = []
        for lv in L:
            h = len(a) + len(lv) - 2 * len(a & lv)
            delta.append(min(h, n - h))
        phi = min(delta)
        if 1000 * phi > cutoff * (p - 1):
            continue
        close = [v for v in range(n, 2 * n - 2) if delta[v] == phi]
        assert close, "a counted pair has an internal closest node"
        v = min(close, key=lambda u: canonical_key(L[u], n))
        h = len(a) + len(L[v]) - 2 * len(a & L[v])
        assert h != n - h
        T = a ^ L[v] if h < n - h else a ^ (everything - L[v])
        assert len(T) == phi
        out[k] = (phi, T)
    return out


def taxa_brute(n, mx, my, rx, ry, cutoff):
    """(moved, pairs, sum of phi over the counted pairs) from the definition with sets"""
    moved = np.zeros(n, np.int64)
    sets = transfer_sets(n, mx, my, rx, ry, cutoff)
    for phi, T in sets.values():
        for t in T:
            moved[t] += 1
    return moved, len(sets), sum(phi for phi, _ in sets.values())


# ---- the report from Newick text --------------------------------------------------------------------------------------------
def _min_over(values, s, e):
    """min of values[s:e] for arrays of intervals (e > s)"""
    idx = np.stack([s, e], axis=1).ravel()
    ext = np.concatenate([values, [values.max() + 1]])
    return np.minimum.reduceat(ext, idx)[::2]


def taxa_from_newick(main_text, rep_texts, names, cutoff):
    """(moved by name index, pairs, B): the definition recomputed from the trees' text; tip t is names[t]"""
    n = len(names)
    mrank, mnodes = _tbe.tree_nodes(main_text, names)
    internal = [(s, e) for s, e, _, leaf in mnodes if not leaf and min(e - s, n - (e - s)) >= 2]
    # the root's two children: [0, x) and [x, n); two branches of one bipartition count once
    listed = set(internal)
    for s, e in internal:
        if s == 0 and (e, n) in listed:
            internal.remove((e, n))
            break
    moved, pairs = np.zeros(n, np.int64), 0
    for text in rep_texts:
        rrank, rnodes = _tbe.tree_nodes(text, names)
        tip_at = np.argsort(rrank)                       # tip at every replicate position
        m_at = mrank[tip_at]                             # main rank of the tip at every replicate position
        iv = np.array([(s, e) for s, e, _, leaf in rnodes if not leaf], np.int64)
        rs, re_ = iv[:, 0], iv[:, 1]
        # canonical key of every internal replicate node: the side without tip 0
        has0 = (rs <= rrank[0]) & (rrank[0] < re_)
        pre = np.concatenate([[n], np.minimum.accumulate(tip_at)])              # min of tip_at[:i]
        suf = np.concatenate([np.minimum.accumulate(tip_at[::-1])[::-1], [n]])  # min of tip_at[i:]
        low = np.where(has0, np.minimum(pre[rs], suf[re_]), _min_over(tip_at, rs, re_))
        size = np.where(has0, n - (re_ - rs), re_ - rs)
        key = low * (n + 1) + size
        for s0, e0 in internal:
            a = e0 - s0
            p = min(a, n - a)
            in_a = (m_at >= s0) & (m_at < e0)
            cum = np.concatenate([[0], np.cumsum(in_a)])
            h = a + (re_ - rs) - 2 * (cum[re_] - cum[rs])
            delta = np.minimum(h, n - h)
            phi = min(int(delta.min()), p - 1)
            if 1000 * phi > cutoff * (p - 1):
                continue
            close = np.flatnonzero(delta == phi)
            v = close[np.argmin(key[close])]
            in_l = np.zeros(n, bool)
            in_l[rs[v]:re_[v]] = True
            t_set = (in_a != in_l) != (h[v] > n - h[v])
            assert int(t_set.sum()) == phi
            moved[tip_at[t_set]] += 1
            pairs += 1
    return moved, pairs, len(internal)


def index_text(moved, pairs):
    """the six-decimal transfer index as the command prints it"""
    if pairs == 0:
        return "0.000000"
    q = (int(moved) * 10**6 + pairs // 2) // pairs
    return "%d.%06d" % (q // 10**6, q % 10**6)


def read_report(path):
    """(header fields as a dict of strings, [(name, moved, index text)]) of a --bootstrap-taxa file"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# dipper transfer index: ") and lines[1] == "taxon\tmoved\tindex"
    head = dict(f.split("=") for f in lines[0][len("# dipper transfer index: "):].split(" "))
    rows = [l.split("\t") for l in lines[2:-1]]
    return head, [(r[0], int(r[1]), r[2]) for r in rows]
