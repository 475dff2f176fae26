"""Helpers of the fixed-backbone placement tests (`-o j`, dpr_place_fixed_*): seeded rooted binary backbones as Newick, the
importer's adjacency arrays of a backbone, the edge numbering of a jplace tree string, and the bootstrap tally of the
command restated in Python."""
import math
import re

import numpy as np

from tests import _util


def random_backbone(rng, m, kind, zero_frac=0.2, prefix="B", max_len=0.05):
    """Newick of a rooted binary tree with m >= 2 leaves.  kind: caterpillar | balanced | random.  Leaves are named
    prefix + index of appearance (= the importer's tip index); lengths have four decimals (exact as binary32 -> the text
    the importer reads is what a "%g" of the stored value gives back), drawn from [0.001, max_len], zero_frac of them are 0."""
    def length():
        return 0.0 if rng.random() < zero_frac else round(float(rng.uniform(0.001, max_len)), 4)

    if kind == "caterpillar":
        tree = 0
        for k in range(1, m):
            tree = (tree, k)
    elif kind == "balanced":
        def build(lo, hi):
            return lo if hi - lo == 1 else (build(lo, (lo + hi) // 2), build((lo + hi) // 2, hi))
        tree = build(0, m)
    elif kind == "random":
        parts = list(range(m))
        while len(parts) > 1:
            i, j = sorted(int(x) for x in rng.choice(len(parts), size=2, replace=False))
            b = parts.pop(j)
            a = parts.pop(i)
            parts.append((a, b) if rng.random() < 0.5 else (b, a))
        tree = parts[0]
    else:
        raise ValueError(kind)
    # text, iteratively (a caterpillar of 300 leaves is 300 levels deep); leaves renamed in order of appearance
    out, count = [], [0]
    stack = [("node", tree, True)]
    while stack:
        what, v, is_root = stack.pop()
        if what == "text":
            out.append(v)
        elif isinstance(v, tuple):
            out.append("(")
            stack.append(("text", ")" + ("" if is_root else ":%g" % length()), False))
            stack.append(("node", v[1], False))
            stack.append(("text", ",", False))
            stack.append(("node", v[0], False))
        else:
            out.append("%s%d:%g" % (prefix, count[0], length()))
            count[0] += 1
    return "".join(out) + ";"


def backbone_arrays(orc, newick, n):
    """the importer's adjacency arrays (sized for n tips, internal node ids from n) and the leaf names by tip index"""
    return _util.backbone_state(orc, newick, n)


def leaves_below_slot(state, slot, names):
    """names of the backbone leaves below edge slot >> 1: behind its child end (slot 2k leads from the child to the parent)"""
    head, e, nxt, belong = state["head"], state["e"], state["nxt"], state["belong"]
    k = int(slot) >> 1
    child, parent = int(belong[2 * k]), int(e[2 * k])
    out, stack = [], [(child, parent)]
    while stack:
        v, frm = stack.pop()
        i, kids = int(head[v]), 0
        while i != -1:
            if int(e[i]) != frm:
                stack.append((int(e[i]), v))
                kids += 1
            i = int(nxt[i])
        if kids == 0:
            out.append(names[v])
    return frozenset(out)


def jplace_edges(tree):
    """jplace tree string -> (plain Newick, {edge number: frozenset of leaf names below}, edge numbers in post-order,
    {edge number: branch length text})"""
    labels = [int(x) for x in re.findall(r"\{(\d+)\}", tree)]
    plain = re.sub(r"\{\d+\}", "", tree)
    kids, length, name, root = _util.parse_newick(plain)
    # post-order of the string = order in which the nodes' `:length{k}` appear
    below, order = {}, []
    stack = [(root, 0)]
    while stack:
        v, k = stack.pop()
        if k < len(kids[v]):
            stack.append((v, k + 1))
            stack.append((kids[v][k], 0))
            continue
        below[v] = frozenset([name[v]]) if not kids[v] else frozenset().union(*[below[c] for c in kids[v]])
        if v != root:
            order.append(v)
    assert len(order) == len(labels)
    texts = re.findall(r":([^,(){}:;]+)\{\d+\}", tree)
    return plain, {lab: below[v] for lab, v in zip(labels, order)}, labels, dict(zip(labels, texts))


def row_of(state, slot, frac, add):
    """(edge_num, distal_length, pendant_length) of an ABI placement"""
    s = int(slot)
    return s >> 1, (float(state["len"][s]) - float(frac)) if s & 1 else float(frac), float(add)


def finite_row(row):
    """a placement the command records: both lengths finite (a pendant length of +inf comes with a NaN position)"""
    return row is not None and math.isfinite(row[1]) and math.isfinite(row[2])


def tally(main, reps):
    """rows of one query as the command lists them: main = (edge, distal, pendant) from the uploaded alignment, reps = the
    same per replicate, in order.  Returns [(edge, count, distal, pendant)]: edges with count > 0 plus the main edge, by count
    descending, the main edge first, then edge ascending; lengths of the main placement for the main edge, else of the
    lowest-numbered replicate that chose the edge.  A placement whose lengths are not finite is not recorded: no rows at all
    (the query is left out of the file) when it is the main one, no count for this query when it is a replicate's -- the
    counts of the query then sum to less than the number of replicates."""
    if not finite_row(main):
        return []
    rows = {main[0]: [0, main[1], main[2]]}
    for edge, distal, pendant in reps:
        if not finite_row((edge, distal, pendant)):
            continue
        if edge not in rows:
            rows[edge] = [0, distal, pendant]
        rows[edge][0] += 1
    return sorted(((e, c, d, p) for e, (c, d, p) in rows.items()), key=lambda r: (-r[1], r[0] != main[0], r[0]))
