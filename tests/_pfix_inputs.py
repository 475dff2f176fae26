"""Inputs of tests/test_gpu_place_fixed_edges.py, built on the CPU from seeds: alignments whose queries are far from the backbone,
saturated (+inf under JC69), without a common site (NaN) or all three in one row, and the conditions that say a set of distance
rows is in the regime a test claims.  The conditions read the rows and the NumPy reference (tests/_pfix_ref.py) only."""
import numpy as np

from tests import _jplace, _pfix_ref, _util

SITES = 200
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
GAP = ord("-")


def as_array(seqs):
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1).copy()


def as_seqs(a):
    return [bytes(r.tobytes()) for r in a]


def p_distance(a, q, cols=slice(None)):
    """NumPy p-distances of sequence q to every row of a over the columns where both hold a base; NaN without such a column"""
    both = (a[:, cols] != GAP) & (q[None, cols] != GAP)
    diff = (a[:, cols] != q[None, cols]) & both
    with np.errstate(invalid="ignore", divide="ignore"):
        return diff.sum(axis=1) / both.sum(axis=1)


# ---- queries far from the backbone, every distance finite -------------------------------------------------------------------------
def divergent(m, c, seed, mean_bl, newick, orc, kinds=(0, 1, 2, 3)):
    """m backbone sequences and c queries, every p-distance between a query and a backbone tip below 0.75 (149 of 200 sites at
    most: JC <= 3.76, finite).  The backbone sequences evolve on a tree of their own with mean branch length `mean_bl` (the
    backbone TREE is `newick`, unrelated to it: far from additive, so the clamps fire); the tips below one edge of the backbone
    tree (about a quarter of them) share one sequence, so that a query next to them finds edges it is closer to than their
    length (a < 0).  Queries, in turn: a backbone tip with 0 .. 24 sites changed; with 40 .. 129; with 141 .. 147 (p >= ~0.70
    to everybody: JC >= ~2); a mosaic of two tips with 0 .. 59 sites changed (`kinds`: the order in which these four repeat).
    A candidate with a p of 0.75 or more is dropped."""
    rng = np.random.default_rng(seed)
    a = as_array(_util.synth_alignment(rng, max(m, 2), SITES, mean_bl=mean_bl, lo=mean_bl / 4, hi=mean_bl * 3))[:m]
    st, names = _jplace.backbone_arrays(orc, newick, m + 1)
    sizes = [(len(_jplace.leaves_below_slot(st, s, names)), s) for s in range(0, 4 * m - 4, 2)]
    _, s = min(sizes, key=lambda t: (abs(t[0] - max(m // 4, 2)), t[1]))
    below = _jplace.leaves_below_slot(st, s, names)
    same = np.array([nm in below for nm in names])
    a[same] = a[np.flatnonzero(same)[0]]
    out = []
    while len(out) < c:
        kind = kinds[len(out) % len(kinds)]
        q = a[int(rng.integers(m))].copy()
        if kind == 3:
            other, cut = a[int(rng.integers(m))], rng.random(SITES) < 0.5
            q[cut] = other[cut]
        k = int(rng.integers(0, 25) if kind == 0 else rng.integers(40, 130) if kind == 1 else rng.integers(141, 148) if kind == 2 else rng.integers(0, 60))
        pos = rng.permutation(SITES)[:k]
        q[pos] = _util.BASES[(np.searchsorted(_util.BASES, q[pos]) + rng.integers(1, 4, size=k)) & 3]
        if p_distance(a, q).max() * SITES <= 149:
            out.append(q)
    return as_seqs(a) + as_seqs(np.array(out))


def _parse(newick):
    """(children, length, leaf name) lists of a rooted binary Newick text, node 0 the root"""
    kids, length, name = [[]], [0.0], [None]
    stack, i, cur = [], 0, 0
    text = newick.strip().rstrip(";")
    assert text[0] == "("
    i = 1
    while i < len(text):
        ch = text[i]
        if ch == "(":
            kids.append([]); length.append(0.0); name.append(None)
            kids[cur].append(len(kids) - 1)
            stack.append(cur)
            cur = len(kids) - 1
            i += 1
        elif ch == ",":
            i += 1
        elif ch == ")":
            j = i + 1
            while j < len(text) and text[j] not in ",()":
                j += 1
            if text[i + 1:j].startswith(":"):
                length[cur] = float(text[i + 2:j])
            cur = stack.pop() if stack else 0
            i = j
        else:
            j = i
            while text[j] not in ",()":
                j += 1
            nm, _, ln = text[i:j].partition(":")
            kids.append([]); length.append(float(ln)); name.append(nm)
            kids[cur].append(len(kids) - 1)
            i = j
    return kids, length, name


def _change(rng, q, k):
    pos = rng.permutation(SITES)[:k]
    q[pos] = _util.BASES[(np.searchsorted(_util.BASES, q[pos]) + rng.integers(1, 4, size=k)) & 3]
    return q


def divergent_on_tree(m, c, seed, newick, factors=(0.2, 0.2, 0.2, 3.0), kinds=(4, 0, 4, 1, 4, 2, 4, 3)):
    """The p-distance counterpart of `divergent`.  p-distances are multiples of 1/200, so between unrelated sequences they scatter
    by less than an edge is long and the clamps do not fire on winning edges by chance: the input is laid out for them.  The
    backbone sequences evolve down the backbone tree ITSELF, an edge of length L changing round(f * 200 L) sites with f drawn
    per edge from `factors`: tips below edges of length 0 are copies of each other, most of the tree is closer than its lengths
    say (a < 0 next to a tip), and across an edge with f = 3 the two sides are farther apart than its length (a query on one
    side: dis1 < 0 and dis2 > L, or dis2 < 0 and dis1 > L).  Queries, in the order of `kinds`: a copy of a tip with 0 .. 3 sites
    changed (0); with 4 .. 24 (1); a mosaic of two tips (2); a tip with 146 .. 149 sites changed, p >= 0.7 to everybody (3); a
    tip moved a random number of steps towards another tip (4); 2 .. 4 with 0 .. 3 more sites changed.  Every p stays < 0.75."""
    rng = np.random.default_rng(seed)
    kids, length, name = _parse(newick)
    seq = {0: _util.BASES[rng.integers(0, 4, size=SITES)]}
    a = np.zeros((m, SITES), dtype=np.uint8)
    todo = [0]
    while todo:
        v = todo.pop()
        for w in kids[v]:
            seq[w] = _change(rng, seq[v].copy(), int(round(float(rng.choice(factors)) * SITES * length[w])))
            todo.append(w)
        if name[v] is not None:
            a[int(name[v][1:])] = seq[v]
    out = []
    while len(out) < c:
        kind = kinds[len(out) % len(kinds)]
        t = int(rng.integers(m))
        q = a[t].copy()
        other = a[int(rng.integers(m))]
        if kind == 2:
            cut = rng.random(SITES) < 0.5
            q[cut] = other[cut]
        elif kind == 4:
            differ = rng.permutation(np.flatnonzero(q != other))
            step = differ[:int(rng.integers(0, len(differ) + 1))]
            q[step] = other[step]
        k = int(rng.integers(4, 25) if kind == 1 else rng.integers(146, 150) if kind == 3 else rng.integers(0, 4))
        q = _change(rng, q, k)
        if p_distance(a, q).max() * SITES <= 149:
            out.append(q)
    return as_seqs(a) + as_seqs(np.array(out))


def divergent_backbone(m, seed, long_edges):
    return _jplace.random_backbone(np.random.default_rng(seed), m, "random", zero_frac=0.2, max_len=1.0 if long_edges else 0.05)


def divergent_conditions(p, rows, dist_type, not_on_winners=()):
    """finite rows; every clamp branch on some eligible and on some winning edge (but for those of `not_on_winners`, which the
    caller has to justify); a winning edge of length 0; JC: at least 10 queries whose winning pendant length is >= 2 (p-distances
    are <= 1, so add <= 1 by the arithmetic: not asked of type 1)"""
    assert np.all(np.isfinite(rows)) and rows.max() >= (2.9 if dist_type == 2 else 0.73), rows.max()
    for b in _pfix_ref.BRANCHES:
        assert p.any_took[b].any(), b
        assert b in not_on_winners or p.win_took[b].any(), ("winning edge", b)
    assert np.any(p.len[p.win] == 0.0)
    if dist_type == 2:
        assert np.count_nonzero(p.win_add >= 2.0) >= 10, np.count_nonzero(p.win_add >= 2.0)
    else:
        assert rows.max() <= 1.0 and p.win_add.max() <= 1.0


# ---- saturated and empty pairs ---------------------------------------------------------------------------------------------------
INV = 50          # columns [0, INV) hold one letter of A, C, G each, the same in every sequence


class Engineered:
    """seqs: m backbone sequences then c queries; at[name] = query index of an engineered query; clade1: bool (m,)"""


def engineered(m, c, seed, newick, orc, gapped=False, positions=None, mean_bl=6e-3, near_tips=False):
    """An alignment of m + c sequences evolved on one tree, then restricted: columns [0, 50) are invariant over the whole alignment
    (a letter of A, C, G per column); in columns [50, 200) the tips of clade 1 (the leaves below one edge of the backbone, between
    a quarter and three quarters of them) hold A or C only (G -> A, T -> C), everything else A, C or G (T -> G).  On top of it:
      inf     the invariant letters, then T: p = 150/200 exactly against every backbone tip (JC: +inf)
      nan     the invariant letters in [0, 40), then T: p = 160/200 (JC: NaN)
      gaps    all gaps: no common site with anybody (NaN through useful == 0)
      clade   the invariant letters, then G: p = 150/200 against clade 1 (+inf), finite against the rest (who hold G in
              about half of those columns)
      half    (gapped = True: the backbone tips with an odd index carry gaps in [0, 100)) a query with gaps in [100, 200): no
              common site with the odd tips (NaN), finite against the even ones
      tip2, tiplast   copies of backbone tip 2 and of tip m - 1
    positions: {name: query index}; the other queries are ordinary ones: tips of the tree the alignment evolved on, or, with
    near_tips, query j a copy of backbone tip j m / c with three sites changed (winners spread over the whole backbone)."""
    rng = np.random.default_rng(seed)
    a = as_array(_util.synth_alignment(rng, m + c, SITES, mean_bl=mean_bl, lo=1e-3, hi=2e-2))
    inv = _util.BASES[rng.integers(0, 3, size=INV)]
    a[:, :INV] = inv[None, :]
    st, names = _jplace.backbone_arrays(orc, newick, m + 1)
    lim = 4 * m - 4
    sizes = [(len(_jplace.leaves_below_slot(st, s, names)), s) for s in range(0, lim, 2)] if m <= 400 else None
    if sizes is not None:
        size, s = min(sizes, key=lambda t: (abs(t[0] - m // 2), t[1]))
        assert m // 4 <= size <= 3 * m // 4 or m < 8, size
        below = _jplace.leaves_below_slot(st, s, names)
        clade1 = np.array([nm in below for nm in names])
    else:
        clade1 = np.arange(m) < m // 2                                        # (large backbones: the first half of the tips)
    body = a[:, INV:]
    body[body == ord("T")] = ord("G")
    one = body[:m][clade1]
    one[one == ord("G")] = ord("A")
    body[:m][clade1] = one
    if near_tips:
        for j in range(c):
            a[m + j] = a[j * m // c]
            pos = INV + rng.permutation(SITES - INV)[:3]
            a[m + j, pos] = _util.BASES[(np.searchsorted(_util.BASES, a[m + j, pos]) + rng.integers(1, 3, size=3)) % 3]
    if gapped:
        a[1:m:2, :100] = GAP
    made = {
        "inf": np.concatenate([inv, np.full(SITES - INV, ord("T"), np.uint8)]),
        "nan": np.concatenate([inv[:40], np.full(SITES - 40, ord("T"), np.uint8)]),
        "gaps": np.full(SITES, GAP, np.uint8),
        "clade": np.concatenate([inv, np.full(SITES - INV, ord("G"), np.uint8)]),
        "tip2": a[2].copy(),
        "tiplast": a[m - 1].copy(),
    }
    half = a[m + c // 2].copy()
    half[100:] = GAP
    made["half"] = half
    out = Engineered()
    out.at = dict(positions or {})
    for name, q in out.at.items():
        a[m + q] = made[name]
    out.m, out.c, out.seqs, out.clade1, out.array = m, c, as_seqs(a), clade1, a
    return out


def engineered_conditions(inp, p, rows):
    """each engineered row is what it is meant to be -- NumPy p-distances of the sequences, np.isinf / np.isnan of the rows -- and
    the reference gives what the definition says for it"""
    a, m = inp.array, inp.m
    bb = a[:m]
    gapped = bool((bb[:, :100] == GAP).any())
    odd = (np.arange(m) & 1) == 1
    lowest = p.slots[0]
    for name, q in inp.at.items():
        pd, row = p_distance(bb, a[m + q]), rows[q]
        if name == "inf" and not gapped:
            assert np.all(pd == 0.75) and np.all(np.isinf(row)) and np.all(row > 0)
            assert np.all(np.isinf(p.add[q])) and p.slot[q] == lowest and np.isnan(p.win_frac[q])
        elif name == "inf":
            assert np.all(pd[~odd] == 0.75) and np.all(pd[odd] == 1.0)
            assert np.all(np.isinf(row[~odd])) and np.all(np.isnan(row[odd]))
        elif name == "nan" and not gapped:
            assert np.all(pd == 0.8) and np.all(np.isnan(row))
        elif name in ("nan", "gaps"):
            assert (np.all(np.isnan(pd)) if name == "gaps" else np.all(pd >= 0.8)) and np.all(np.isnan(row))
        elif name == "clade":
            far = inp.clade1 & ~(odd & gapped)
            assert np.all(pd[far] == 0.75) and np.all(np.isinf(row[far]))
            assert np.all(pd[~inp.clade1] < 0.7) and np.all(np.isfinite(row[~inp.clade1 & ~(odd & gapped)]))
            assert far.any() and (~inp.clade1).any()
        elif name == "half":
            assert gapped and np.all(np.isnan(pd[odd])) and np.all(np.isnan(row[odd]))
            assert np.all(pd[~odd] < 0.7) and np.all(np.isfinite(row[~odd]))
        elif name in ("tip2", "tiplast"):
            t = 2 if name == "tip2" else m - 1
            assert row[t] == 0.0 or (gapped and t & 1)
        if name in ("nan", "gaps"):                                              # NaN to everybody: add = 0 on every edge, the lowest slot, the middle
            assert np.all(p.add[q] == 0.0) and p.slot[q] == lowest and p.win_frac[q] == p.len[0] / 2
    ordinary = np.ones(len(rows), dtype=bool)
    ordinary[[q for q in inp.at.values()]] = False
    assert np.all(np.isfinite(rows[ordinary][:, ~(odd & gapped)]))


def chunk_conditions(p, m):
    """every reduce wavefront has work in several rounds, and the winners are spread: at least 100 distinct winning slots, some in
    the first and some in the last tenth of [0, 4m - 4)"""
    lim = 4 * m - 4
    won = np.unique(p.slot)
    assert len(won) >= 100, len(won)
    assert won[0] < lim // 10 and won[-1] >= lim - lim // 10, (won[0], won[-1], lim)
    return len(won)
