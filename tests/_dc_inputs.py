"""Inputs of tests/test_gpu_dc_edges.py, built on the CPU from seeds, and the conditions that say an input is in the regime a test
claims.  The conditions read the oracle only (orc.dc_run, orc.dc_run(..., backbone_only=True)) on a distance matrix: the oracle's own
distances in tests/test_dc_inputs.py, the GPU's in tests/test_gpu_dc_edges.py.

The central tool is trimming by the oracle's own assignment.  The backbone is frozen while the queries are assigned and distances are
pairwise, so the cluster of a query does not depend on which other queries are present: build a superset, take the oracle's cluster_id
on it, keep exactly the wanted number of queries per cluster, run on the subset.  A builder returns a Case: the superset's sequences,
the backbone size, the flag for the reference's unwritten last-tip distance, and trim(cluster_id) -> the kept tips in ascending order."""
import numpy as np

from tests import _util

GAP = ord("-")


class Case:
    """seqs (superset: backbone tips first), B, L (alignments), skip_last (what orc.dc_run takes; the library's flags are
    DC_EXACT_LAST where it is 0), trim(cluster_id) -> kept tip indices, and what the builder's condition needs"""

    def flags(self):
        from dipper_amd import capi
        return 0 if self.skip_last else capi.DC_EXACT_LAST


def as_array(seqs):
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1).copy()


def as_seqs(a):
    return [bytes(r.tobytes()) for r in a]


def clone(rng, s, lo=1, hi=12):
    """a copy of sequence s (uint8 array) with `lo` .. `hi - 1` sites drawn and set to a random base"""
    t = s.copy()
    pos = rng.integers(0, len(t), size=int(rng.integers(lo, hi)))
    t[pos] = _util.BASES[rng.integers(0, 4, size=len(pos))]
    return t


def assignment(orc, M, B, skip_last):
    """the oracle's cluster_id on a matrix: backbone tree and assignment only"""
    return orc.dc_run(M, B, skip_last_backbone=skip_last, backbone_only=True)["cluster_id"]


def submatrix(M, keep):
    return np.ascontiguousarray(M[np.ix_(keep, keep)])


def sizes_of(cluster_id, B):
    """sorted member counts of the clusters"""
    return sorted(np.unique(cluster_id[B:], return_counts=True)[1].tolist())


def cap_per_cluster(cluster_id, B, cap, queries=None):
    """the backbone and, in tip order, the queries (all, or those given) as long as their cluster holds fewer than `cap` kept ones"""
    held, keep = {}, list(range(B))
    for t in (range(B, len(cluster_id)) if queries is None else queries):
        c = int(cluster_id[t])
        if held.get(c, 0) < cap:
            held[c] = held.get(c, 0) + 1
            keep.append(int(t))
    return np.array(sorted(keep))


def placed_everything(ref, n):
    assert ref["next_slot"] == 4 * n - 4, ref["next_slot"]


# ---- cluster sizes at the seams ---------------------------------------------------------------------------------------------------
SIZES = [1, 2, 31, 32, 33, 54, 55, 63, 64, 65, 129]
# 64 | 65: dc_cluster_kernel<1> | <16>;  32 | 33 and 64 | 65: one | two row tiles of the 32- and the 64-tile job list;  54 | 55: the
# 10 + m columns of a cluster end at 64 | 65;  1 and 2: no earlier member, one;  odd and even m: ld = (10 + m + 1) & ~1;  129: three
# row tiles of 64, five of 32


def size_families(seed=7, over=20):
    """Backbone of 200 tips, 1 200 sites; one clone family per backbone tip 3, 10, 17, ... (a clone: 1 to 11 sites redrawn), each
    generated `over` above its size of SIZES, in a shuffled order, and trimmed to that size: n = 200 + 529 = 729 after trimming."""
    rng = np.random.default_rng(seed)
    B, L = 200, 1200
    a = as_array(_util.synth_alignment(rng, B, L, mean_bl=5e-3, lo=1e-4, hi=5e-2))
    fam = np.repeat(np.arange(len(SIZES)), [s + over for s in SIZES])
    fam = fam[rng.permutation(len(fam))]
    q = np.array([clone(rng, a[3 + 7 * f]) for f in fam])
    c = Case()
    c.seqs, c.B, c.L, c.skip_last, c.fam = as_seqs(a) + as_seqs(q), B, L, 1, fam

    def trim(cluster_id):
        keep, used = list(range(B)), set()
        for f, size in enumerate(SIZES):
            tips = B + np.flatnonzero(fam == f)
            ids, cnt = np.unique(cluster_id[tips], return_counts=True)
            main = int(ids[np.argmax(cnt)])
            assert main not in used and cnt.max() >= size, ("family", f, "clusters", ids, cnt)
            used.add(main)
            keep += [int(t) for t in tips[cluster_id[tips] == main][:size]]
        return np.array(sorted(keep))
    c.trim = trim
    return c


def size_conditions(ref, B):
    """the oracle's sorted cluster sizes are exactly SIZES, every tip is placed and every pendant length is < 2"""
    n = len(ref["cluster_id"])
    placed_everything(ref, n)
    assert sizes_of(ref["cluster_id"], B) == SIZES, sizes_of(ref["cluster_id"], B)
    assert np.all(ref["trace"][2:, 2] < 2.0), ref["trace"][2:, 2].max()


# ---- gaps and ambiguity codes -------------------------------------------------------------------------------------------------------
def gapped(L, seed=0):
    """460 tips evolved on one tree, the first 100 the backbone, 3 % of every sequence's sites a gap, an N or a lower-case letter,
    plus 40 clones of backbone tip 5 (its gaps included): 500 tips.  The oracle's `useful` counts the sites where at least ONE side
    holds a base, so scattered gaps alone leave it within a site or two of L: deletions are shared.  Tip 5 has a run of 40 gaps,
    which two of three clones keep (pairs within the family: useful <= L - 40; against the third clone: the band table); 6 backbone
    tips and 30 queries share a run of 20 more.  L = 500 stays within one 16-word stage, 1 000 uses the full (useful, match)
    table, 1 100 the band table.  Run with the last-tip distance computed: with the reference's unwritten one this input puts
    most queries into one cluster (295 of 400 at 3 % invalid sites, 72 at none) and the oracle ends in -2.  Trimmed so that every
    cluster stays below the backbone size."""
    rng = np.random.default_rng(1000 + L + seed)
    B = 100
    a = as_array(_util.synth_alignment(rng, 460, L, mean_bl=5e-3, lo=1e-4, hi=5e-2, invalid_frac=0.03))
    run = slice(L // 3, L // 3 + 40)
    filled = a[5, run].copy()
    a[5, run] = GAP
    q = np.array([clone(rng, a[5]) for _ in range(40)])
    q[2::3, run] = filled
    shared = np.concatenate([rng.permutation(B)[:6], B + rng.permutation(360)[:30]])
    a[shared, L // 2:L // 2 + 20] = GAP
    c = Case()
    c.seqs, c.B, c.L, c.skip_last = as_seqs(a) + as_seqs(q), B, L, 0
    c.trim = lambda cluster_id: cap_per_cluster(cluster_id, B, B - 1)
    return c


def gapped_conditions(orc, seqs, L, ref, B):
    """seqs: the kept sequences, the clones of tip 5 last.  Among the backbone and the last 30 sequences some pair shares every
    site (useful == L), some pair is within the band table (L - 15 <= useful < L) and some beyond it (useful < L - 15), the last
    also between two queries of one cluster; all placed, every cluster below the backbone size"""
    n = len(seqs)
    placed_everything(ref, n)
    assert max(sizes_of(ref["cluster_id"], B)) < B
    pick = list(range(B)) + list(range(n - 30, n))
    useful, _ = orc.msa_counts(orc.pack4_many([seqs[t] for t in pick]), L)
    r, c = np.tril_indices(len(pick), -1)
    off = useful[r, c]
    assert np.any(off == L) and np.any((off >= L - 15) & (off < L)) and np.any(off < L - 15), (off.min(), off.max(), L)
    cl = ref["cluster_id"][pick]
    assert np.any((off < L - 15) & (cl[r] == cl[c]) & (c >= B)), "no in-cluster pair beyond the band table"


# ---- exact ties --------------------------------------------------------------------------------------------------------------------
def duplicates(seed=0):
    """Backbone of 120 tips, 800 sites; 80 ordinary queries; 70 exact copies of backbone tip 17 and 33 of tip 40, shuffled among
    each other.  Ordinary queries that share a cluster with the copies are trimmed away."""
    rng = np.random.default_rng(2000 + seed)
    B, L = 120, 800
    a = as_array(_util.synth_alignment(rng, B + 80, L, mean_bl=5e-3, lo=1e-4, hi=5e-2))
    of = np.array([17] * 70 + [40] * 33)[rng.permutation(103)]
    c = Case()
    c.seqs, c.B, c.L, c.skip_last, c.copy_of = as_seqs(a) + as_seqs(a[of]), B, L, 1, of
    first = B + 80

    def trim(cluster_id):
        theirs = set(cluster_id[first:].tolist())
        return np.array([t for t in range(len(cluster_id)) if t < B or t >= first or int(cluster_id[t]) not in theirs])
    c.trim = trim
    return c


def duplicate_conditions(M, ref, B):
    """the copies are the last 103 tips: the 70 and the 33 each form one cluster of exactly that size, at least 100 of them are
    placed with a pendant length of exactly 0, and the matrix holds at least 1 000 zeros below its diagonal"""
    n = len(ref["cluster_id"])
    placed_everything(ref, n)
    ids, cnt = np.unique(ref["cluster_id"][n - 103:], return_counts=True)
    assert sorted(cnt.tolist()) == [33, 70], (ids, cnt)
    for i, k in zip(ids, cnt):
        assert np.count_nonzero(ref["cluster_id"] == i) == k
    assert np.count_nonzero(ref["trace"][n - 103:, 2] == 0.0) >= 100
    assert np.count_nonzero(M[np.tril_indices(n, -1)] == 0.0) >= 1000


# ---- tiny backbones, and the chunk that closes at 64 entries ---------------------------------------------------------------------------
def tiny_backbone(B, skip_last, seed=0, far=None):
    """Backbone of 3, 4 or 5 tips (closest lists with -1 entries), 600 sites; 60 queries, every other one a clone of a backbone tip
    (20 to 59 sites redrawn), trimmed to at most B - 1 per cluster.  far: that backbone tip is an unrelated random sequence, at
    NaN, +inf or a distance >= 2 from every query (far_conditions())."""
    rng = np.random.default_rng(3000 + 10 * B + seed)
    L = 600
    a = as_array(_util.synth_alignment(rng, B + 30, L, mean_bl=2e-2, lo=2e-3, hi=8e-2))
    if far is not None:
        a[far] = _util.BASES[rng.integers(0, 4, size=L)]
    q = np.array([clone(rng, a[int(rng.integers(B))], 20, 60) for _ in range(30)])
    mixed = np.empty((60, L), dtype=np.uint8)
    mixed[0::2], mixed[1::2] = a[B:], q
    c = Case()
    c.seqs, c.B, c.L, c.skip_last = as_seqs(a[:B]) + as_seqs(mixed), B, L, skip_last
    c.trim = lambda cluster_id: cap_per_cluster(cluster_id, B, B - 1)
    return c


def tiny_conditions(bb, ref, B, skip_last):
    """bb: the oracle's backbone_only state.  Closest lists of the backbone hold -1 entries; one cluster is full (B - 1 members),
    and there are several (not asked with the reference's unwritten last-tip distance: a 0.0 to tip B - 1 of three to five pulls
    every query onto that tip's edge); all placed below 2"""
    n = len(ref["cluster_id"])
    placed_everything(ref, n)
    absent = int(np.count_nonzero(bb["cid"][:5 * (4 * B - 4)] == -1))
    assert absent > 0
    sz = sizes_of(ref["cluster_id"], B)
    assert sz[-1] == B - 1 and (len(sz) >= 2 or skip_last), sz
    assert np.all(ref["trace"][B:, 2] < 2.0)
    return absent


TINY_FAR = [(5, 2), (5, 3)]            # (backbone tips, the far one): inputs of far_conditions with the oracle's distances


def far_conditions(M, bb, ref, B):
    """Every tip is placed below 2, and some query is at +inf or beyond 2.1 from the backbone tip whose distance row comes first in
    the scan chunk (table_stats): distances above the path length 2.0 that an empty list entry holds, on a backbone where every
    side of every edge has such entries.  (No assignment depends on it here -- every edge shifts alike; FAR40 has those.)"""
    n = len(ref["cluster_id"])
    placed_everything(ref, n)
    assert np.all(ref["trace"][B:, 2] < 2.0)
    d = M[B:, table_stats(bb, B)["first_leaf"]]
    hits = int(np.count_nonzero(~np.isnan(d) & (d > 2.1)))
    assert hits >= 1
    return hits


def backbone40(nq, seed=0, far=None):
    """Backbone of 40 tips: 78 table entries whose lists name at most 40 distinct tips, so the first chunk closes because it holds
    64 entries, and a second one of 14 follows.  nq = 1, 64, 65 queries: a lone query, a full group of 64, one more.
    far: that backbone tip is an unrelated random sequence, at NaN, +inf or a distance >= 2 from every query (FAR40)."""
    rng = np.random.default_rng(4000 + seed)
    B, L = 40, 600
    c = Case()
    c.seqs, c.B, c.L, c.skip_last = _util.synth_alignment(rng, B + 200, L, mean_bl=5e-3, lo=1e-4, hi=5e-2), B, L, 1
    if far is not None:
        c.seqs[far] = _util.BASES[np.random.default_rng(far).integers(0, 4, size=L)].tobytes()

    def trim(cluster_id):
        keep = cap_per_cluster(cluster_id, B, B - 1)
        assert len(keep) >= B + nq
        return keep[:B + nq]
    c.trim = trim
    return c


# ---- saturated and empty pairs ---------------------------------------------------------------------------------------------------------
def saturated(L, seed, variant="plain", redrawn=1.0):
    """300 tips, backbone 80, the last-tip distance computed.  Three to five queries have a share `redrawn` of their sites drawn
    anew: at 1.0 they are unrelated random sequences, whose JC distances are a mix of NaN, +inf and finite values at or above 2;
    at 0.85 to 0.9 they stay just below 2 from their nearest backbone tips.  Every variant but "plain" has one more query that is
    all gaps (NaN to everybody: add = 0 on every edge of every chunk and of its cluster); "backboneN": backbone tip 7 is all N
    (a NaN column); "backboneX": backbone tip 7 is an unrelated random sequence (a column of NaN, +inf and values >= 2 for
    every query, and a backbone tip that the backbone tree itself places with the default tuple).
    Two regimes, told apart from the oracle's result alone (regime())."""
    rng = np.random.default_rng(5000 + L + 17 * seed)
    n, B = 300, 80
    a = as_array(_util.synth_alignment(rng, n, L, mean_bl=5e-3, lo=1e-4, hi=5e-2))
    alien = B + rng.permutation(n - B)[:int(rng.integers(3, 6))]
    for t in alien:
        hit = rng.random(L) < redrawn
        a[t, hit] = _util.BASES[rng.integers(0, 4, size=int(hit.sum()))]
    c = Case()
    c.alien, c.empty = np.sort(alien), []
    if variant != "plain":
        t = int(np.setdiff1d(np.arange(B, n), alien)[int(rng.integers(n - B - len(alien)))])
        a[t] = GAP
        c.empty.append(t)
    if variant == "backboneN":
        a[7] = ord("N")
    if variant == "backboneX":
        a[7] = _util.BASES[rng.integers(0, 4, size=L)]
    c.seqs, c.B, c.L, c.skip_last = as_seqs(a), B, L, 0
    c.trim = lambda cluster_id: cap_per_cluster(cluster_id, B, B - 1)
    return c


def regime(M, ref, B):
    """"placeable": every member's final pendant length is < 2, and at least one query has NaN to every backbone tip.
    "no candidate": some member ends with a final pendant length of exactly 2, the default tuple, and none above it -- the oracle
    then splits slot 0 as the reference would, which the library refuses.  Anything else (the oracle gave up, or a pendant length
    above 2) is no input of these tests: None.

    A member that was assigned to slot 0 and is still placed below 2 exists in the second regime only, and never as the first
    member of its cluster: a query gets cluster 0 when no eligible backbone edge gives a pendant length below 2, the edge behind
    slot 0 (scanned through its reverse, which is eligible) among them; the first member of cluster 0 meets exactly that edge with
    exactly those lists and distances again, so it ends with the default tuple.  Later members of cluster 0 may land below 2 on
    the edges that the oracle made by splitting slot 0."""
    n = len(ref["cluster_id"])
    if ref["next_slot"] != 4 * n - 4:
        return None
    add = ref["trace"][B:, 2]
    if np.any(add == 2.0) and np.all(add <= 2.0):
        first = {}
        for t in range(B, n):
            first.setdefault(int(ref["cluster_id"][t]), t)
        assert 0 in first and add[first[0] - B] == 2.0
        return "no candidate"
    if np.all(add < 2.0) and np.any(np.all(np.isnan(M[B:, :B]), axis=1)):
        assert not np.any(ref["cluster_id"][B:] == 0)
        return "placeable"
    return None


# (L, seed, variant, redrawn): with the oracle's own distances the first, second and last are "no candidate", the others "placeable"
# (the third and fourth with unrelated random queries)
SATURATED = [(200, 0, "plain", 1.0), (600, 1, "backboneN", 1.0), (200, 2, "backboneN", 1.0), (200, 5, "backboneN", 1.0),
             (200, 0, "backboneX", 0.85), (600, 1, "backboneX", 0.85), (200, 2, "backboneX", 0.9)]


def saturated_conditions(M, B):
    """the matrix holds NaN, +inf and finite values >= 2 between queries and backbone"""
    rows = M[B:, :B]
    assert np.isnan(rows).any() and np.isposinf(rows).any() and np.any(np.isfinite(rows) & (rows >= 2.0))


# ---- reads -------------------------------------------------------------------------------------------------------------------------
def _read_clone(rng, r):
    t = np.frombuffer(r, dtype=np.uint8).copy()
    pos = rng.integers(0, len(t), size=int(rng.integers(1, 4)))
    t[pos] = _util.BASES[rng.integers(0, 4, size=len(pos))]
    return t.tobytes()


def mash_families(case, seed=0, over=20):
    """Reads of 600 to 1 000 bases (k = 15, S = 1 000: most sketches are shorter than S).  The backbone reads evolve on a tree, with
    indels.  Case 1: backbone 150, clone families (1 to 3 bases redrawn) of backbone reads 3, 10, 17, 24 trimmed to 8, 9, 64 and 65
    members -- one | two row groups of kLRows = 8, dc_cluster_kernel<1> | <16>.  Case 2: backbone 520, one family of read 3 trimmed
    to 503 members: 513 columns, of which member t reads the first 10 + t, so the last row group ends at column 511, the last of the
    first column job.  Case 3: the same with 504 members: member 503 reads column 512, the second column job (jobs_expected())."""
    rng = np.random.default_rng(6000 + 100 * min(case, 2) + seed)                # (cases 2 and 3: the same backbone)
    B, sizes = (150, [8, 9, 64, 65]) if case == 1 else (520, [503 if case == 2 else 504])
    base = _util.synth_reads(rng, B, 1000, mean_bl=2e-2, lo=2e-3, hi=8e-2)
    reads = []
    for r in base:
        ln = int(rng.integers(600, 1001))
        reads.append(r[:ln] if len(r) >= ln else r)
    fam = np.repeat(np.arange(len(sizes)), [s + over for s in sizes])
    fam = fam[rng.permutation(len(fam))]
    c = Case()
    c.seqs, c.B, c.L, c.skip_last, c.sizes = reads + [_read_clone(rng, reads[3 + 7 * f]) for f in fam], B, None, 0, sizes

    def trim(cluster_id):
        keep, used = list(range(B)), set()
        for f, size in enumerate(sizes):
            tips = B + np.flatnonzero(fam == f)
            ids, cnt = np.unique(cluster_id[tips], return_counts=True)
            main = int(ids[np.argmax(cnt)])
            assert main not in used and cnt.max() >= size, ("family", f, "clusters", ids, cnt)
            used.add(main)
            keep += [int(t) for t in tips[cluster_id[tips] == main][:size]]
        return np.array(sorted(keep))
    c.trim = trim
    return c


def jobs_expected(sizes, rows=8, cols=512):
    """pair jobs of the Mash front-end: per group of `rows` members one job per `cols` columns up to the last member's 10 + t"""
    return sum(-(-(10 + min(m, t0 + rows) - 1) // cols) for m in sizes for t0 in range(0, m, rows))


def mash_conditions(ref, B, sizes):
    placed_everything(ref, len(ref["cluster_id"]))
    assert sizes_of(ref["cluster_id"], B) == sorted(sizes), sizes_of(ref["cluster_id"], B)


# ---- the assignment table, restated from the oracle's backbone -----------------------------------------------------------------------
MAX_ENTRIES, MAX_LEAVES = 64, 48       # a scan chunk: table entries, distinct backbone tips named by their closest lists


def table_stats(bb, B):
    """What dpr_get_dc_table_stats reports for a backbone, from the oracle's backbone_only state: the eligible slot of every edge in
    depth-first order from the root-side node (a stack, children in adjacency-list order), cut into chunks that close before the
    entry that would bring them above MAX_LEAVES distinct tips or MAX_ENTRIES entries.
    Returns entries, chunks, most entries in a chunk, most distinct tips in a chunk."""
    head, e, nxt, belong, cid = bb["head"], bb["e"], bb["nxt"], bb["belong"], bb["cid"]
    n = len(bb["cluster_id"])
    order, stack = [], [(n, -1)]
    while stack:
        node, via = stack.pop()
        i = int(head[node])
        while i != -1:
            if not (via >= 0 and e[i] == belong[via]):
                to = int(e[i])
                r = int(head[to])
                while e[r] != node:
                    r = int(nxt[r])
                order.append(i if belong[i] >= e[i] else r)
                stack.append((to, i))
            i = int(nxt[i])
    assert len(order) == 2 * B - 2
    chunks, cur, held, firsts = [], set(), 0, []
    for s in order:
        rev = int(head[e[s]])
        while e[rev] != belong[s]:
            rev = int(nxt[rev])
        named = [int(t) for t in np.concatenate([cid[5 * s:5 * s + 5], cid[5 * rev:5 * rev + 5]]) if t >= 0]
        if len(cur | set(named)) > MAX_LEAVES or held >= MAX_ENTRIES:
            chunks.append((held, len(cur)))
            cur, held = set(), 0
        if held == 0:
            firsts.append(named[0])
        cur |= set(named)
        held += 1
    chunks.append((held, len(cur)))
    return dict(entries=len(order), chunks=len(chunks), max_entries=max(c[0] for c in chunks), max_leaves=max(c[1] for c in chunks),
                first_leaf=firsts[0], first_leaves=firsts, order=order, chunk_entries=[c[0] for c in chunks])


FAR40 = [27, 32]       # far tips of backbone40 that come out as the first row of a scan chunk, and for which absent_entry_flips() > 0


def absent_entry_flips(bb, B, M, skip_last):
    """How many queries would be assigned to another cluster if an absent (-1) closest-list entry, which holds the path length 2.0,
    read the first distance row of its scan chunk instead of a row of -inf: its candidate is then distance - 2.0, which exceeds
    the running maximum (it starts at 0) only for a distance above 2 -- on every other input the two are the same function.
    The assignment scan restated from the oracle's backbone_only state, once as it is (checked against bb's cluster_id) and once
    with that change."""
    ts = table_stats(bb, B)
    head, e, nxt, belong, cid, cdis, length = bb["head"], bb["e"], bb["nxt"], bb["belong"], bb["cid"], bb["cdis"], bb["len"]
    n = len(bb["cluster_id"])
    D = np.array(M, dtype=np.float64)
    if skip_last:
        D[:, B - 1] = 0.0
    first_row, k = {}, 0
    for c, held in enumerate(ts["chunk_entries"]):
        for s in ts["order"][k:k + held]:
            first_row[int(s)] = ts["first_leaves"][c]
        k += held

    def scan(changed):
        out = []
        for q in range(B, n):
            best, slot = 2.0, 0
            for s in sorted(first_row):
                rev = int(head[e[s]])
                while e[rev] != belong[s]:
                    rev = int(nxt[rev])
                dis = []
                for side in (s, rev):
                    d = 0.0
                    for i in range(5):
                        t = int(cid[5 * side + i])
                        if t < 0 and not changed:
                            continue
                        v = D[q, t if t >= 0 else first_row[s]] - cdis[5 * side + i]
                        if v > d:
                            d = v
                    dis.append(d)
                d1, d2 = dis
                L = length[s]
                with np.errstate(invalid="ignore"):
                    a = (d1 + d2 - L) / 2
                    if a < 0:
                        a = 0.0
                    d1, d2 = d1 - a, d2 - a                                  # (their clamp at 0 does not enter a: L >= 0)
                    if d1 > L:
                        a += d1 - L
                    if d2 > L:
                        a += d2 - L
                if a < best:
                    best, slot = a, s
            out.append(slot)
        return np.array(out)
    as_is = scan(False)
    assert np.array_equal(as_is, bb["cluster_id"][B:])
    return int(np.count_nonzero(scan(True) != as_is))
