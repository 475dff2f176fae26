"""The definition of the placement on a fixed backbone in NumPy float64, independent of orc_place_run: there is
no (slot 0, add 2) default tuple here, so distances of any size, +inf and NaN are in its domain.

Input: the importer's state after place_init_lists (head, e, nxt, belong, len, cid, cdis), the number of backbone tips m, and a
(Q, m) block of distances.  Per eligible slot s (belong[s] >= e[s], s < 4m - 4) the two maxima over the closest list of s and of
the opposite slot start at +0 and take a candidate only where `val > dis` (a NaN candidate and an absent entry, cid == -1, are
passed over); then the clamp sequence of orc_edge_scan (oracle/dipper_oracle.c, `double L = ...` to `d1 = dis1`) in its order.
Every operation is an IEEE add, subtract, halving or compare of the oracle's operands in the oracle's order -- no multiply,
nothing to contract -- so a comparison with this reference needs no tolerance: bit for bit, NaN equal to NaN of any payload.

scan_scalar is the same loop for one (row, slot), a line-by-line transcription in Python floats that test_pfix_ref.py holds
against the vectorised tables."""
import numpy as np

BRANCHES = ("a<0", "dis1<0", "dis2<0", "dis1>L", "dis2>L")


def eligible_slots(st, m):
    lim = 4 * m - 4
    return np.flatnonzero(st["belong"][:lim] >= st["e"][:lim])


def opposite_slots(st, slots):
    """for every slot s the slot of the same edge seen from the other end: walk head[e[s]] until e[oe] == belong[s]"""
    head, e, nxt, belong = st["head"], st["e"], st["nxt"], st["belong"]
    out = np.empty(len(slots), dtype=np.int64)
    for k, s in enumerate(slots):
        x, oe = int(belong[s]), int(head[e[s]])
        while int(e[oe]) != x:
            oe = int(nxt[oe])
        out[k] = oe
    return out


def _list_max(st, slots, rows):
    cid, cdis = st["cid"], st["cdis"]
    dis = np.zeros((rows.shape[0], len(slots)))                                  # +0
    for i in range(5):
        ids = cid[slots * 5 + i]
        present = ids != -1
        with np.errstate(invalid="ignore"):
            val = rows[:, np.where(present, ids, 0)] - cdis[slots * 5 + i][None, :]
            dis = np.where(present[None, :] & (val > dis), val, dis)             # NaN > dis is False: passed over
    return dis


class Placement:
    """slots (E,): the eligible slots ascending; add, frac (Q, E): the tables; slot, win_add, win_frac (Q,): the winner by
    smallest (add, slot); took[b] (Q, E) bool: edges on which clamp branch b fired; win_took[b], any_took[b] (Q,)"""


def place(st, m, rows):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[1] == m
    slots = eligible_slots(st, m)
    assert len(slots) == 2 * m - 2
    dis1 = _list_max(st, slots, rows)
    dis2 = _list_max(st, opposite_slots(st, slots), rows)
    L = st["len"][slots][None, :]
    assert np.all(np.isfinite(L))
    took = {}
    with np.errstate(invalid="ignore"):                                          # inf - inf
        a = (dis1 + dis2 - L) / 2
        took["a<0"] = a < 0
        a = np.where(took["a<0"], 0.0, a)
        dis1 = dis1 - a
        dis2 = dis2 - a
        took["dis1<0"] = dis1 < 0
        dis1 = np.where(took["dis1<0"], 0.0, dis1)
        took["dis2<0"] = dis2 < 0
        dis2 = np.where(took["dis2<0"], 0.0, dis2)
        took["dis1>L"] = dis1 > L
        a = np.where(took["dis1>L"], a + (dis1 - L), a)
        dis1 = np.where(took["dis1>L"], L, dis1)
        took["dis2>L"] = dis2 > L
        a = np.where(took["dis2>L"], a + (dis2 - L), a)
        dis2 = np.where(took["dis2>L"], L, dis2)
        rest = L - dis1 - dis2
        frac = dis1 + rest / 2
    assert not np.isnan(a).any()                                                 # L and cdis are finite: the maxima are never NaN
    p = Placement()
    p.slots, p.add, p.frac, p.took, p.len = slots, a, frac, took, st["len"][slots]
    if rows.shape[0]:
        w = np.argmin(a, axis=1)                                                 # the first minimum: slots ascend
    else:
        w = np.zeros(0, dtype=np.int64)
    q = np.arange(rows.shape[0])
    p.win = w
    p.slot = slots[w].astype(np.int32)
    p.win_add, p.win_frac = a[q, w], frac[q, w]
    p.win_took = {b: t[q, w] for b, t in took.items()}
    p.any_took = {b: t.any(axis=1) for b, t in took.items()}
    return p


def scan_scalar(st, row, s):
    """(frac, add) of slot s for one distance row: orc_edge_scan's eligible branch, statement by statement"""
    head, e, nxt, belong, ln, cid, cdis = (st[k] for k in ("head", "e", "nxt", "belong", "len", "cid", "cdis"))
    x, oth = int(belong[s]), int(e[s])
    assert x >= oth
    dis1 = dis2 = 0.0
    for i in range(5):
        if cid[s * 5 + i] != -1:
            val = float(row[cid[s * 5 + i]]) - float(cdis[s * 5 + i])
            if val > dis1:
                dis1 = val
    oe = int(head[oth])
    while int(e[oe]) != x:
        oe = int(nxt[oe])
    for i in range(5):
        if cid[oe * 5 + i] != -1:
            val = float(row[cid[oe * 5 + i]]) - float(cdis[oe * 5 + i])
            if val > dis2:
                dis2 = val
    L = float(ln[s])
    add = (dis1 + dis2 - L) / 2
    if add < 0:
        add = 0.0
    dis1 -= add
    dis2 -= add
    if dis1 < 0:
        dis1 = 0.0
    if dis2 < 0:
        dis2 = 0.0
    if dis1 > L:
        add += dis1 - L
        dis1 = L
    if dis2 > L:
        add += dis2 - L
        dis2 = L
    rest = L - dis1 - dis2
    dis1 += rest / 2
    return dis1, add


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_f64(a, b):
    """element-wise: the same bits, or both NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, p, what=""):
    """the ABI's (slot, frac, add) against a Placement"""
    slot, frac, add = got
    assert len(slot) == len(p.slot), what
    bad = np.flatnonzero(slot != p.slot)
    assert bad.size == 0, (what, "slot", bad[:8], slot[bad[:8]], p.slot[bad[:8]], add[bad[:8]], p.win_add[bad[:8]])
    bad = np.flatnonzero(bits(add) != bits(p.win_add))
    assert bad.size == 0, (what, "add", bad[:8], add[bad[:8]], p.win_add[bad[:8]])
    bad = np.flatnonzero(~same_f64(frac, p.win_frac))
    assert bad.size == 0, (what, "frac", bad[:8], frac[bad[:8]], p.win_frac[bad[:8]])
