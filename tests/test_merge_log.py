"""What counts as a merge log, at every host entry point that takes one (no GPU needed).  Two rules are in force: the support and
BME functions take what dpr_nj_run emits, 0 <= x < y < n - it; the two tree converters also take a descending pair, 0 <= x, y <
n - it with x != y.  n = 5 is the smallest size at which the support functions read the log at all: an NJ log has three entries over
5, 4 and 3 live slots, a UPGMA log a fourth over 2.  The expected trees are replayed by hand below, not computed."""
import numpy as np
import pytest

N = 5
GOOD = ([0, 0, 0], [4, 3, 2])             # every y is the last live slot: nothing moves
PAST = ([0, 0, 0], [4, 4, 1])             # it = 1: slot 4 of 4 live ones
EQUAL = ([1, 0, 0], [1, 1, 1])
NEGATIVE = ([-1, 0, 0], [4, 3, 2])
DESCENDING = ([3, 0, 0], [1, 1, 1])
STRICT_RULE = "0 <= x < y < n - it"
LENIENT_RULE = "0 <= x, y < n - it, x != y"
BX, BY, LAST = [0.25, 0.5, 0.75], [1.25, 1.5, 1.75], 3.0


def metric():
    """a 5 x 5 metric: points on a line"""
    at = np.array([0.0, 1.0, 2.5, 4.0, 7.0])
    return np.abs(at[:, None] - at[None, :])


def strict_entry_points():
    """name -> call(log): the five entry points under the strict rule; the support functions get `log` as the main tree and as the
    replicate, each next to a good log"""
    from dipper_amd import capi
    out = {}
    for name, fn in (("split_support", capi.split_support), ("transfer_support_host", capi.transfer_support_host),
                     ("transfer_taxa_host", capi.transfer_taxa_host)):
        out[name + " (main)"] = lambda log, fn=fn: fn(N, log[0], log[1], GOOD[0], GOOD[1])
        out[name + " (replicate)"] = lambda log, fn=fn: fn(N, GOOD[0], GOOD[1], log[0], log[1])
    out["bme_nni_host"] = lambda log: capi.bme_nni_host(metric(), log[0], log[1], 1)
    out["bme_spr_host"] = lambda log: capi.bme_spr_host(metric(), log[0], log[1], 1)
    return out


def from_nj(log):
    from dipper_amd import capi
    return capi.tree_from_nj(log[0], log[1], BX, BY, LAST)


def refused(call, log, rule):
    from dipper_amd import capi
    with pytest.raises(capi.DipperError) as ei:
        call(log)
    assert ei.value.code == -1 and rule in str(ei.value), str(ei.value)


def test_accepted_by_all():
    for name, call in strict_entry_points().items():
        call(GOOD)
    # node 5 joins tips 0 and 4, node 6 joins 5 and tip 3, node 7 joins 6 and tip 2; the root 8 joins 7 and tip 1
    parent, length = from_nj(GOOD)
    assert parent.tolist() == [5, 8, 7, 6, 5, 6, 7, 8, -1]
    assert length.tolist() == [BX[0], LAST / 2, BY[2], BY[1], BY[0], BX[1], BX[2], LAST / 2, 0.0]


@pytest.mark.parametrize("log", [PAST, EQUAL, NEGATIVE], ids=["one_past_the_last_live_slot", "equal_slots", "negative_slot"])
def test_rejected_by_all(log):
    for name, call in strict_entry_points().items():
        refused(call, log, STRICT_RULE)
    refused(from_nj, log, LENIENT_RULE)


def test_descending_pair():
    for name, call in strict_entry_points().items():
        refused(call, DESCENDING, STRICT_RULE)
    # node 5 joins the nodes of slots 3 and 1, tips 3 and 1; it stays in slot 3, slot 4 (tip 4) moves to slot 1.  Node 6 joins the nodes
    # of slots 0 and 1, tips 0 and 4; slot 3 (node 5) moves to slot 1.  Node 7 joins 6 and 5; slot 2 (tip 2) moves to slot 1.  The root 8
    # joins 7 and tip 2.
    parent, length = from_nj(DESCENDING)
    assert parent.tolist() == [6, 5, 8, 5, 6, 7, 7, 8, -1]
    # the x child on bx[it], the y child on by[it], the root's two children on half of `last` each
    assert length.tolist() == [BX[1], BY[0], LAST / 2, BX[0], BY[1], BY[2], BX[2], LAST / 2, 0.0]


def test_upgma_log():
    from dipper_amd import capi
    heights = [1.0, 2.0, 3.0, 4.0]
    # node 5 (height 1) joins tips 0 and 4; node 6 (2) joins 5 and tip 3; node 7 (3) joins 6 and tip 2; the root 8 (4) joins 7 and tip 1:
    # a branch is the parent's height minus the child's, a tip's height being 0
    for last in ((0, 1), (1, 0)):
        parent, length = capi.tree_from_upgma([0, 0, 0, last[0]], [4, 3, 2, last[1]], heights)
        assert parent.tolist() == [5, 8, 7, 6, 5, 6, 7, 8, -1]
        assert length.tolist() == [1.0, 4.0, 3.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.0]
    for last in ((0, 2), (2, 1), (0, 0), (1, 1), (-1, 1), (0, -1)):
        refused(lambda log: capi.tree_from_upgma(log[0], log[1], heights), ([0, 0, 0, last[0]], [4, 3, 2, last[1]]), LENIENT_RULE)
    # the first three entries fall under the same rule as an NJ log's
    for x, y in (PAST, EQUAL, NEGATIVE):
        refused(lambda log: capi.tree_from_upgma(log[0], log[1], heights), (x + [0], y + [1]), LENIENT_RULE)
    parent, _ = capi.tree_from_upgma(DESCENDING[0] + [1], DESCENDING[1] + [0], heights)
    assert parent.tolist() == [6, 5, 8, 5, 6, 7, 7, 8, -1]
