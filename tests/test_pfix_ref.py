"""The NumPy reference of the fixed-backbone placement (tests/_pfix_ref.py) against the oracle, on the CPU.

Where the oracle's default tuple (slot 0, add 2) cannot win -- random rows <= 0.5, so every add < 2 -- orc_place_run's
trace[m] for the query as the first tip added is the definition's triple: bit for bit on every backbone shape of
tests/test_gpu_place_fixed.py and a 1 500-tip random one.  For rows holding NaN, +inf and values up to 10, where
orc_place_run no longer is the definition, the per-slot tables are held against scan_scalar, the statement-by-statement
transcription of orc_edge_scan's eligible branch."""
import numpy as np
import pytest

from tests import _jplace, _pfix_ref

SHAPES = [(3, "caterpillar"), (4, "balanced"), (6, "random"), (40, "random"), (300, "random"), (1500, "random")]


def backbone(m, kind, zero_frac=0.2):
    return _jplace.random_backbone(np.random.default_rng(100 + m), m, kind, zero_frac=zero_frac)


_STATE = {}


def state(orc, m, kind):
    if (m, kind) not in _STATE:
        st, _ = _jplace.backbone_arrays(orc, backbone(m, kind), m + 1)
        orc.place_init_lists(m + 1, m, st)
        _STATE[(m, kind)] = st
    return _STATE[(m, kind)]


@pytest.mark.parametrize("m,kind", SHAPES)
def test_reference_equals_place_run_where_the_default_tuple_cannot_win(orc, m, kind):
    st0 = state(orc, m, kind)
    Q = 40 if m <= 300 else 12
    rows = np.random.default_rng(7 * m).uniform(0.0, 0.5, size=(Q, m))
    rows[1] = rows[0]                                                            # the same row twice
    rows[2] = 0.0                                                                # ties on every edge: the lowest eligible slot
    p = _pfix_ref.place(st0, m, rows)
    assert np.all(p.add < 2.0)
    assert p.slot[2] == p.slots[0] and p.win_add[2] == 0.0
    for q in range(Q):
        st = {k: v.copy() for k, v in st0.items()}
        D = np.zeros((m + 1, m + 1))
        D[m, :m] = rows[q]
        slot, frac, add = orc.place_run(D, first=m, state=st)["trace"][m]
        assert int(slot) == p.slot[q], (q, slot, p.slot[q])
        assert _pfix_ref.bits(add) == _pfix_ref.bits(p.win_add[q]) and _pfix_ref.bits(frac) == _pfix_ref.bits(p.win_frac[q]), q
    # the tables hold the winner's values and nothing smaller before it
    q = np.arange(Q)
    assert np.array_equal(p.add[q, p.win], p.win_add) and np.all(p.add >= p.win_add[:, None])
    assert all(np.all(p.add[k, :p.win[k]] > p.win_add[k]) for k in range(Q))


def hostile_rows(rng, Q, m):
    """values up to 10, with +inf and NaN cells, one row all +inf, one all NaN, one half NaN"""
    rows = rng.uniform(0.0, 10.0, size=(Q, m))
    rows[rng.random((Q, m)) < 0.15] = np.inf
    rows[rng.random((Q, m)) < 0.15] = np.nan
    rows[0] = np.inf
    rows[1] = np.nan
    rows[2, : m // 2] = np.nan
    rows[3] = rng.uniform(0.0, 0.05, size=m)                                     # and a close one
    return rows


@pytest.mark.parametrize("m,kind,zero_frac", [(6, "random", 0.2), (40, "random", 0.5), (300, "random", 0.2), (300, "caterpillar", 0.2)])
def test_tables_equal_the_scalar_transcription_on_nonfinite_rows(orc, m, kind, zero_frac):
    st, _ = _jplace.backbone_arrays(orc, backbone(m, kind, zero_frac), m + 1)
    orc.place_init_lists(m + 1, m, st)
    rng = np.random.default_rng(900 + m)
    Q = 12
    rows = hostile_rows(rng, Q, m)
    p = _pfix_ref.place(st, m, rows)
    E = len(p.slots)
    picks = [(q, k) for q in range(4) for k in (0, E - 1)] + [(int(rng.integers(Q)), int(rng.integers(E))) for _ in range(50)]
    picks += [(q, int(p.win[q])) for q in range(Q)]
    seen_inf = seen_nan_frac = 0
    for q, k in picks:
        frac, add = _pfix_ref.scan_scalar(st, rows[q], int(p.slots[k]))
        assert not np.isnan(add)
        assert _pfix_ref.bits(add) == _pfix_ref.bits(p.add[q, k]), (q, k, add, p.add[q, k])
        assert _pfix_ref.same_f64(frac, p.frac[q, k]), (q, k, frac, p.frac[q, k])
        seen_inf += np.isinf(add)
        seen_nan_frac += np.isnan(frac)
    assert seen_inf > 0 and seen_nan_frac > 0
    # what the definition gives for the engineered rows
    assert np.all(np.isinf(p.add[0])) and p.slot[0] == p.slots[0] and np.isnan(p.win_frac[0])
    assert np.all(p.add[1] == 0.0) and p.slot[1] == p.slots[0] and p.win_frac[1] == st["len"][p.slots[0]] / 2
    assert np.isfinite(p.win_add[3]) and p.win_add[3] < 2.0
    # winner = smallest (add, slot)
    for q in range(Q):
        best = min((p.add[q, k], int(p.slots[k])) for k in range(E))
        assert (p.win_add[q], int(p.slot[q])) == best


def test_branch_masks_describe_the_scalar_run(orc):
    """the masks of the vectorised form are the `if`s the scalar form takes"""
    m = 40
    st = state(orc, m, "random")
    rows = np.random.default_rng(5).uniform(0.0, 3.0, size=(6, m))
    p = _pfix_ref.place(st, m, rows)
    for b in _pfix_ref.BRANCHES:
        assert np.array_equal(p.any_took[b], p.took[b].any(axis=1))
        assert np.array_equal(p.win_took[b], p.took[b][np.arange(6), p.win])
    assert np.all(p.add[p.took["a<0"]] >= 0.0) and np.all(p.add[p.took["a<0"] & ~p.took["dis1>L"] & ~p.took["dis2>L"]] == 0.0)
