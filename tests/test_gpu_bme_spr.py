"""GPU tests of the balanced minimum evolution SPR search (dpr_bme_spr): the device -- table, mirror, scan and best-of-two-sides
kernels -- against the host restatement dpr_bme_spr_host bit for bit (tests/test_bme_spr.py pins that restatement against a
reference without tables), over the sizes where the launches change shape, deep and shallow trees, every layout of the fresh
matrix, non-finite and tied distances; the shared table; the state and argument errors."""
import numpy as np
import pytest

from tests import _bme_ref as R, _nonfinite
from tests.test_bme_nni import start_log
from tests.test_bme_spr import TIE_INPUT, tie_input

pytestmark = pytest.mark.gpu
ROUNDS = 6


@pytest.fixture(scope="module")
def dev():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_same(got, ref):
    for k in ("rounds", "moves", "fallbacks", "candidates0", "long_moves", "max_k", "top"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("kids", "L_rounds", "len"):
        assert same_bits(got[k], ref[k]), (k, got[k][:8], ref[k][:8])


def device_search(d, D, mx, my, rounds=ROUNDS):
    from dipper_amd import capi
    d.set_matrix_full(D)
    d.dist_matrix(capi.SRC_MATRIX)
    return d.bme_spr(mx, my, rounds)


_inputs = {}


def noisy(n):
    if n not in _inputs:
        _inputs[n] = R.random_matrix(np.random.default_rng(100 + n), n)
    return _inputs[n]


# ---- device against the host restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5, 8, 33, 65, 257, 1000])
def test_nj_trees_equal_the_host_bit_for_bit(dev, n):
    from dipper_amd import capi
    D = noisy(n)
    mx, my = start_log("nj", n, D)
    got = device_search(dev, D, mx, my)
    assert_same(got, capi.bme_spr_host(D, mx, my, ROUNDS))
    if n >= 65:
        assert got["rounds"] >= 2 and got["long_moves"] >= 2


@pytest.mark.parametrize("start,n", [("caterpillar", 300), ("caterpillar", 1200), ("balanced", 256)])
def test_deep_and_shallow_trees(dev, start, n):
    """the caterpillar's paths reach n - 3 edges: at 1 200 tips beyond the 1 074 halvings after which a coefficient is zero"""
    from dipper_amd import capi
    D = noisy(n)
    mx, my = start_log(start, n, D)
    rounds = 3 if n > 1000 else ROUNDS
    got = device_search(dev, D, mx, my, rounds)
    assert_same(got, capi.bme_spr_host(D, mx, my, rounds))
    assert got["rounds"] >= 2 and got["moves"] > got["rounds"] and got["long_moves"] >= 1
    if start == "caterpillar":
        assert got["max_k"] > 64


@pytest.mark.parametrize("plan", ["stream", "pruned", "bionj"])
@pytest.mark.parametrize("n", [5, 65, 257])
def test_every_layout_of_the_fresh_matrix(n, plan):
    """the streaming plan keeps the fresh matrix in slot space, the pruned plan in position space, BIONJ beside its variances:
    the same table either way"""
    import dipper_amd
    from dipper_amd import capi
    D = noisy(n)
    d = dipper_amd.Dipper(0)
    try:
        if plan == "bionj":
            d.set_nj_variant(1)
        else:
            d.set_nj_mode(1 if plan == "pruned" else 0)
        mx, my = start_log("bionj" if plan == "bionj" else "nj", n, D)
        assert_same(device_search(d, D, mx, my), capi.bme_spr_host(D, mx, my, ROUNDS))
    finally:
        d.close()


@pytest.mark.parametrize("name", ["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_nonfinite_distances(dev, name):
    from dipper_amd import capi
    n = 100
    D = dict(_nonfinite.matrices(n, 5))[name]
    mx, my = R.balanced_log(n)
    got = device_search(dev, D, mx, my)
    assert_same(got, capi.bme_spr_host(D, mx, my, ROUNDS))
    assert not np.isfinite(got["L_rounds"][0]) and got["rounds"] == 0


def test_exact_ties(dev):
    from dipper_amd import capi
    D, mx, my = tie_input(*TIE_INPUT)
    got = device_search(dev, D, mx, my)
    assert_same(got, capi.bme_spr_host(D, mx, my, ROUNDS))
    assert got["moves"] >= 2
    n = 40
    flat = np.full((n, n), 2.0)
    np.fill_diagonal(flat, 0.0)
    cx, cy = R.caterpillar_log(n)
    got = device_search(dev, flat, cx, cy)
    assert_same(got, capi.bme_spr_host(flat, cx, cy, ROUNDS))
    assert (got["rounds"], got["candidates0"]) == (0, 0)


def test_zero_rounds_equals_the_nni_entry_point(dev):
    from dipper_amd import capi
    n = 65
    D = noisy(n)
    mx, my = start_log("nj", n, D)
    a = device_search(dev, D, mx, my, 0)
    dev.dist_matrix(capi.SRC_MATRIX)
    b = dev.bme_nni(mx, my, 0)
    for k in ("kids", "len", "L_rounds"):
        assert same_bits(a[k], b[k])
    assert a["top"] == b["top"]


# ---- the shared table, state, arguments -------------------------------------------------------------------------------------
def test_table_is_shared_with_nni_and_nothing_is_allocated_twice():
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        n = 257
        D = noisy(n)
        mx, my = start_log("balanced", n, D)
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        d.bme_nni(mx, my, 2)
        s1 = d.bme_stats()
        assert s1["allocations"] == 4 and d.bme_spr_stats()["allocations"] == 0 and d.bme_spr_stats()["stack_bytes"] == 0
        first = device_search(d, D, mx, my)
        s2, p2 = d.bme_stats(), d.bme_spr_stats()
        assert s2["allocations"] == 4 and s2["table_bytes"] == s1["table_bytes"]          # no new table
        assert p2["allocations"] == 5 and p2["stack_bytes"] == p2["workers"] * 3 * 32 * 12 and p2["launches"] == 4 * s2["evaluations"]
        assert_same(first, capi.bme_spr_host(D, mx, my, ROUNDS))
        small = noisy(65)                                                                   # fewer tips: the same buffers
        sx, sy = start_log("nj", 65, small)
        assert_same(device_search(d, small, sx, sy), capi.bme_spr_host(small, sx, sy, ROUNDS))
        assert d.bme_stats()["allocations"] == 4 and d.bme_spr_stats()["allocations"] == 5
        table_ms, select_ms = d.bme_timing()
        assert table_ms > 0 and select_ms > 0 and d.bme_spr_timing() > 0
        d.dist_matrix(capi.SRC_MATRIX)                                                      # the NNI search after the scan's mirror
        assert np.array_equal(d.bme_nni(sx, sy, ROUNDS)["kids"], capi.bme_nni_host(small, sx, sy, ROUNDS)["kids"])
    finally:
        d.close()


def test_state_error_after_an_nj_iteration(dev):
    from dipper_amd import capi
    n = 64
    D = noisy(65)[:n, :n]
    mx, my = start_log("nj", n, D)
    dev.set_matrix_full(D)
    dev.dist_matrix(capi.SRC_MATRIX)
    dev.nj_run(max_iters=1)
    with pytest.raises(capi.DipperError) as ei:
        dev.bme_spr(mx, my, 3)
    assert ei.value.code == -3
    dev.dist_matrix(capi.SRC_MATRIX)                 # a fresh matrix again
    assert_same(dev.bme_spr(mx, my, 3), capi.bme_spr_host(D, mx, my, 3))
    with pytest.raises(capi.DipperError) as ei:      # a log that is none, and one of another size
        dev.bme_spr(my, mx, 3)
    assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        dev.bme_spr(mx[:10], my[:10], 3)
    assert ei.value.code == -1


def test_virtual_ranks_and_shards_are_refused():
    import dipper_amd
    from dipper_amd import capi
    n = 200
    D = noisy(257)[:n, :n]
    mx, my = start_log("nj", n, D)
    d = dipper_amd.Dipper(0, virtual_world=2)
    try:
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        with pytest.raises(capi.DipperError) as ei:
            d.bme_spr(mx, my, 3)
        assert ei.value.code == -1
    finally:
        d.close()
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_virtual_shards(2)
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        with pytest.raises(capi.DipperError) as ei:
            d.bme_spr(mx, my, 3)
        assert ei.value.code == -1
        d.set_nj_virtual_shards(-1)
        assert_same(device_search(d, D, mx, my, 3), capi.bme_spr_host(D, mx, my, 3))
    finally:
        d.close()
