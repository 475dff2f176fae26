"""GPU tests of the NJ plan of a context (dpr_nj_plan_resolve decides it, every entry point reads it): one context taken through
several plans in a row reports and runs each of them, none of them leaves anything behind for the next, and a rank that holds
the whole matrix reads the final distance from its own copy.  Merge logs bit for bit against the oracle (NJ) and the host
restatement (BIONJ)."""
import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu
KEYS = ("merge_x", "merge_y", "bl_x", "bl_y")
EXCHANGE = {0: "legacy", 1: "peer", 2: "mailbox"}


def _same(res, ref, what):
    assert res["iters"] == ref["iters"], what
    for key in KEYS:
        assert np.array_equal(res[key], ref[key]), (what, key)
    assert res["last_d"] == ref["last_d"], what


def test_single_rank_context_through_its_plans(orc):
    """pruned, streaming, BIONJ, pruned with 4 virtual shards, pruned with 1: one context, n = 300"""
    import dipper_amd
    from dipper_amd import capi
    n = 300
    D = _util.random_additive_matrix(np.random.default_rng(5), n, zero_frac=0.2)
    D = np.tril(D, -1) + np.tril(D, -1).T
    ref = orc.nj_run(np.tril(D, -1))
    host = capi.nj_variant_host(1, D)
    # (variant, mode, virtual shards)
    steps = [("pruned", 0, 1, 1), ("streaming", 0, 0, 1), ("bionj", 1, 0, 1), ("pruned, 4 virtual shards", 0, 1, 4), ("pruned, 1 shard", 0, 1, 1)]
    d = dipper_amd.Dipper(0)
    try:
        d.set_matrix_full(D)
        for i, (what, variant, mode, vshards) in enumerate(steps):
            d.set_nj_variant(variant)
            d.set_nj_mode(mode)
            d.set_nj_virtual_shards(vshards)
            d.dist_matrix(capi.SRC_MATRIX)
            res = d.nj_run()
            if variant == 1:
                _same(res, host, what)
                assert np.array_equal(d.nj_lambda(), host["lam"]), what
            else:
                _same(res, ref, what)
            assert res["iters"] == n - 2, what
            assert d.nj_multi_info() == "single rank", what
            assert d.nj_is_unit_sharded() == 0, what
            if i > 0 and steps[i - 1][1] == 1:
                with pytest.raises(capi.DipperError):      # the BIONJ matrix is gone
                    d.nj_lambda()
    finally:
        d.close()


def test_virtual_ranks_context_through_its_plans(orc):
    """streaming with the legacy exchange, with mailboxes, rows pruned, streaming with the peer exchange: one context of 3 virtual
    ranks, n = 1300; what one plan reports is not what the one before it left"""
    import dipper_amd
    from dipper_amd import capi
    n = 1300
    D = _util.random_additive_matrix(np.random.default_rng(6), n, zero_frac=0.2)
    ref = orc.nj_run(np.tril(D, -1), threads=8)
    # (mode, exchange, expected active exchange plan of the streaming loop or None)
    steps = [(0, 0, 0), (0, 2, 2), (1, 1, None), (0, 1, 1)]
    d = dipper_amd.Dipper(0, virtual_world=3)
    try:
        d.set_nj_multi_plan(3)
        d.set_matrix_full(D)
        for i, (mode, exchange, active) in enumerate(steps):
            d.set_nj_mode(mode)
            d.set_nj_exchange(exchange)
            d.dist_matrix(capi.SRC_MATRIX)
            _same(d.nj_run(), ref, f"step {i}")
            info = d.nj_exchange_info()
            if active is None:
                assert "row-sharded pruned" in info["note"], info
            else:
                assert info["plan"] == EXCHANGE[active], (i, info)
                assert "row-sharded pruned" not in info["note"], (i, info)
                assert d.nj_multi_info().startswith("streaming, rows sharded"), (i, d.nj_multi_info())
            assert d.nj_is_unit_sharded() == 0
    finally:
        d.close()


def test_replica_rank_reads_the_final_distance_from_its_own_copy(orc, monkeypatch):
    """replicas plan (several real ranks, each on its own whole copy): no collective and no window, so one process can be any
    rank of it.  The run hands over to the streaming loop once and ends in slot space; every rank then reads D[1][0] from the
    matrix it holds."""
    import dipper_amd
    from dipper_amd import capi
    monkeypatch.setenv("DPR_NJ_STREAM_FRAC", "0")
    monkeypatch.setenv("DPR_NJ_GRAPH_ITERS", "8")
    monkeypatch.delenv("DPR_NJ_EPOCH_MIN", raising=False)
    n = 900
    D = np.random.default_rng(11).random((n, n))
    D = np.tril(D, -1) + np.tril(D, -1).T
    ref = orc.nj_run(np.tril(D, -1))
    got = []
    for rank in (1, 0):
        d = dipper_amd.Dipper(0)
        try:
            d.comm_init_local(rank, 2)
            d.set_nj_mode(1)
            d.set_nj_multi_plan(2)
            d.set_matrix_full(D)
            d.dist_matrix(capi.SRC_MATRIX)
            assert "replicas" in d.nj_multi_info()
            res = d.nj_run()
            _same(res, ref, f"rank {rank} of 2")
            assert d.nj_adaptive_stats()[1] >= 1          # handed over: the run ended in slot space
            got.append(res)
        finally:
            d.close()
    _same(got[0], got[1], "rank 1 against rank 0")
