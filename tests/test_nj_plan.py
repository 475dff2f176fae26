"""CPU test of dpr_nj_plan_resolve: the one function that chooses a context's NJ plan.  Every row of its table (include/
dipper_hip.h) with the expected kind written out here; the rows of several real ranks cannot be reached on one GPU, so this is
where they are pinned."""
import itertools

import pytest

from dipper_amd import capi

SS, SP, BIONJ, RS, REPL, UNIT, RP = range(7)
GIB, BIG = 2 ** 30, 2 ** 50


def resolve(world, virtual, variant, pruned, multi, vshards, n, total=BIG):
    return capi.nj_plan_resolve(world, virtual, variant, pruned, multi, vshards, n, total)


def test_constants_are_the_headers():
    assert (capi.NJ_PLAN_SINGLE_STREAM, capi.NJ_PLAN_SINGLE_PRUNED, capi.NJ_PLAN_BIONJ, capi.NJ_PLAN_ROWS_STREAM, capi.NJ_PLAN_REPLICAS,
            capi.NJ_PLAN_UNIT_SHARDED, capi.NJ_PLAN_ROWS_PRUNED) == (SS, SP, BIONJ, RS, REPL, UNIT, RP)


def test_bionj_is_bionj_whatever_mode_and_multi_plan_say():
    for world, pruned, multi, n, total in itertools.product((1, 2, 8), (0, 1), (0, 1, 2, 3), (2, 3, 300, 70000), (GIB, BIG)):
        assert resolve(world, False, 1, pruned, multi, 1, n, total) == BIONJ, (world, pruned, multi, n, total)


@pytest.mark.parametrize("world,virtual,vshards", [(2, True, 1), (4, True, 4), (1, False, 2), (4, False, 64)])
def test_bionj_refuses_virtual_ranks_and_virtual_shards(world, virtual, vshards):
    with pytest.raises(capi.DipperError) as ei:
        resolve(world, virtual, 1, 1, 0, vshards, 300)
    assert ei.value.code == -1 and "BIONJ" in str(ei.value)


def test_one_rank():
    for multi, vshards, total in itertools.product((0, 1, 2, 3), (1, 4), (GIB, BIG)):
        assert resolve(1, False, 0, 1, multi, vshards, 3, total) == SP          # virtual shards are a detail of the pruned plan
        assert resolve(1, False, 0, 1, multi, vshards, 70000, total) == SP
        assert resolve(1, False, 0, 1, multi, vshards, 2, total) == SS          # n < 3
        assert resolve(1, False, 0, 0, multi, vshards, 300, total) == SS        # streaming wanted


def test_several_ranks_streaming_or_tiny_is_rows_streaming():
    for world, virtual, multi, total in itertools.product((2, 3, 8), (False, True), (0, 1, 2, 3), (GIB, BIG)):
        assert resolve(world, virtual, 0, 0, multi, 1, 300, total) == RS
        assert resolve(world, virtual, 0, 0, multi, 1, 70000, total) == RS
        assert resolve(world, virtual, 0, 1, multi, 1, 2, total) == RS


def test_virtual_ranks_pruned():
    for world, n in itertools.product((2, 3, 8), (3, 1300, 70000)):
        assert resolve(world, True, 0, 1, 3, 1, n) == RP
        for multi in (0, 1, 2):
            assert resolve(world, True, 0, 1, multi, 1, n, BIG) == RS
            assert resolve(world, True, 0, 1, multi, 1, n, 1) == RS             # whatever the memory says


def test_real_ranks_pruned_explicit_plans():
    for world, n, total in itertools.product((2, 4), (3, 1300, 70000), (1, GIB, BIG)):
        assert resolve(world, False, 0, 1, 3, 1, n, total) == RP
        assert resolve(world, False, 0, 1, 1, 1, n, total) == UNIT
        assert resolve(world, False, 0, 1, 2, 1, n, total) == REPL


def test_real_ranks_auto_memory_rule():
    # 16 * 7552**2 = 912 523 264 <= 0.85 * 2**30 = 912 680 550.4 < 16 * 7553**2 = 912 764 944
    assert resolve(4, False, 0, 1, 0, 1, 7552, GIB) == REPL
    assert resolve(4, False, 0, 1, 0, 1, 7553, GIB) == RP
    assert resolve(2, False, 0, 1, 0, 1, 70000, GIB) == RP                      # (the memory rule comes before the tip count)


def test_real_ranks_auto_unit_sharded_from_65536_tips():
    assert resolve(4, False, 0, 1, 0, 1, 65535, BIG) == REPL
    assert resolve(4, False, 0, 1, 0, 1, 65536, BIG) == UNIT
    assert resolve(2, False, 0, 1, 0, 1, 3, BIG) == REPL


@pytest.mark.parametrize("args", [(0, 0, 0, 1, 0, 1, 300), (2, 0, 2, 1, 0, 1, 300), (2, 0, 0, 1, 4, 1, 300), (2, 0, 0, 1, -1, 1, 300),
                                  (2, 0, 0, 1, 0, 0, 300), (2, 0, 0, 1, 0, 1, 1)])
def test_bad_arguments(args):
    with pytest.raises(capi.DipperError) as ei:
        resolve(*args)
    assert ei.value.code == -1
