"""GPU tests of UPGMA / WPGMA (dpr_upgma_run): the device loop -- a nearest neighbour cached per row, three launches an iteration --
against the naive host restatement dpr_upgma_host bit for bit (tests/test_upgma.py pins that restatement against a NumPy reference
from the definition), over the sizes where the launches change shape, both linkages, every layout of the fresh matrix and every
distance source; the inputs that drive the cache's special cases; non-finite distances; and what the call leaves of the context.

Which launch a size is an edge of (a run at n passes through every m <= n; the first fill of the cache scans at m = n):
  2, 3            the last slots: no rescan after the last merge, one slot left to move;
  63, 64, 65      a wavefront of the reductions in pick and rescan;
  255, 256, 257   a workgroup of update, fill and init (256 threads, one per slot / column);
  600, 1 000      several workgroups of update; pick and rescan still within one pass of their 1 024 threads;
  1 023 .. 1 025  pick's 1 024 threads: above it a thread reduces a second cache entry (its own (key, pair) order between passes);
  2 100           rescan's 1 024 threads x 2 doubles = 2 048 columns: above it a thread takes a second 16-byte load of a row, and the
                  odd tail (m = 2 049) and three entries a thread in pick (m > 2 048) are passed on the way down.
The tie-heavy inputs at 1 025 and 2 100 make the (key, index) order decide between a thread's several entries."""
import numpy as np
import pytest

from tests import _aa_ref, _nonfinite, _upgma_ref as R, _util
from tests.test_upgma import assert_same_log, tie_matrix

pytestmark = pytest.mark.gpu
SIZES = [2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 600, 1000, 1023, 1024, 1025, 2100]
LINK = pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])


@pytest.fixture(scope="module")
def dev():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


_inputs = {}


def noisy(n):
    if n not in _inputs:
        D = R.noisy_matrix(np.random.default_rng(900 + n), n)
        D.setflags(write=False)
        _inputs[n] = D
    return _inputs[n]


_host = {}


def host(name, D, linkage):
    """dpr_upgma_host on a named input: computed once (the naive loop is cubic), shared, never changed"""
    from dipper_amd import capi
    if (name, linkage) not in _host:
        _host[(name, linkage)] = capi.upgma_host(D, linkage)
    return _host[(name, linkage)]


def check_counts(d, n):
    """rows x and y are scanned again after every merge but the last; no iteration lists more rows than it has slots"""
    st = d.upgma_stats()
    assert st["rescanned"] >= 2 * (n - 2), (st, n)
    assert st["rescanned"] <= sum(n - it for it in range(max(n - 2, 0))), (st, n)
    assert st["launches"] == 3 + 3 * (n - 1) - 1
    return st


def device_run(d, D, linkage):
    from dipper_amd import capi
    d.set_matrix_full(D)
    d.dist_matrix(capi.SRC_MATRIX)
    got = d.upgma(linkage)
    assert len(got["merge_x"]) == len(got["merge_y"]) == len(got["height"]) == D.shape[0] - 1
    check_counts(d, D.shape[0])
    return got


# ---- device against the host restatement ------------------------------------------------------------------------------------
@LINK
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_bit_for_bit(dev, n, linkage):
    D = noisy(n)
    assert_same_log(device_run(dev, D, linkage), host(("noisy", n), D, linkage))


@LINK
@pytest.mark.parametrize("mode", [1, 0], ids=["pruned", "stream"])
@pytest.mark.parametrize("n", [5, 65, 600])
def test_both_matrix_layouts(n, mode, linkage):
    """the pruned plan keeps the fresh matrix in position space, the streaming plan in slot space: the same copy either way"""
    import dipper_amd
    D = noisy(n)
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_mode(mode)
        assert_same_log(device_run(d, D, linkage), host(("noisy", n), D, linkage))
    finally:
        d.close()


@LINK
def test_bionj_context(dev, linkage):
    D = noisy(257)
    dev.set_nj_variant(1)
    try:
        assert_same_log(device_run(dev, D, linkage), host(("noisy", 257), D, linkage))
    finally:
        dev.set_nj_variant(0)


@LINK
def test_alignment_source(dev, linkage):
    from dipper_amd import capi
    seqs = _util.synth_alignment(np.random.default_rng(3), n=130, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    dev.set_msa(capi.pack4_many(seqs), 300)
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    M = dev.matrix()
    got = dev.upgma(linkage)
    check_counts(dev, 130)
    assert_same_log(got, host("alignment", M, linkage))      # short alignments: many equal distances, the tie rule at work


@LINK
def test_protein_source(dev, linkage):
    from dipper_amd import capi
    seqs = _aa_ref.evolve_yule(np.random.default_rng(9), 90, 200)
    dev.set_msa_aa(capi.pack_aa_many(seqs))
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)
    M = dev.matrix()
    got = dev.upgma(linkage)
    check_counts(dev, 90)
    assert_same_log(got, host("protein", M, linkage))


# ---- the cache's special cases ----------------------------------------------------------------------------------------------
@LINK
@pytest.mark.parametrize("n", [8, 130, 1025, 2100])
def test_whole_number_ties(dev, n, linkage):
    D = tie_matrix(n)
    assert_same_log(device_run(dev, D, linkage), host(("ties", n), D, linkage))


@LINK
@pytest.mark.parametrize("n", [65, 130, 2100])
def test_all_equal_matrix_lists_every_row(dev, n, linkage):
    D = R.symmetric(np.full((n, n), 0.375))
    got = device_run(dev, D, linkage)
    assert_same_log(got, host(("equal", n), D, linkage))
    assert np.all(got["merge_x"] == 0) and np.all(got["merge_y"] == 1)
    # every row's neighbour is slot 0 or 1, the pair that merges: all m - 1 rows that are left are listed in every iteration
    assert dev.upgma_stats()["rescanned"] == sum(n - it - 1 for it in range(n - 2))


@LINK
def test_last_slot_is_every_rows_neighbour_and_is_renamed(dev, linkage):
    """the first winner is (0, 1), so slot n-1 moves to 1 while every other row's cached neighbour is n-1"""
    n = 130
    D = noisy(257)[:n, :n].copy()
    D[:, n - 1] = D[n - 1, :] = 0.02 + 1e-4 * np.arange(n)
    D[n - 1, n - 1] = 0.0
    D[0, 1] = D[1, 0] = 0.001
    ref = host("last_column", D, linkage)
    assert (ref["merge_x"][0], ref["merge_y"][0]) == (0, 1)
    assert all(int(np.argmin(np.where(np.arange(n) == k, np.inf, D[k]))) == n - 1 for k in range(2, n - 1))
    assert_same_log(device_run(dev, D, linkage), ref)


@LINK
def test_first_winner_in_the_last_slot_moves_nothing(dev, linkage):
    n = 130
    D = noisy(257)[:n, :n].copy()
    D[n - 1, 3] = D[3, n - 1] = 0.001
    ref = host("no_move", D, linkage)
    assert (ref["merge_x"][0], ref["merge_y"][0]) == (3, n - 1)
    assert_same_log(device_run(dev, D, linkage), ref)


@LINK
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_nonfinite_distances(dev, which, linkage):
    n = 100
    name, D = _nonfinite.matrices(n, 11)[which]
    got = device_run(dev, D, linkage)
    assert_same_log(got, host(("nonfinite", name), D, linkage))
    finite = np.isfinite(got["height"])
    assert not finite[-1] and finite[0] and not finite[int(np.argmin(finite)):].any()      # they merge last


# ---- repeats, allocations, the context afterwards -------------------------------------------------------------------------------
def test_two_runs_agree_and_the_second_allocates_nothing():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    try:
        n = 257
        D = noisy(n)
        first = device_run(d, D, 0)
        s1 = d.upgma_stats()
        assert s1["allocations"] > 0 and s1["bytes"] >= n * n * 8
        again = device_run(d, D, 0)
        s2 = d.upgma_stats()
        assert_same_log(again, first)
        assert s2["allocations"] == s1["allocations"] and s2["launches"] == s1["launches"] and s2["rescanned"] == s1["rescanned"]
        small = noisy(65)                            # fewer tips: the same buffers
        assert_same_log(device_run(d, small, 1), host(("noisy", 65), small, 1))
        assert d.upgma_stats()["allocations"] == s1["allocations"] and d.upgma_stats()["bytes"] == s1["bytes"]
        assert d.upgma_timing() > 0
    finally:
        d.close()


def test_nj_after_upgma_is_the_nj_of_an_untouched_context(dev):
    import dipper_amd
    from dipper_amd import capi
    n = 257
    D = noisy(n)
    for mode in (1, 0):
        logs = []
        for with_upgma in (False, True):
            d = dipper_amd.Dipper(0)
            try:
                d.set_nj_mode(mode)
                d.set_matrix_full(D)
                d.dist_matrix(capi.SRC_MATRIX)
                if with_upgma:
                    assert_same_log(d.upgma(0), host(("noisy", n), D, 0))
                logs.append(d.nj_run())
            finally:
                d.close()
        for k in ("merge_x", "merge_y", "bl_x", "bl_y"):
            assert np.array_equal(logs[0][k], logs[1][k]), (mode, k)
        assert logs[0]["iters"] == logs[1]["iters"] == n - 2 and logs[0]["last_d"] == logs[1]["last_d"]


def test_state_and_argument_errors(dev):
    import dipper_amd
    from dipper_amd import capi
    n = 64
    D = noisy(n)
    d = dipper_amd.Dipper(0)
    try:
        with pytest.raises(capi.DipperError) as ei:      # no matrix yet
            d.upgma(0)
        assert ei.value.code == -3
    finally:
        d.close()
    dev.set_matrix_full(D)
    dev.dist_matrix(capi.SRC_MATRIX)
    dev.nj_run(max_iters=1)
    with pytest.raises(capi.DipperError) as ei:
        dev.upgma(0)
    assert ei.value.code == -3 and "fresh" in str(ei.value)
    dev.dist_matrix(capi.SRC_MATRIX)                     # a fresh matrix again
    for linkage in (-1, 2):
        with pytest.raises(capi.DipperError) as ei:
            dev.upgma(linkage)
        assert ei.value.code == -1
    assert_same_log(dev.upgma(1), host(("noisy", n), D, 1))


def test_virtual_ranks_and_shards_are_refused():
    import dipper_amd
    from dipper_amd import capi
    n = 200
    D = noisy(257)[:n, :n]
    nj = capi.nj_variant_host(0, D)
    d = dipper_amd.Dipper(0, virtual_world=2)
    try:
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        with pytest.raises(capi.DipperError) as ei:
            d.upgma(0)
        assert ei.value.code == -1
        res = d.nj_run()                             # the context is as usable as before
        assert np.array_equal(res["merge_x"], nj["merge_x"]) and np.array_equal(res["merge_y"], nj["merge_y"])
    finally:
        d.close()
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_virtual_shards(2)
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        with pytest.raises(capi.DipperError) as ei:
            d.upgma(0)
        assert ei.value.code == -1
        d.set_nj_virtual_shards(-1)
        assert_same_log(device_run(d, D, 0), host("noisy200", D, 0))
    finally:
        d.close()
