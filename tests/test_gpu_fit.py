"""GPU tests of the tree fit (dpr_tree_fit, dpr_tree_patristic_rows): the device's two passes -- lowest common ancestors from a sparse
table over the depth-first order of the tips -- against the host restatement dpr_tree_fit_host, which climbs the parent array, bit for
bit (tests/test_fit_tree.py pins that restatement against a NumPy / math.fsum reference); per element against that reference; every
layout of the fresh matrix and every distance source; skipped pairs; and what the call leaves of the context.

Which edge a size is:
  2, 3, 4, 5        the smallest trees: one gap, a table of one row; the star and the first multifurcation;
  15, 16, 17        the 16 accumulators of a column part (wave w takes the rows i = w mod 16);
  63, 64, 65        the 64 columns of a workgroup of the column pass, a wavefront of the row pass's reductions;
  128, 129          a table row more (floor(log2(n - 1)) changes at 129), half the row pass's accumulators;
  255, 256, 257     the 256 accumulators of a row part: above it a thread adds a second term;
  513               two terms and more in every accumulator, nine column workgroups, a caterpillar 512 nodes deep.
Nothing of the lookup is staged in LDS, so no size is the capacity of a staged structure; the caterpillars are the deepest trees of
their size."""
import numpy as np
import pytest

from tests import _aa_ref, _fit_ref as R, _nonfinite, _util
from tests.test_fit_tree import check_against_reference, trees, ultrametric

pytestmark = pytest.mark.gpu
SIZES = [2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256, 257, 513]


@pytest.fixture(scope="module")
def dev():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


_inputs = {}


def noisy(n):
    if n not in _inputs:
        D = R.noisy_matrix(np.random.default_rng(700 + n), n)
        D.setflags(write=False)
        _inputs[n] = D
    return _inputs[n]


def assert_same_fit(got, ref, what=""):
    """every entry of sums, taxon_ss, taxon_pairs and worst, as bits"""
    for k in ("sums", "taxon_ss"):
        a, b = got[k].view(np.uint64), ref[k].view(np.uint64)
        if not np.array_equal(a, b):
            bad = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{what}: {k}[{bad}] differs: {got[k][bad]!r} vs {ref[k][bad]!r}")
    assert np.array_equal(got["taxon_pairs"], ref["taxon_pairs"]), what
    assert np.array_equal(got["worst"], ref["worst"]), (what, got["worst"], ref["worst"])


def load(d, D):
    from dipper_amd import capi
    d.set_matrix_full(D)
    d.dist_matrix(capi.SRC_MATRIX)


# ---- device against the host restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_bit_for_bit(dev, n):
    from dipper_amd import capi
    D = noisy(n)
    load(dev, D)
    for name, (parent, length) in trees(n).items():
        got = dev.tree_fit(parent, length)
        assert_same_fit(got, capi.tree_fit_host(D, parent, length), f"n {n} {name}")
        assert got["n"] == n * (n - 1) // 2 and dev.fit_stats()["launches"] == 2


@pytest.mark.parametrize("mode", [1, 0], ids=["pruned", "stream"])
@pytest.mark.parametrize("n", [5, 65, 600])
def test_both_matrix_layouts(n, mode):
    """the pruned plan keeps the fresh matrix in position space, the streaming plan in slot space: the same entries either way"""
    import dipper_amd
    from dipper_amd import capi
    D = noisy(n)
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_mode(mode)
        load(d, D)
        for name in ("nj", "caterpillar"):
            parent, length = trees(n)[name]
            assert_same_fit(d.tree_fit(parent, length), capi.tree_fit_host(D, parent, length), f"mode {mode} n {n} {name}")
    finally:
        d.close()


def test_bionj_context(dev):
    from dipper_amd import capi
    n = 257
    D = noisy(n)
    dev.set_nj_variant(1)
    try:
        load(dev, D)
        parent, length = trees(n)["nj"]
        assert_same_fit(dev.tree_fit(parent, length), capi.tree_fit_host(D, parent, length))
    finally:
        dev.set_nj_variant(0)


def fit_own_nj_tree(dev, n):
    """the NJ tree of the context's matrix, the matrix built again, the fit against the host's on the matrix read back"""
    from dipper_amd import capi
    M = dev.matrix()
    nj = dev.nj_run()
    parent, length = capi.tree_from_nj(nj["merge_x"], nj["merge_y"], nj["bl_x"], nj["bl_y"], nj["last_d"], n=n)
    return M, parent, length


def test_alignment_source(dev):
    from dipper_amd import capi
    seqs = _util.synth_alignment(np.random.default_rng(3), n=130, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    dev.set_msa(capi.pack4_many(seqs), 300)
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    M, parent, length = fit_own_nj_tree(dev, 130)
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    got = dev.tree_fit(parent, length)
    assert_same_fit(got, capi.tree_fit_host(M, parent, length))
    assert got["explained"] > 0.9      # an NJ tree of distances that come from a tree explains them


def test_protein_source(dev):
    from dipper_amd import capi
    seqs = _aa_ref.evolve_yule(np.random.default_rng(9), 90, 200)
    dev.set_msa_aa(capi.pack_aa_many(seqs))
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)
    M, parent, length = fit_own_nj_tree(dev, 90)
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)
    assert_same_fit(dev.tree_fit(parent, length), capi.tree_fit_host(M, parent, length))


# ---- per element -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 65, 257])
def test_patristic_rows_per_element(dev, n):
    """bit for bit the reference's depth formula; within 4 (h + 2) 2^-53 (sum |len| on the two root paths) of the edges of each path
    added one at a time (the bound of the recursive sums involved)"""
    for name, (parent, length) in trees(n).items():
        t = R.Tree(n, parent, length)
        P = dev.tree_patristic_rows(n, parent, length)
        ref = t.patristic_depth()
        assert np.array_equal(P.view(np.uint64), ref.view(np.uint64)), (n, name)
        Pp, absroot = t.patristic_paths()
        bound = 4 * (t.height + 2) * 2.0 ** -53 * (absroot[:, None] + absroot[None, :])
        assert (np.abs(P - Pp) <= bound).all(), (n, name)
    # a block of rows in the middle
    if n >= 65:
        part = dev.tree_patristic_rows(n, parent, length, row0=n // 2, nrows=3)
        assert np.array_equal(part, P[n // 2:n // 2 + 3])


# ---- an exact case --------------------------------------------------------------------------------------------------------------
def test_exact_case(dev):
    """WPGMA of an ultrametric matrix of small integers times 2^-10 averages equal values: every height and depth is exact"""
    from dipper_amd import capi
    n = 300
    D = ultrametric(n, np.random.default_rng(14))
    up = capi.upgma_host(D, 1)
    parent, length = capi.tree_from_upgma(up["merge_x"], up["merge_y"], up["height"])
    host = capi.tree_fit_host(D, parent, length)      # the construction is exact: checked on the CPU first
    assert host["ss"] == 0.0 and host["max_e"] == 0.0
    load(dev, D)
    dup = dev.upgma(1)
    parent, length = capi.tree_from_upgma(dup["merge_x"], dup["merge_y"], dup["height"])
    got = dev.tree_fit(parent, length)
    assert got["n"] == n * (n - 1) // 2 and got["ss"] == 0.0 and got["max_e"] == 0.0 and got["explained"] == 1.0
    assert (got["taxon_ss"] == 0.0).all() and abs(got["cophenetic"] - 1.0) <= 2.0 ** -50
    assert_same_fit(got, host)


# ---- skipped pairs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_skipped_pairs(dev, which):
    from dipper_amd import capi
    n = 100
    name, D = _nonfinite.matrices(n, 11)[which]
    parent, length = R.balanced(n, np.random.default_rng(5))
    length = length.copy()
    length[7] = np.inf
    load(dev, D)
    got = dev.tree_fit(parent, length)
    assert_same_fit(got, capi.tree_fit_host(D, parent, length), name)
    ref = check_against_reference(D, parent, length, got)
    assert ref["skipped"] >= n - 1 and got["taxon_pairs"][7] == 0


def test_all_skipped_and_zero_distances(dev):
    from dipper_amd import capi
    n = 70
    parent, length = R.caterpillar(n, np.random.default_rng(6))
    D = np.full((n, n), np.nan)
    np.fill_diagonal(D, 0.0)
    load(dev, D)
    got = dev.tree_fit(parent, length)
    assert got["n"] == 0 and got["skipped"] == n * (n - 1) // 2 and tuple(got["worst"]) == (-1, -1)
    assert all(np.isnan(got[k]) for k in ("rms", "rms_rel", "explained", "cophenetic"))
    assert_same_fit(got, capi.tree_fit_host(D, parent, length))
    D = noisy(n).copy()
    D[3, 1] = D[1, 3] = 0.0
    D[69, 0] = D[0, 69] = 0.0
    load(dev, D)
    got = dev.tree_fit(parent, length)
    assert got["n"] == n * (n - 1) // 2 and got["n_w"] == got["n"] - 2      # D = 0 pairs are left out of WSS only
    assert_same_fit(got, capi.tree_fit_host(D, parent, length))


# ---- state, arguments, allocations ------------------------------------------------------------------------------------------------
def test_state_and_argument_errors(dev):
    import dipper_amd
    from dipper_amd import capi
    n = 64
    D = noisy(n)
    parent, length = trees(n)["balanced"]
    d = dipper_amd.Dipper(0)
    try:
        with pytest.raises(capi.DipperError) as ei:      # no matrix yet
            d.tree_fit(parent, length, n=n)
        assert ei.value.code == -3
        assert d.tree_patristic_rows(n, parent, length).shape == (n, n)      # needs none
    finally:
        d.close()
    load(dev, D)
    dev.nj_run(max_iters=1)
    with pytest.raises(capi.DipperError) as ei:
        dev.tree_fit(parent, length)
    assert ei.value.code == -3 and "the matrix is not fresh (1 NJ iterations since dpr_dist_matrix); build it again" in str(ei.value)
    dev.dist_matrix(capi.SRC_MATRIX)                     # a fresh matrix again
    p65, l65 = trees(65)["balanced"]
    with pytest.raises(capi.DipperError) as ei:          # n other than the matrix's
        dev.tree_fit(p65, l65, n=65)
    assert ei.value.code == -1 and "n differs" in str(ei.value)
    bad = parent.copy()
    bad[0] = 1
    with pytest.raises(capi.DipperError) as ei:
        dev.tree_fit(bad, length)
    assert ei.value.code == -1 and "not a tree" in str(ei.value)
    bad = parent.copy()
    bad[-1] = n
    with pytest.raises(capi.DipperError) as ei:
        dev.tree_fit(bad, length)
    assert ei.value.code == -1
    assert_same_fit(dev.tree_fit(parent, length), capi.tree_fit_host(D, parent, length))      # the context works afterwards
    nj = dev.nj_run()                                    # and the matrix is as it was
    ref = capi.nj_variant_host(0, D)
    assert np.array_equal(nj["merge_x"], ref["merge_x"]) and np.array_equal(nj["bl_x"], ref["bl_x"])


def test_virtual_ranks_and_shards_are_refused():
    import dipper_amd
    from dipper_amd import capi
    n = 200
    D = noisy(257)[:n, :n]
    parent, length = trees(n)["balanced"]
    nj = capi.nj_variant_host(0, D)
    d = dipper_amd.Dipper(0, virtual_world=2)
    try:
        load(d, D)
        with pytest.raises(capi.DipperError) as ei:
            d.tree_fit(parent, length, n=n)
        assert ei.value.code == -1
        res = d.nj_run()                             # the context is as usable as before
        assert np.array_equal(res["merge_x"], nj["merge_x"]) and np.array_equal(res["merge_y"], nj["merge_y"])
    finally:
        d.close()
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_virtual_shards(2)
        load(d, D)
        with pytest.raises(capi.DipperError) as ei:
            d.tree_fit(parent, length, n=n)
        assert ei.value.code == -1
        d.set_nj_virtual_shards(-1)
        load(d, D)
        assert_same_fit(d.tree_fit(parent, length), capi.tree_fit_host(D, parent, length))
    finally:
        d.close()


def test_two_calls_agree_and_the_second_allocates_nothing():
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        n = 257
        D = noisy(n)
        parent, length = trees(n)["nj"]
        load(d, D)
        first = d.tree_fit(parent, length)
        s1 = d.fit_stats()
        assert s1["allocations"] > 0 and s1["bytes"] > 0 and s1["levels"] == 9
        again = d.tree_fit(parent, length)
        s2 = d.fit_stats()
        assert_same_fit(again, first)
        assert s2 == s1
        small = noisy(65)                            # fewer tips: the same buffers
        load(d, small)
        p, ln = trees(65)["caterpillar"]
        assert_same_fit(d.tree_fit(p, ln), capi.tree_fit_host(small, p, ln))
        s3 = d.fit_stats()
        assert s3["allocations"] == s1["allocations"] and s3["bytes"] == s1["bytes"] and s3["levels"] == 7
        assert d.fit_timing()[0] > 0 and d.fit_timing()[1] == 0
        d.set_fit_compare(True)
        assert_same_fit(d.tree_fit(p, ln), capi.tree_fit_host(small, p, ln))
        assert d.fit_timing()[1] > 0 and d.fit_stats()["launches"] == 3
    finally:
        d.close()
