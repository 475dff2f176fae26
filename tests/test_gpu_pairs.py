"""GPU: the pairs within a distance threshold and their clusters (dpr_pairs_*, pairs.hip) against the host restatement
dpr_pairs_within_host, as bits: i, j, d viewed as uint64, label, and the counts of stats.  No tolerance anywhere.

A row is walked by one workgroup of 256 lanes in steps of 512 columns, two sub-steps of 256 (four wavefronts of 64) each.  Row i has i
entries, so a matrix of n tips has rows of every length below n; which edge a size puts at the END of the longest rows:

    n      edge
    2, 3   the smallest inputs: one pair; a row of one and a row of two entries
    63     the longest row fills one wavefront less two lanes
    64     ... less one lane (row 63 has 63 entries)
    65     row 64 fills one wavefront exactly
    255    the first sub-step less two lanes, all four wavefronts of it in use
    256    ... less one lane
    257    row 256 fills the first sub-step exactly: the second sub-step of the step stays empty
    511    one step less two entries
    512    one step less one entry
    513    row 512 fills one step exactly (both parities of the per-step counts are used from n = 514 on)
    514    row 513 runs into a second step by one entry
    1025   two steps; row 1024 fills them exactly
    1026   two steps and one entry

block_rows in {1, 7, 64, n - 1, n, n + 5} and 0 (the library's choice) must give one and the same stream: 1 makes every row a block
(n blocks, the scan over one count), 7 and 64 leave a partial last block at most sizes, n - 1 leaves a last block of one row, n + 5 is
clamped.  Thresholds: one equal to an entry of the matrix (so `<=` and `<` differ), one below every entry (nothing kept: every count
0), DBL_MAX (every finite pair kept: a row's count is its length, the offsets and the pair buffers at their largest)."""
import functools

import numpy as np
import pytest

from tests import _aa_ref, _pairs_ref as R, _util

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 514, 1025, 1026]


def block_rows_of(n):
    return sorted({1, 7, 64, max(n - 1, 1), n, n + 5})


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def host(name, n, T):
    """the host restatement of a named matrix at T, computed once and shared"""
    from dipper_amd import capi
    return capi.pairs_within_host(matrix(name, n), T)


@functools.lru_cache(maxsize=None)
def matrix(name, n):
    if name == "nonfinite":
        return R.nonfinite(n)
    if name == "noisy":
        return R.noisy(n)
    return R.shapes(n)[name][0]


def thresholds(D):
    n = D.shape[0]
    vals = D[np.tril_indices(n, -1)]
    finite = np.sort(vals[np.isfinite(vals)])
    entry = float(finite[len(finite) // 10]) if len(finite) else 0.5
    return (entry, 0.001, R.DBL_MAX)


def check(got, ref, n):
    R.same(got, ref)
    assert got["stats"]["blocks"] >= 1 and got["info"]["n"] == n


@pytest.mark.parametrize("n", SIZES)
def test_matrix_source_with_nonfinite_entries_at_every_block_size(gpu, n):
    from dipper_amd import capi
    D = matrix("nonfinite", n)
    gpu.set_matrix_full(D)
    for T in thresholds(D):
        ref = host("nonfinite", n, T)
        if T == 0.001:
            assert ref["stats"]["pairs"] == int(np.isneginf(D[np.tril_indices(n, -1)]).sum())      # nothing but the -inf entries
        auto = gpu.pairs_within(capi.SRC_MATRIX, threshold=T, block_rows=0)
        check(auto, ref, n)
        for rows in block_rows_of(n):
            got = gpu.pairs_within(capi.SRC_MATRIX, threshold=T, block_rows=rows)
            check(got, ref, n)
            assert got["info"]["block_rows"] == min(rows, n) and got["stats"]["blocks"] == -(-n // min(rows, n))


@pytest.mark.parametrize("n", [3, 65, 257, 513, 1026])
def test_dense_and_empty_streams(gpu, n):
    """DBL_MAX on a matrix without non-finite entries: row i keeps all i entries; a threshold below every entry: header only"""
    from dipper_amd import capi
    D = matrix("noisy", n)
    gpu.set_matrix_full(D)
    for rows in (0, 7, 64):
        dense = gpu.pairs_within(capi.SRC_MATRIX, threshold=R.DBL_MAX, block_rows=rows)
        check(dense, host("noisy", n, R.DBL_MAX), n)
        ii, jj = np.tril_indices(n, -1)
        assert np.array_equal(dense["i"], ii) and np.array_equal(dense["j"], jj) and dense["stats"]["components"] == 1
        none = gpu.pairs_within(capi.SRC_MATRIX, threshold=0.01, block_rows=rows)
        check(none, host("noisy", n, 0.01), n)
        assert none["stats"]["pairs"] == 0 and none["stats"]["singletons"] == n and np.array_equal(none["label"], np.arange(n))


@pytest.mark.parametrize("n", [6, 65, 514, 1026])
@pytest.mark.parametrize("shape", ["path", "star", "cliques", "singletons"])
def test_component_shapes(gpu, shape, n):
    """labels are the smallest index of each component whatever the order of the hooks: a path under a random relabelling (chains
    of parents across blocks), a star, two cliques joined by one pair of the last row, no pair at all"""
    from dipper_amd import capi
    D, T = R.shapes(n)[shape]
    gpu.set_matrix_full(D)
    ref = host(shape, n, T)
    assert ref["stats"]["components"] == (n if shape == "singletons" else 1)
    for rows in (0, 1, 7, n - 1):
        got = gpu.pairs_within(capi.SRC_MATRIX, threshold=T, block_rows=rows)
        check(got, ref, n)
        comp = {}
        for v, r in enumerate(got["label"].tolist()):
            comp.setdefault(r, []).append(v)
        assert all(min(m) == r for r, m in comp.items())


# ---- computed sources: the expected matrix from dist_matrix + get_matrix_row on a second context --------------------------------
@functools.lru_cache(maxsize=None)
def nucleotides():
    rng = np.random.default_rng(41)
    seqs = _util.synth_alignment(rng, n=130, L=600, mean_bl=0.02, lo=0.002, hi=0.1, invalid_frac=0.02)
    seqs[77] = seqs[12]      # duplicates: zeros off the diagonal
    seqs[129] = seqs[0]
    return seqs


@functools.lru_cache(maxsize=None)
def residues():
    rng = np.random.default_rng(43)
    return [bytes(s) for s in _aa_ref.scatter(rng, [bytearray(s) for s in _aa_ref.evolve_yule(rng, 67, 300)], 0.02)]


@functools.lru_cache(maxsize=None)
def reads():
    return _util.synth_reads(np.random.default_rng(47), n=70, L=4000, mean_bl=0.01, lo=0.001, hi=0.05)


def upload(d, kind):
    from dipper_amd import capi
    if kind == "aa":
        d.set_msa_aa(capi.pack_aa_many(residues()))
        return capi.SRC_MSA, 15
    if kind == "mash":
        d.set_reads(reads())
        d.sketch(k=13, S=400, fetch=False)
        return capi.SRC_MASH, 13
    seqs = nucleotides()
    d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
    return capi.SRC_MSA, 15


_EXPECTED = {}


def expected(kind, dist_type):
    """the matrix of a second context, and the host restatement's answer at a threshold equal to one of its entries"""
    import dipper_amd
    from dipper_amd import capi
    key = (kind, dist_type)
    if key not in _EXPECTED:
        d2 = dipper_amd.Dipper(0)
        try:
            src, k = upload(d2, kind)
            d2.dist_matrix(src, dist_type, k)
            M = d2.matrix()
        finally:
            d2.close()
        vals = M[np.tril_indices(M.shape[0], -1)]
        finite = np.sort(vals[np.isfinite(vals)])
        T = float(finite[len(finite) // 8])
        M.setflags(write=False)
        _EXPECTED[key] = (M, T, capi.pairs_within_host(M, T), capi.pairs_within_host(M, R.DBL_MAX))
    return _EXPECTED[key]


@pytest.mark.parametrize("kind,dist_type", [("nt", 2), ("nt", 4), ("nt", 9), ("aa", 8), ("mash", 0)])
def test_computed_sources_equal_the_matrix(gpu, kind, dist_type):
    M, T, ref, ref_all = expected(kind, dist_type)
    n = M.shape[0]
    src, k = upload(gpu, kind)
    assert ref["stats"]["pairs"] >= n // 8 and (ref["d"] == T).any()
    for rows in [0] + block_rows_of(n):
        check(gpu.pairs_within(src, dist_type, k, threshold=T, block_rows=rows), ref, n)
    for rows in (0, 7):
        check(gpu.pairs_within(src, dist_type, k, threshold=R.DBL_MAX, block_rows=rows), ref_all, n)
    if kind == "nt" and dist_type == 2:
        zero = gpu.pairs_within(src, dist_type, k, threshold=0.0)
        assert {(77, 12), (129, 0)} <= set(zip(zero["i"].tolist(), zero["j"].tolist())) and zero["label"][77] == 12 and zero["label"][129] == 0


def test_two_runs_on_one_context_give_identical_bytes(gpu):
    M, T, ref, _ = expected("nt", 2)
    src, k = upload(gpu, "nt")
    a = gpu.pairs_within(src, 2, k, threshold=T, block_rows=7)
    b = gpu.pairs_within(src, 2, k, threshold=T, block_rows=7)
    for key in ("i", "j", "d", "label"):
        assert a[key].tobytes() == b[key].tobytes()
    assert {k2: v for k2, v in a["stats"].items()} == {k2: v for k2, v in b["stats"].items()}


@pytest.mark.parametrize("kind", ["matrix", "nt"])
def test_the_context_is_left_intact(kind):
    """a dist_matrix + nj_run after a stream of pairs gives the merge log of a fresh context"""
    import dipper_amd
    from dipper_amd import capi
    logs = []
    for with_pairs in (True, False):
        d = dipper_amd.Dipper(0)
        try:
            if kind == "matrix":
                D = matrix("noisy", 257)
                d.set_matrix_full(D)
                src, dt, k = capi.SRC_MATRIX, 1, 15
            else:
                src, k = upload(d, "nt")
                dt = 2
            if with_pairs:
                got = d.pairs_within(src, dt, k, threshold=0.3, block_rows=7)
                assert got["stats"]["pairs"] > 0
            d.dist_matrix(src, dt, k)
            logs.append(d.nj_run())
        finally:
            d.close()
    for key in ("merge_x", "merge_y", "bl_x", "bl_y"):
        assert logs[0][key].tobytes() == logs[1][key].tobytes(), key
    assert logs[0]["iters"] == logs[1]["iters"]


def test_a_stream_between_matrix_and_nj_leaves_the_matrix(gpu):
    from dipper_amd import capi
    D = matrix("noisy", 65)
    gpu.set_matrix_full(D)
    gpu.dist_matrix(capi.SRC_MATRIX)
    before = gpu.matrix()
    gpu.pairs_within(capi.SRC_MATRIX, threshold=0.5)
    assert gpu.matrix().tobytes() == before.tobytes()


def test_peak_device_bytes_follow_the_block_not_the_matrix(gpu):
    """a condition on the design, not a measurement: at n = 1 025 and block_rows = 16 the block (16 x 1 040 x 8 bytes), the pair
    buffers at their largest (16 x 1 024 x 16), the counts and 2 x 4 n bytes of parents and labels stay below a quarter of 8 n^2"""
    from dipper_amd import capi
    rng = np.random.default_rng(53)
    n = 1025
    seqs = _util.synth_alignment(rng, n=n, L=96, mean_bl=0.02, lo=0.002, hi=0.1)
    gpu.set_msa(capi.pack4_many(seqs), 96)
    for T in (0.05, R.DBL_MAX):
        got = gpu.pairs_within(capi.SRC_MSA, 2, threshold=T, block_rows=16)
        assert got["stats"]["blocks"] == 65 and 0 < got["stats"]["peak_device_bytes"] < 8 * n * n // 4, got["stats"]
    assert got["stats"]["peak_device_bytes"] <= 16 * 1040 * 8 + 16 * 1024 * 16 + 8 * 17 + 2 * 4 * n


def test_errors(gpu):
    import dipper_amd
    from dipper_amd import capi
    gpu.set_matrix_full(matrix("noisy", 65))
    for T in (float("nan"), -0.1, float("inf")):
        with pytest.raises(capi.DipperError) as ei:
            gpu.pairs_begin(capi.SRC_MATRIX, threshold=T)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        gpu.pairs_begin(capi.SRC_MATRIX, threshold=0.1, block_rows=-1)
    assert ei.value.code == -1
    gpu.pairs_end()
    with pytest.raises(capi.DipperError) as ei:
        gpu.pairs_next()
    assert ei.value.code == -3
    gpu.pairs_begin(capi.SRC_MATRIX, threshold=0.3, block_rows=16)
    gpu.pairs_next()
    with pytest.raises(capi.DipperError) as ei:
        gpu.pairs_labels(65)      # rows_done is 16
    assert ei.value.code == -3
    gpu.pairs_end()
    d = dipper_amd.Dipper(0)
    try:
        for src in (capi.SRC_MSA, capi.SRC_MASH, capi.SRC_MATRIX):
            with pytest.raises(capi.DipperError) as ei:
                d.pairs_begin(src, threshold=0.1)      # nothing uploaded
            assert ei.value.code == -3
    finally:
        d.close()
    # the end of the stream is said again by every later call
    gpu.pairs_begin(capi.SRC_MATRIX, threshold=0.3, block_rows=64)
    seen = [gpu.pairs_next()[3] for _ in range(4)]
    assert seen == [64, 65, 65, 65] and len(gpu.pairs_next()[0]) == 0
    gpu.pairs_end()
