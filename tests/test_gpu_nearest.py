"""GPU: each sequence's K nearest neighbours (dpr_nearest_*, nearest.hip) against the host restatement dpr_nearest_host of the same
matrix, as bits: j and cnt equal, d equal viewed as uint64.  No tolerance anywhere.

A row of n columns is walked by one workgroup of 256 lanes (four wavefronts).  A lane loads pairs of neighbouring columns: in one step
the pair at 2 lane and the pair 512 columns further on, so a wavefront covers 128 consecutive columns of a load and a step 1 024.  The
FIRST step of a row is short, 256 columns (lanes 0 .. 127, the first load only), and is followed at once by a selection that yields the
bound; full steps begin at columns 256, 1 280, 2 304, 3 328.  Candidates are held in a buffer of 1 536 places in LDS; at the start of
a step with max(2 K, 128) or more of them held -- never more than 512, so that a step always fits -- the buffer is cut back to its K
best and the bound tightened.  Which edge a size puts at the END of a row:

    n      edge
    2, 3   the smallest inputs: one candidate a row; two
    K, K + 1, K + 2   a row holds K - 1, exactly K, K + 1 candidates (K = 10, 64, 256)
    127    the first wavefront of the first step less one column
    128    ... exactly (the second wavefront idle)
    129    one column in the second wavefront; n odd: the last pair of columns is half outside the row
    255    the first step less one column
    256    the first step exactly: no full step
    257    one column in the first full step
    767    the first load of the first full step (columns 256 .. 767) less one column
    769    one column in its second load
    1279   the first full step less one column
    1280   ... exactly
    1281   one column in a second full step
    2305   two full steps and one column: both parities of the per-step counts used twice

n = 3 329 (one column in a fourth full step) is where a `descending` row -- every later column beats the bound, so every column is a
survivor -- has cut its buffer back four times before the row ends: once after the first step (256 held, the bound), then before the
second, third and fourth full step (K + 1 024 held each time, of a capacity of 1 536): three cuts of a buffer two thirds full or more.

block_rows in {1, 7, 64, n - 1, n, n + 5, 0} must give one and the same answer."""
import functools

import numpy as np
import pytest

from tests import _aa_ref, _nearest_ref as R, _pairs_ref, _util
from tests.conftest import dirty_device_memory

pytestmark = pytest.mark.gpu

EDGES = [2, 3, 127, 128, 129, 255, 256, 257, 767, 769, 1279, 1280, 1281, 2305]
KS = [1, 2, 10, 64, 256]
NAMES = sorted(R.MATRICES)
FLUSH_N = 3329


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=256)
def host(name, n, K):
    """the host restatement of a named matrix, computed once and shared"""
    from dipper_amd import capi
    return capi.nearest_host(R.matrix(name, n, K), K)


def check(got, ref, n, K):
    R.same(got, ref)
    assert got["info"]["n"] == n and got["stats"]["blocks"] >= 1
    assert got["stats"]["neighbours"] == int(ref["cnt"].sum())
    assert got["stats"]["fewer"] == int((ref["cnt"] < K).sum()) and got["stats"]["none"] == int((ref["cnt"] == 0).sum())


def run(gpu, name, n, K, block_rows=0):
    from dipper_amd import capi
    got = gpu.nearest(capi.SRC_MATRIX, K=K, block_rows=block_rows)
    check(got, host(name, n, K), n, K)
    return got


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", NAMES)
def test_matrix_source_at_every_walk_edge(gpu, name, n):
    if name != "nonfinite":
        gpu.set_matrix_full(R.matrix(name, n))
    for K in KS:
        if name == "nonfinite":      # (rows with exactly K - 1 and K finite entries: the matrix depends on K)
            gpu.set_matrix_full(R.matrix(name, n, K))
        got = run(gpu, name, n, K)
        if name == "constant":
            # rows 0 and n - 1: the self column first and last; the index tie-break across lanes, waves and steps
            assert got["j"][0, : min(K, n - 1)].tolist() == list(range(1, min(K, n - 1) + 1))
            assert got["j"][n - 1, : min(K, n - 1)].tolist() == list(range(min(K, n - 1)))


@pytest.mark.parametrize("K", [10, 64, 256])
def test_rows_of_k_minus_one_k_and_k_plus_one_candidates(gpu, K):
    for n in (K, K + 1, K + 2):
        for name in NAMES:
            gpu.set_matrix_full(R.matrix(name, n, K))
            got = run(gpu, name, n, K)
            if name in ("noisy", "constant", "descending", "ascending"):
                assert (got["cnt"] == min(K, n - 1)).all()


@pytest.mark.parametrize("n", [129, 1281])
@pytest.mark.parametrize("name", ["noisy", "nonfinite", "three_values"])
def test_every_block_size_gives_the_same_answer(gpu, name, n):
    K = 10
    gpu.set_matrix_full(R.matrix(name, n, K))
    for rows in (1, 7, 64, n - 1, n, n + 5, 0):
        got = run(gpu, name, n, K, block_rows=rows)
        if rows:
            assert got["info"]["block_rows"] == min(rows, n) and got["stats"]["blocks"] == -(-n // min(rows, n))


@pytest.mark.parametrize("K", [10, 256])
def test_a_descending_row_cuts_a_full_buffer_back_three_times(gpu, K):
    n = FLUSH_N
    gpu.set_matrix_full(R.descending(n))
    got = run(gpu, "descending", n, K)
    # per row: the cut that yields the bound (not in a row whose first step holds 255 < K = 256 candidates) and three of K + 1 024 held
    assert got["stats"]["flushes"] >= 3 * n, got["stats"]
    assert got["j"][0, :3].tolist() == [n - 1, n - 2, n - 3] and got["j"][n - 1, :3].tolist() == [n - 2, n - 3, n - 4]


def test_an_ascending_row_keeps_nothing_behind_its_first_step(gpu):
    n, K = 1281, 10
    gpu.set_matrix_full(R.ascending(n))
    got = run(gpu, "ascending", n, K)
    assert got["stats"]["flushes"] == n, got["stats"]      # the one cut that yields the bound; nothing survives afterwards
    assert got["j"][5].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]


def test_signed_zeros_and_negative_entries(gpu):
    n, K = 257, 64
    D = R.signed_zero(n)
    gpu.set_matrix_full(D)
    got = run(gpu, "signed_zero", n, K)
    row, cols = got["d"][0], got["j"][0]
    neg = int((D[0] < 0).sum())
    assert neg >= 1 and (row[:neg] < 0).all() and (row[neg:] >= 0).all()
    zeros = cols[row == 0]
    assert {1, 2, n - 1} <= set(zeros.tolist()) and (np.diff(zeros) > 0).all()
    sign = {int(c): bool(np.signbit(v)) for c, v in zip(cols, row)}
    assert sign[1] is False and sign[2] is True and sign[n - 1] is True


def test_rows_without_a_finite_entry_are_padded(gpu):
    n, K = 129, 10
    gpu.set_matrix_full(R.nonfinite(n, K))
    got = run(gpu, "nonfinite", n, K)
    assert got["cnt"][1] == 0 and (got["j"][1] == -1).all() and (got["d"][1].view(np.uint64) == R.PAD_BITS).all()
    assert got["cnt"][2] == K - 1 and got["cnt"][3] == K and got["stats"]["none"] >= 1 and got["stats"]["fewer"] >= 2


def test_padding_columns_are_never_candidates_in_poisoned_memory():
    """device memory full of 0x80 bytes (as fp64 a finite negative number: nearer than any entry) before the context's allocations.
    n = 129 has 15 padding columns up to ld = 144 and K = 256 takes every candidate there is: a padding column or a place nobody wrote,
    read as a candidate, would lead a row"""
    import dipper_amd
    from dipper_amd import capi
    capi.load_library()
    dirty_device_memory(2 << 30, 0x80)
    d = dipper_amd.Dipper(0)
    try:
        for name, n, K in (("noisy", 129, 256), ("nonfinite", 129, 10), ("three_values", 1281, 256)):
            d.set_matrix_full(R.matrix(name, n, K))
            for rows in (0, 7):
                check(d.nearest(capi.SRC_MATRIX, K=K, block_rows=rows), host(name, n, K), n, K)
        src, k = upload(d, "nt")
        M = matrix_of(d, src, 2, k)
        check(d.nearest(src, 2, k, K=256, block_rows=64), capi.nearest_host(M, 256), M.shape[0], 256)
    finally:
        d.close()


# ---- computed sources: against the matrix the library returns for the same context ------------------------------------------------
@functools.lru_cache(maxsize=None)
def nucleotides():
    rng = np.random.default_rng(61)
    seqs = _util.synth_alignment(rng, n=130, L=600, mean_bl=0.02, lo=0.002, hi=0.1, invalid_frac=0.02)
    seqs[77] = seqs[12]      # duplicates: zeros off the diagonal, ties by column
    seqs[129] = seqs[0]
    return seqs


@functools.lru_cache(maxsize=None)
def residues():
    rng = np.random.default_rng(63)
    return [bytes(s) for s in _aa_ref.scatter(rng, [bytearray(s) for s in _aa_ref.evolve_yule(rng, 130, 300)], 0.02)]


@functools.lru_cache(maxsize=None)
def reads():
    return _util.synth_reads(np.random.default_rng(67), n=130, L=4000, mean_bl=0.01, lo=0.001, hi=0.05)


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


def matrix_of(d, src, dist_type, k):
    d.dist_matrix(src, dist_type, k)
    return d.matrix()


@pytest.mark.parametrize("kind,dist_type", [("nt", 1), ("nt", 2), ("nt", 9), ("aa", 8), ("mash", 0)])
def test_computed_sources_equal_the_matrix_of_the_same_context(gpu, kind, dist_type):
    """also where a row provider whose (i, j) and (j, i) bits differ would show: the block holds both, the matrix one of them mirrored"""
    from dipper_amd import capi
    src, k = upload(gpu, kind)
    M = matrix_of(gpu, src, dist_type, k)
    n, K = M.shape[0], 10
    assert n == 130 and np.array_equal(M, M.T, equal_nan=True)
    ref = capi.nearest_host(M, K)
    for rows in (64, 0):
        check(gpu.nearest(src, dist_type, k, K=K, block_rows=rows), ref, n, K)
    if kind == "nt" and dist_type == 2:
        got = gpu.nearest(src, dist_type, k, K=K)
        assert got["j"][77, 0] == 12 and got["j"][12, 0] == 77 and got["j"][129, 0] == 0 and got["d"][129, 0] == 0.0


def test_two_streams_in_a_row_give_identical_results(gpu):
    src, k = upload(gpu, "nt")
    a = gpu.nearest(src, 2, k, K=10, block_rows=7)
    b = gpu.nearest(src, 2, k, K=10, block_rows=7)
    for key in ("j", "d", "cnt"):
        assert a[key].tobytes() == b[key].tobytes()
    assert a["stats"] == b["stats"]


def test_a_stream_of_pairs_is_independent_of_a_stream_of_neighbours(gpu):
    """pairs before and after neighbours on one context, and a stream of pairs left open across a whole stream of neighbours"""
    from dipper_amd import capi
    n, T, K = 257, 0.3, 10
    D = _pairs_ref.noisy(n)
    gpu.set_matrix_full(D)
    want_pairs, want_near = capi.pairs_within_host(D, T), capi.nearest_host(D, K)
    _pairs_ref.same(gpu.pairs_within(capi.SRC_MATRIX, threshold=T, block_rows=16), want_pairs)
    R.same(gpu.nearest(capi.SRC_MATRIX, K=K, block_rows=16), want_near)
    _pairs_ref.same(gpu.pairs_within(capi.SRC_MATRIX, threshold=T, block_rows=16), want_pairs)
    gpu.pairs_begin(capi.SRC_MATRIX, threshold=T, block_rows=100)
    parts = [gpu.pairs_next()]
    R.same(gpu.nearest(capi.SRC_MATRIX, K=K, block_rows=50), want_near)
    while parts[-1][3] < n:
        parts.append(gpu.pairs_next())
    label = gpu.pairs_labels(n)
    gpu.pairs_end()
    assert np.array_equal(np.concatenate([p[0] for p in parts]), want_pairs["i"]) and np.array_equal(np.concatenate([p[1] for p in parts]), want_pairs["j"])
    assert np.array_equal(np.concatenate([p[2] for p in parts]).view(np.uint64), want_pairs["d"].view(np.uint64)) and np.array_equal(label, want_pairs["label"])


def test_peak_device_bytes_follow_the_block_not_the_matrix(gpu):
    """a condition on the design, not a measurement: the block of 16 full rows (16 x 1 296 x 8 bytes), 16 x K places of 12 bytes and
    two counts a row"""
    from dipper_amd import capi
    n, K = 1281, 10
    gpu.set_matrix_full(R.noisy(n))
    got = run(gpu, "noisy", n, K, block_rows=16)
    assert got["stats"]["blocks"] == 81 and 0 < got["stats"]["peak_device_bytes"] <= 16 * 1296 * 8 + 16 * K * 12 + 16 * 8


def test_errors(gpu):
    import dipper_amd
    from dipper_amd import capi
    gpu.set_matrix_full(R.noisy(129))
    for K in (0, 257, -4):
        with pytest.raises(capi.DipperError) as ei:
            gpu.nearest_begin(capi.SRC_MATRIX, K=K)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        gpu.nearest_begin(capi.SRC_MATRIX, K=3, block_rows=-1)
    assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        gpu.nearest_begin(7, K=3)
    assert ei.value.code == -1
    gpu.nearest_end()
    for call in (lambda: gpu.nearest_next(3), gpu.nearest_stats, gpu.nearest_info):
        with pytest.raises(capi.DipperError) as ei:
            call()
        assert ei.value.code == -3
    d = dipper_amd.Dipper(0)
    try:
        for src in (capi.SRC_MSA, capi.SRC_MASH, capi.SRC_MATRIX):
            with pytest.raises(capi.DipperError) as ei:
                d.nearest_begin(src, K=3)      # nothing uploaded
            assert ei.value.code == -3
    finally:
        d.close()
    # the end of the stream is said again by every later call
    gpu.nearest_begin(capi.SRC_MATRIX, K=3, block_rows=100)
    seen = [(len(c), r0) for _, _, c, r0 in (gpu.nearest_next(3) for _ in range(4))]
    assert seen == [(100, 0), (29, 100), (0, 129), (0, 129)]
    gpu.nearest_end()
    gpu.nearest_end()      # without a stream: nothing to do
