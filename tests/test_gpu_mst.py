"""GPU: the minimum spanning forest of the distances (dpr_mst_run, mst.hip) against the host Kruskal dpr_mst_host of the same matrix, as
bits: i, j and label equal, d equal viewed as uint64.  No tolerance anywhere.

A row of n columns is walked by one workgroup of 256 lanes (four wavefronts) in steps of 1 024 columns.  A lane loads pairs of
neighbouring columns (16 bytes of distances, 8 bytes of labels): in one step the pair at 2 lane and the pair 512 columns further on, so
a wavefront covers 128 consecutive columns of a load, a load 512 and a step 1 024; every step is a full one (there is no short first
step: the walk keeps no bound).  A lane keeps its own minimum, a wavefront reduces by shuffles, the four wavefronts meet in LDS.  The
rows live in a block whose row stride is n rounded up to 16 columns.  Which edge a size puts at the END of a row:

    n      edge
    2, 3   the smallest inputs: one candidate a row; two
    63     the first half of the first wavefront's lanes less one column; n odd: the last pair of columns is half outside the row
    64     ... exactly
    65     one column in lane 32
    127    the first wavefront of the first load less one column
    128    ... exactly (the second wavefront idle)
    129    one column in the second wavefront
    255, 256, 257   the same between the second and the third wavefront
    511    the first load less one column
    512    ... exactly: the second load idle
    513    one column in the second load
    1023   the first step less one column
    1024   ... exactly: the last column of the first step
    1025   one column in a second step (the first column of the next); n odd
    2049   one column in a third step

block_rows in {1, 7, 64, n - 1, n, n + 5, 0} must give one and the same answer."""
import functools

import numpy as np
import pytest

from tests import _aa_ref, _mst_ref as R, _nearest_ref, _pairs_ref, _util
from tests.conftest import dirty_device_memory

pytestmark = pytest.mark.gpu

EDGES = [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
NAMES = sorted(R.MATRICES)


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=256)
def host(name, n):
    """the host Kruskal of a named matrix, computed once and shared"""
    from dipper_amd import capi
    return capi.mst_host(R.matrix(name, n))


def check(got, ref, n):
    R.same(got, ref)
    s = R.summary(ref["label"])
    st = got["stats"]
    assert got["info"]["n"] == n and st["edges"] == len(ref["i"]) == n - s["components"]
    assert (st["components"], st["largest"], st["singletons"]) == (s["components"], s["largest"], s["singletons"])
    assert 1 <= st["rounds"] <= int(np.ceil(np.log2(n))) + 1 and st["rows_walked"] == st["rounds"] * n
    assert st["blocks"] == st["rounds"] * -(-n // got["info"]["block_rows"])


def run(gpu, name, n, block_rows=0):
    from dipper_amd import capi
    got = gpu.mst(capi.SRC_MATRIX, block_rows=block_rows)
    check(got, host(name, n), n)
    return got


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", NAMES)
def test_matrix_source_at_every_walk_edge(gpu, name, n):
    gpu.set_matrix_full(R.matrix(name, n))
    got = run(gpu, name, n)
    if name in ("constant", "chain"):
        i, j = R.closed_form(name, n)
        assert np.array_equal(got["i"], i) and np.array_equal(got["j"], j)
        assert got["stats"]["rounds"] == 1


@pytest.mark.parametrize("n", [1024, 1025])
def test_hierarchy_takes_the_rounds_of_the_numpy_boruvka(gpu, n):
    gpu.set_matrix_full(R.hierarchy(n))
    got = run(gpu, "hierarchy", n)
    ref, rounds = R.boruvka(R.hierarchy(n))
    R.same(got, ref)
    assert got["stats"]["rounds"] == rounds == 10


@pytest.mark.parametrize("name", ["noisy", "three_values", "negative"])
def test_rounds_equal_the_numpy_boruvka(gpu, name):
    n = 257
    gpu.set_matrix_full(R.matrix(name, n))
    got = run(gpu, name, n)
    ref, rounds = R.boruvka(R.matrix(name, n))
    R.same(got, ref)
    assert got["stats"]["rounds"] == rounds


def test_a_chain_is_joined_in_one_round(gpu):
    n = 2049
    gpu.set_matrix_full(R.chain(n))
    got = run(gpu, "chain", n, block_rows=100)
    assert got["stats"]["rounds"] == 1 and got["stats"]["blocks"] == 21 and (got["d"] == 1.0).all()


@pytest.mark.parametrize("n", [129, 1025])
def test_non_finite_entries_end_on_a_round_that_emits_nothing(gpu, n):
    D = R.nonfinite(n)
    gpu.set_matrix_full(D)
    got = run(gpu, "nonfinite", n)
    ref, rounds = R.boruvka(D)
    s = R.summary(ref["label"])
    assert s["components"] >= 3 and s["singletons"] >= 1 and got["label"][1] == 1
    assert got["stats"]["rounds"] == rounds      # the last of them found no edge: more than one component is left
    assert (got["stats"]["components"], got["stats"]["largest"], got["stats"]["singletons"]) == (s["components"], s["largest"], s["singletons"])


@pytest.mark.parametrize("n", [129, 1025])
@pytest.mark.parametrize("name", ["noisy", "nonfinite", "three_values", "hierarchy"])
def test_every_block_size_gives_the_same_answer(gpu, name, n):
    gpu.set_matrix_full(R.matrix(name, n))
    rounds = set()
    for rows in (1, 7, 64, n - 1, n, n + 5, 0):
        got = run(gpu, name, n, block_rows=rows)
        rounds.add(got["stats"]["rounds"])
        if rows:
            assert got["info"]["block_rows"] == min(rows, n)
            assert got["stats"]["blocks"] == got["stats"]["rounds"] * -(-n // min(rows, n))
    assert len(rounds) == 1


def test_signed_zeros_and_negative_entries(gpu):
    n = 257
    D = _nearest_ref.signed_zero(n)
    gpu.set_matrix_full(D)
    got = run(gpu, "signed_zero", n)
    neg = int((got["d"] < 0).sum())
    assert neg >= 1 and (got["d"][:neg] < 0).all() and (got["d"][neg:] >= 0).all()
    zero = got["d"] == 0
    assert zero.any() and np.signbit(got["d"][zero]).any() and (~np.signbit(got["d"][zero])).any()
    assert np.array_equal(np.signbit(got["d"]), np.signbit(D[got["i"], got["j"]]))


def test_padding_columns_are_never_candidates_in_poisoned_memory():
    """device memory full of 0x80 bytes (as fp64 a finite negative number: smaller than any entry; as a label a number no tip has)
    before the context's allocations.  n = 129 has 15 padding columns up to ld = 144: a padding column, a padding label or a place
    nobody wrote, read as a candidate, would give an edge nobody has"""
    import dipper_amd
    from dipper_amd import capi
    capi.load_library()
    dirty_device_memory(2 << 30, 0x80)
    d = dipper_amd.Dipper(0)
    try:
        for name, n in (("noisy", 129), ("nonfinite", 129), ("three_values", 1025), ("hierarchy", 1025)):
            d.set_matrix_full(R.matrix(name, n))
            for rows in (0, 7):
                check(d.mst(capi.SRC_MATRIX, block_rows=rows), host(name, n), n)
        src, k = upload(d, "nt")
        M = matrix_of(d, src, 2, k)
        check(d.mst(src, 2, k, block_rows=64), capi.mst_host(M), M.shape[0])
    finally:
        d.close()


# ---- computed sources: against the matrix the library returns for the same context ------------------------------------------------
@functools.lru_cache(maxsize=None)
def nucleotides():
    rng = np.random.default_rng(71)
    seqs = _util.synth_alignment(rng, n=130, L=600, mean_bl=0.02, lo=0.002, hi=0.1, invalid_frac=0.02)
    seqs[77] = seqs[12]      # duplicates: zeros off the diagonal, ties by (i, j)
    seqs[129] = seqs[0]
    seqs[5] = seqs[0].translate(bytes.maketrans(b"ACGT", b"CGTA"))      # every site differs from sequence 0: saturated under JC
    return seqs


@functools.lru_cache(maxsize=None)
def residues():
    rng = np.random.default_rng(73)
    seqs = [bytes(s) for s in _aa_ref.scatter(rng, [bytearray(s) for s in _aa_ref.evolve_yule(rng, 130, 300)], 0.02)]
    seqs[40] = seqs[3]
    return seqs


@functools.lru_cache(maxsize=None)
def reads():
    seqs = _util.synth_reads(np.random.default_rng(77), n=130, L=4000, mean_bl=0.01, lo=0.001, hi=0.05)
    seqs[90] = seqs[7]
    seqs[60] = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(79).integers(0, 4, 4000)])      # shares nothing with anybody
    return seqs


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


@pytest.mark.parametrize("kind,dist_type", [("nt", 2), ("nt", 9), ("aa", 8), ("mash", 0)])
def test_computed_sources_equal_the_matrix_of_the_same_context(gpu, kind, dist_type):
    """also where a row provider whose (i, j) and (j, i) bits differ would show: a component's edge is read from the row of whichever
    end lies in it"""
    from dipper_amd import capi
    src, k = upload(gpu, kind)
    M = matrix_of(gpu, src, dist_type, k)
    n = M.shape[0]
    assert n == 130 and np.array_equal(M, M.T, equal_nan=True)
    ref = capi.mst_host(M)
    for rows in (64, 0):
        check(gpu.mst(src, dist_type, k, block_rows=rows), ref, n)
    if kind == "nt" and dist_type == 2:
        assert not np.isfinite(M[5, 0]) and M[77, 12] == 0.0 and M[129, 0] == 0.0
        got = gpu.mst(src, dist_type, k)
        assert (got["i"][0], got["j"][0], got["d"][0]) == (77, 12, 0.0) and (got["i"][1], got["j"][1]) == (129, 0)


def test_two_runs_on_one_context_give_identical_results(gpu):
    src, k = upload(gpu, "nt")
    a = gpu.mst(src, 2, k, block_rows=7)
    b = gpu.mst(src, 2, k, block_rows=7)
    for key in ("i", "j", "d", "label"):
        assert a[key].tobytes() == b[key].tobytes()
    assert a["stats"] == b["stats"]


def test_open_streams_of_pairs_and_of_neighbours_still_deliver(gpu):
    from dipper_amd import capi
    n, T, K = 257, 0.3, 10
    D = _pairs_ref.noisy(n)
    gpu.set_matrix_full(D)
    want_pairs, want_near, want = capi.pairs_within_host(D, T), capi.nearest_host(D, K), capi.mst_host(D)
    gpu.pairs_begin(capi.SRC_MATRIX, threshold=T, block_rows=100)
    gpu.nearest_begin(capi.SRC_MATRIX, K=K, block_rows=100)
    pairs, near = [gpu.pairs_next()], [gpu.nearest_next(K)]
    check(gpu.mst(capi.SRC_MATRIX, block_rows=50), want, n)
    while pairs[-1][3] < n:
        pairs.append(gpu.pairs_next())
    while sum(len(p[2]) for p in near) < n:
        near.append(gpu.nearest_next(K))
    label = gpu.pairs_labels(n)
    gpu.pairs_end()
    gpu.nearest_end()
    assert np.array_equal(np.concatenate([p[0] for p in pairs]), want_pairs["i"]) and np.array_equal(np.concatenate([p[1] for p in pairs]), want_pairs["j"])
    assert np.array_equal(label, want_pairs["label"])
    _nearest_ref.same(dict(j=np.concatenate([p[0] for p in near]), d=np.concatenate([p[1] for p in near]), cnt=np.concatenate([p[2] for p in near])),
                      want_near)
    # cutting the forest at T gives the clusters of the pairs within T
    cut = R._Forest(n)
    for a, b in zip(want["i"][want["d"] <= T].tolist(), want["j"][want["d"] <= T].tolist()):
        cut.join(a, b)
    assert np.array_equal(cut.labels(), want_pairs["label"])


def test_peak_device_bytes_follow_the_block_not_the_matrix(gpu):
    """a condition on the design, not a measurement: the block of 16 full rows (16 x 1 040 x 8 bytes), 56 bytes a tip and the count"""
    n = 1025
    gpu.set_matrix_full(R.matrix("noisy", n))
    got = run(gpu, "noisy", n, block_rows=16)
    assert got["stats"]["blocks"] == got["stats"]["rounds"] * 65
    assert 0 < got["stats"]["peak_device_bytes"] <= 16 * 1040 * 8 + 56 * 1040 + 8


def test_errors(gpu):
    import dipper_amd
    from dipper_amd import capi
    gpu.set_matrix_full(R.matrix("noisy", 129))
    with pytest.raises(capi.DipperError) as ei:
        gpu.mst(capi.SRC_MATRIX, block_rows=-1)
    assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        gpu.mst(7)
    assert ei.value.code == -1
    n = 129
    i, j, d = np.full(n, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32), np.full(n, -5.0)
    label, E = np.full(n, -5, dtype=np.int32), np.full(1, -5, dtype=np.int64)
    pi, pj, pd, pe, pl = (a.ctypes.data_as(t) for a, t in ((i, capi.c_i32p), (j, capi.c_i32p), (d, capi.c_f64p), (E, capi.c_i64p), (label, capi.c_i32p)))
    for args in ((None, pj, pd, pe, pl), (pi, None, pd, pe, pl), (pi, pj, None, pe, pl), (pi, pj, pd, None, pl), (pi, pj, pd, pe, None)):
        assert gpu.L.dpr_mst_run(gpu.h, capi.SRC_MATRIX, 1, 15, 0, *args) == -1
    assert gpu.L.dpr_mst_run(gpu.h, capi.SRC_MATRIX, 1, 15, -3, pi, pj, pd, pe, pl) == -1
    assert (i == -5).all() and (j == -5).all() and (d == -5.0).all() and (label == -5).all() and E[0] == -5      # nothing was written
    d2 = dipper_amd.Dipper(0)
    try:
        for call in (d2.mst_stats, d2.mst_info):
            with pytest.raises(capi.DipperError) as ei:
                call()
            assert ei.value.code == -3
        for src in (capi.SRC_MSA, capi.SRC_MASH, capi.SRC_MATRIX):
            with pytest.raises(capi.DipperError) as ei:
                d2.mst(src)      # nothing uploaded
            assert ei.value.code == -3
    finally:
        d2.close()
