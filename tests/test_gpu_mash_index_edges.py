"""The Mash inverted-index kernel (mash_dist_index_kernel, dipper_amd/csrc/mash_index.hip) at the edges of its own constants: the
chunk of C tips, the dense threshold Dm, the list lengths of the sparse path, sketches of the largest size, the bounded grid of
a batch beside the tree kernels, and every output form (mirrored matrix, placement rows, transposed block, row shards) over more
than one chunk.  C and Dm come from Dipper.mash_index_info(), so a change of the constants moves these tests with it; the inputs
and the conditions that place them on the edges are tests/_mash_inputs.py (shown on the oracle alone in tests/test_mash_inputs.py)
and are asserted again here on the device's sketches.  Reference: the oracle's literal merge (orc_mash_dist_row), rtol = 1e-12.

What a one-line slip in mash_index.hip does here (the last three were also built and run: 14, 14 and 8 of the 20 tests fail):
  * `ent >> 17` -> `>> 16` in mi_dense_fill_kernel: tip t's position lands in slot 2 t of the dense block, odd slots stay "absent":
    every value of Dm .. C entries loses its odd tips -- test_dense_threshold_and_list_lengths, all rows;
  * counters not zeroed per task: a workgroup of the bounded grid starts its second task on the counts of the first --
    test_placement_batches_and_the_bounded_grid (trace against the oracle on the matrix of the unbounded grid, and against the
    context that produces every batch alone);
  * memset byte 0x7f -> 0xff: an absent tip's position reads -1 and passes the sign test, every dense value counts for tips that do
    not hold it -- test_dense_threshold_and_list_lengths and 13 others;
  * value B before value A in the fused update: the value at a pair's cut-off (position_A + position_B - count = S exactly) sees
    the count without its predecessor's copies -- test_largest_sketches (sketches full, thousands of dense values, multiplicities
    up to 2 110) and 12 others;
  * `>= kIDenseMin` -> `>`: the lists of exactly Dm entries stay sparse (same distances): info["dense"] falls short of the host's
    count in test_chunk_edges, test_dense_threshold_and_list_lengths (e.g. 88 against 111 at 2 C tips)."""
import ctypes as C_

import numpy as np
import pytest

from tests import _jplace, _mash_inputs as mi
from tests.test_gpu_dc import _same_dc_state
from tests.test_gpu_mash_place import _reads, _same_state
from tests.test_gpu_place_fixed import same as same_triples

pytestmark = pytest.mark.gpu

BATCH = 1024           # rows per placement batch of Mash input (PlacePolicy::batch_rows)
INFO_KEYS = ("built", "chunk_tips", "chunks", "distinct", "dense", "dense_min", "max_sketch", "beside_task_bound")


@pytest.fixture(scope="module")
def consts():
    """the kernel's constants, from a context that has sketched two reads"""
    import dipper_amd
    d = dipper_amd.Dipper(0)
    try:
        d.set_reads([b"ACGTTGCAAC" * 4, b"TTGACCAGTA" * 4])
        d.sketch(k=8, S=16, fetch=False)
        info = d.mash_index_info()
    finally:
        d.close()
    assert tuple(info) == INFO_KEYS
    assert info["chunk_tips"] >= 128 and info["chunk_tips"] % 128 == 0 and 1 < info["dense_min"] < info["chunk_tips"]
    return info


def _sizes(n, C):
    return [C] * (n // C) + ([n % C] if n % C else [])


def _index_context(monkeypatch, kernel="index", virtual_world=0):
    import dipper_amd
    monkeypatch.setenv("DPR_MASH_KERNEL", kernel)      # (read at every sketch / distance call)
    d = dipper_amd.Dipper(0, virtual_world=virtual_world)
    d.set_nj_mode(0)                                   # the plain slot-space matrix
    return d


def _matrix(d, k):
    from dipper_amd import capi
    d.dist_matrix(capi.SRC_MASH, 0, k)
    M = d.matrix()
    assert np.array_equal(M, M.T) and np.all(np.diag(M) == 0)
    return M


def _assert_info(info, consts, sk, built=1):
    C, Dm = consts["chunk_tips"], consts["dense_min"]
    tables = mi.chunk_tables(sk, C)
    distinct, dense = mi.index_counts(tables, Dm)
    assert info["built"] == built
    assert info["chunks"] == -(-len(sk) // C) == len(tables)
    assert info["distinct"] == distinct
    assert info["dense"] == dense
    for key in ("chunk_tips", "dense_min", "max_sketch", "beside_task_bound"):
        assert info[key] == consts[key]
    return tables


@pytest.mark.parametrize("chunks,extra,S,k", [(1, -1, 256, 15), (1, 0, 256, 15), (1, 1, 256, 15), (2, -1, 256, 15), (2, 0, 256, 15),
                                              (2, 1, 256, 15), (1, 1, 1, 2), (1.5, 1, 33, 5)],
                         ids=["C-1", "C", "C+1", "2C-1", "2C", "2C+1", "C+1,S=1", "C+C/2+1"])
def test_chunk_edges(orc, monkeypatch, consts, chunks, extra, S, k):
    """One tip short of a chunk, exactly one, one over, and the same around two chunks: the WHOLE matrix against the oracle, and the
    index reports the chunks, the distinct (chunk, value) pairs and the dense ones that the sketches give on the host.  C + 1 tips
    with sketches of one value of k = 2 (every sketch value is shared by hundreds of tips); C + C/2 + 1 tips: the chunk sort's top-level
    merge has a right run of one tip."""
    C, Dm = consts["chunk_tips"], consts["dense_min"]
    n = int(chunks * C) + extra
    rng = np.random.default_rng(1000 * n + S)
    seqs = mi.marker_reads(rng, _sizes(n, C), k, mi.list_length_edges(C, Dm))
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        sk = d.sketch(k=k, S=S)
        info = d.mash_index_info()
        M = _matrix(d, k)
        assert d.mash_index_info() == info
    finally:
        d.close()
    _assert_info(info, consts, sk)
    assert np.array_equal(sk[[0, n // 2, n - 1]], mi.oracle_sketches(orc, [seqs[0], seqs[n // 2], seqs[n - 1]], k, S))
    mi.assert_rows(M, mi.oracle_rows(orc, sk, k, range(1, n)))


def test_dense_threshold_and_list_lengths(orc, monkeypatch, consts):
    """Two full chunks + 7 tips of marker reads, every k-mer in its sketch: posting lists of exactly 1, 2, 63 .. 65, 127 .. 129, 191 ..
    193, 255 .. 257, 319 .. 321, Dm - 1, Dm, Dm + 1, 600 and C entries in both full chunks (the preloaded group, whole groups of 192, one
    to three partial groups, the last sparse and the first dense length), the padding value in every tip with tens to hundreds of
    copies at differing first positions, every pairing of dense and sparse values in the two-values-per-step loop -- all rows
    against the oracle.  A tip index read from the wrong bits of a posting, an absent tip that passes the dense path's sign test, or a
    threshold off by one changes a distance or the reported dense count here."""
    C, Dm = consts["chunk_tips"], consts["dense_min"]
    n, S, k = 2 * C + 7, 512, 15
    seqs = mi.marker_reads(np.random.default_rng(2055), [C, C, 7], k, mi.list_length_edges(C, Dm))
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        sk = d.sketch(k=k, S=S)
        info = d.mash_index_info()
        M = _matrix(d, k)
    finally:
        d.close()
    assert max(len(s) for s in seqs[:2 * C]) - k + 1 < S
    full = mi.marker_conditions(sk, C, Dm)
    assert sorted(full) == [0, 1]
    tables = _assert_info(info, consts, sk)
    assert info["chunks"] == 3
    last_uniq, last_cnt = tables[2]
    assert last_cnt.max() < Dm                              # the partial chunk has no dense value ...
    assert info["dense"] == sum(int((cnt >= Dm).sum()) for _, cnt in tables[:2]) > 0      # ... and the index reports none for it
    mi.assert_pair_classes(mi.pair_classes(sk, tables, C, Dm, range(1, n)))
    mi.assert_rows(M, mi.oracle_rows(orc, sk, k, range(1, n)))


_CLONAL = {}


def _clonal_reads():
    if "reads" not in _CLONAL:
        _CLONAL["reads"] = mi.clonal_4096(np.random.default_rng(4096))
    return _CLONAL["reads"]


@pytest.mark.parametrize("short", [0, 1], ids=["S=max", "S=max-1"])
def test_largest_sketches(orc, monkeypatch, consts, short):
    """Sketches of the largest size the library takes (and one value fewer): positions up to S - 1, counters up to S, a padding value
    with more than 2 000 copies behind shared values -- where "every difference fits 16 signed bits" of the packed dense path would
    first break -- on clonal reads, whose thousands of dense values run through the fused two-value update in ascending order."""
    C, Dm = consts["chunk_tips"], consts["dense_min"]
    S, k = consts["max_sketch"] - short, 15
    assert consts["max_sketch"] == 4096
    seqs = _clonal_reads()
    n = len(seqs)
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        sk = d.sketch(k=k, S=S)
        info = d.mash_index_info()
        M = _matrix(d, k)
    finally:
        d.close()
    seen = mi.clonal_conditions(sk, C, Dm)
    tables = _assert_info(info, consts, sk)
    rows = sorted(set([1, 2, 63, 64, 65, C - 1, C, C + 1, n - 1] + [int(i) for i in np.random.default_rng(1).integers(1, n, size=30)]))
    mi.assert_pair_classes(mi.pair_classes(sk, tables, C, Dm, rows))
    mi.assert_rows(M, mi.oracle_rows(orc, sk, k, rows))
    assert seen["dense"] >= 1000


def test_sketch_above_the_largest_size_is_refused(consts):
    import dipper_amd
    d = dipper_amd.Dipper(0)
    try:
        d.set_reads([b"ACGT" * 20, b"TTGACC" * 20])
        with pytest.raises(dipper_amd.DipperError, match=r"sketch size must be in \[1,4096\]"):
            d.sketch(k=15, S=consts["max_sketch"] + 1)
    finally:
        d.close()


def test_placement_batches_and_the_bounded_grid(orc, monkeypatch, consts):
    """4 300 tips: five placement batches, four of them produced beside the previous batch's tree kernels, where the launch is a
    bounded grid whose workgroups walk several (chunk, row) tasks and reuse their LDS counters (the batches from row 2 + 2 x 1 024 on
    have more tasks than the bound).  Matrix rows around every chunk edge against the oracle, the placement trace against the oracle
    on the device's matrix, and the same state from a context that produces every batch alone."""
    from dipper_amd import capi
    C = consts["chunk_tips"]
    n, S, k = 4300, 32, 15
    rng = np.random.default_rng(4300)
    seqs = _reads(rng, n, 300, 1500)
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        sk = d.sketch(k=k, S=S)
        _assert_info(d.mash_index_info(), consts, sk)
        M = _matrix(d, k)
        rows = [c * C + e for c in (1, 2, 3, 4) for e in (-1, 1)] + [n - 1] + [int(i) for i in rng.integers(1, n, size=20)]
        mi.assert_rows(M, mi.oracle_rows(orc, sk, k, sorted(set(rows))))
        got = d.place_run(capi.SRC_MASH, n, k=k)
        batches, beside = d.place_policy()
    finally:
        d.close()
    ref = orc.place_run(M)
    assert np.array_equal(got["trace"][2:], ref["trace"][2:])
    _same_state(got, ref, n)
    assert batches == -(-(n - 2) // BATCH) and beside >= 3, (batches, beside)
    i0 = 2 + 3 * BATCH
    nr = min(BATCH, n - i0)
    assert nr == BATCH and -(-(i0 + nr - 1) // C) * nr > consts["beside_task_bound"]
    monkeypatch.setenv("DPR_PLACE_NO_OVERLAP", "1")
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        d.sketch(k=k, S=S, fetch=False)
        alone = d.place_run(capi.SRC_MASH, n, k=k)
        assert d.place_policy() == (batches, 0)
    finally:
        d.close()
    _same_state(alone, got, n)


def test_transposed_block_over_two_chunks(orc, monkeypatch, consts):
    """divide-and-conquer assignment: the query x backbone block is written transposed, here over a backbone of C + 6 tips"""
    from dipper_amd import capi
    C = consts["chunk_tips"]
    n, B, S, k = C + 500, C + 6, 64, 15
    seqs = _reads(np.random.default_rng(n), n, 1500, 3000)
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        d.sketch(k=k, S=S, fetch=False)
        assert d.mash_index_info()["chunks"] == 2
        M = _matrix(d, k)
        got = d.dc_run(capi.SRC_MASH, n, B, k=k)
    finally:
        d.close()
    _same_dc_state(got, orc.dc_run(M, B, skip_last_backbone=0), n, B)


def test_fixed_backbone_over_two_chunks(orc, monkeypatch, consts):
    """40 queries against a fixed backbone of C + 5 tips, Mash source: every (slot, frac, add) equals the oracle's placement of
    that query alone on the backbone, from the device's own distance row"""
    from dipper_amd import capi
    C = consts["chunk_tips"]
    m, c, k = C + 5, 40, 15
    seqs = _reads(np.random.default_rng(m), m + c, 1500, 2500)
    nwk = _jplace.random_backbone(np.random.default_rng(100 + m), m, "random")
    d = _index_context(monkeypatch)
    try:
        d.set_reads(seqs)
        d.sketch(k=k, S=1000, fetch=False)
        assert d.mash_index_info()["chunks"] == 2
        d.set_place_fixed_batch(64)
        d.place_fixed_set(m, m + c, _jplace.backbone_arrays(orc, nwk, m + c)[0])
        got = d.place_fixed_run(capi.SRC_MASH, 0, k=k)
        rows = np.ascontiguousarray(_matrix(d, k)[m:, :m])
    finally:
        d.close()
    st0, _ = _jplace.backbone_arrays(orc, nwk, m + 1)
    orc.place_init_lists(m + 1, m, st0)
    ref = np.zeros((c, 3))
    D = np.zeros((m + 1, m + 1))
    for q in range(c):
        D[m, :m] = rows[q]
        ref[q] = orc.place_run(D, first=m, state={name: v.copy() for name, v in st0.items()})["trace"][m]
    same_triples(got, (ref[:, 0].astype(np.int32), ref[:, 1].copy(), ref[:, 2].copy()))


_ONE_RANK = {}


def _sharded_input(orc, monkeypatch, consts):
    """2 C + 7 tips of marker reads at S = 64 and their one-rank matrix, computed once"""
    if not _ONE_RANK:
        C, Dm = consts["chunk_tips"], consts["dense_min"]
        seqs = mi.marker_reads(np.random.default_rng(77), [C, C, 7], 15, mi.list_length_edges(C, Dm))
        d = _index_context(monkeypatch)
        try:
            d.set_reads(seqs)
            sk = d.sketch(k=15, S=64)
            M = _matrix(d, 15)
        finally:
            d.close()
        rows = sorted(set([1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, len(seqs) - 1] + [int(i) for i in np.random.default_rng(7).integers(1, len(seqs), size=12)]))
        mi.assert_rows(M, mi.oracle_rows(orc, sk, 15, rows))
        M.setflags(write=False)
        _ONE_RANK.update(seqs=seqs, M=M, rows=len(rows))
    return _ONE_RANK


@pytest.mark.parametrize("world", [2, 3])
def test_row_sharded_over_three_chunks(orc, monkeypatch, consts, world):
    """rows shared by row blocks over virtual ranks: every rank walks all rows on the index and keeps the pairs of its own rows,
    direct and mirrored -- bitwise the one-rank matrix, which 20 rows around the chunk edges tie to the oracle"""
    one = _sharded_input(orc, monkeypatch, consts)
    assert one["rows"] == 20
    d = _index_context(monkeypatch, virtual_world=world)
    try:
        d.set_reads(one["seqs"])
        d.sketch(k=15, S=64, fetch=False)
        assert d.mash_index_info()["chunks"] == 3
        from dipper_amd import capi
        d.dist_matrix(capi.SRC_MASH, 0, 15)
        M = d.matrix()
    finally:
        d.close()
    assert np.array_equal(M.view(np.uint64), one["M"].view(np.uint64))


@pytest.mark.parametrize("kernel", ["tokens", "table"])
def test_fallback_kernels_past_one_block(orc, monkeypatch, consts, kernel):
    """the kernels that serve where the index cannot be built, at C + 6 tips: more than one 512-column block of the table kernel,
    several row tiles of the token kernel"""
    C = consts["chunk_tips"]
    n, S, k = C + 6, 64, 15
    rng = np.random.default_rng(n)
    seqs = _reads(rng, n, 300, 1500)
    d = _index_context(monkeypatch, kernel=kernel)
    try:
        d.set_reads(seqs)
        sk = d.sketch(k=k, S=S)
        assert d.mash_index_info()["built"] == 0
        M = _matrix(d, k)
    finally:
        d.close()
    rows = sorted(set([1, 63, 64, 65, 255, 256, 257, 511, 512, 513, C - 1, C, C + 1, n - 1] + [int(i) for i in rng.integers(1, n, size=20)]))
    mi.assert_rows(M, mi.oracle_rows(orc, sk, k, rows))


def test_index_info(monkeypatch, consts):
    """dpr_get_mash_index_info: argument and state errors, no index under DPR_MASH_KERNEL=noindex, untouched by a distance call"""
    import dipper_amd
    from dipper_amd import capi
    L = capi.load_library()
    info = (C_.c_int64 * 8)()
    assert L.dpr_get_mash_index_info(None, info) == -1                  # DPR_ERR_ARG
    seqs = _reads(np.random.default_rng(3), 40, 200, 600)
    d = dipper_amd.Dipper(0)
    try:
        assert L.dpr_get_mash_index_info(d.h, None) == -1
        with pytest.raises(dipper_amd.DipperError) as ei:
            d.mash_index_info()
        assert ei.value.code == -3                                      # DPR_ERR_STATE: no sketch yet
        d.set_nj_mode(0)
        d.set_reads(seqs)
        with pytest.raises(dipper_amd.DipperError) as ei:
            d.mash_index_info()
        assert ei.value.code == -3
        sk = d.sketch(k=15, S=100)
        before = d.mash_index_info()
        _assert_info(before, consts, sk)
        assert before["chunks"] == 1 and before["beside_task_bound"] % 256 == 0
        _matrix(d, 15)
        d.place_run(capi.SRC_MASH, len(seqs), k=15)
        assert d.mash_index_info() == before
        monkeypatch.setenv("DPR_MASH_KERNEL", "noindex")
        d.sketch(k=15, S=100, fetch=False)
        off = d.mash_index_info()
        assert off == dict(before, built=0, chunks=0, distinct=0, dense=0)
    finally:
        d.close()
