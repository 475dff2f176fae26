"""The Mash pair kernels beside the inverted index -- bucket tables (mash_dist_lookup_kernel), run-encoded tokens (mash_encode_kernel,
mash_dist_tokens_kernel), the literal merge (mash_dist_rows_kernel) -- and the sketch kernel (mash_sketch_kernel) of
dipper_amd/csrc/mash.hip at the edges of their own rules and constants.  The inputs and the conditions that place them there are
tests/_mash_pair_inputs.py (shown on the oracle alone in tests/test_mash_pair_inputs.py); every test asserts them again on the
device's sketches.  Each input runs under DPR_MASH_KERNEL = table, tokens, noindex and literal.  Reference: the oracle's literal
merge (orc_mash_dist_row), rtol = 1e-12 (integer counts: the suite's rule, _mash_inputs.assert_rows); the three pair kernels also
agree bit for bit.  The divide-and-conquer run reaches mash_dist_lookup_kernel<true> (cluster jobs) and the transposed block.

The padding defect these tests found (fixed in the same change): the table kernel keeps two pad entries of ~0 behind a resident row
and took `row entry at the rank == column value` for a match without asking for rank < S, so the first pad of a padded column met
the pad entry behind an unpadded row; with duplicates in the row the multiplicities matched before it can exceed the pad's position,
the cut-off passes and the intersection counts one too many.  Before the fix 7 of the 124 tests failed: [phantom-table] of
test_rows_against_the_oracle (row 9, column 8: 0.0039728 against the oracle's 0.0045995, the figure of the restatement without the
bound), test_pair_kernels_bit_for_bit[phantom], test_phantom_pairs_in_both_roles and test_cluster_jobs_and_the_transposed_block under
all four kernel choices (table: its matrix row 25; the others: the cluster trees, built from mash_dist_lookup_kernel<true>).

What a one-line slip in mash.hip does here.  Each was built from a scratch copy and this file run once against it; every one
changes arithmetic only (no index or loop bound depends on the changed value).  Failing tests of 124:
  * `while (b0 < av)` walk removed: 12 -- test_rows_against_the_oracle[equal_tags | crowded | cut_off - table | noindex] (noindex takes the
    table kernel on these divergent reads), their bit-for-bit tests, test_shapes_and_placement_batches[table | noindex];
  * `row_dups` forced false: 33 -- every input with a duplicate in a row under `table` (phantom, crowded, crowded_dups, multiplicity,
    tokens_family, padded_reference, S = 63 .. 1 024), test_phantom_pairs_in_both_roles, the cluster jobs under all four choices;
  * `prev != a[u]` dropped from firstmask: the same 33;
  * `(mtotal + below)` -> `mtotal` in the cut-off of rows without duplicates: 45 -- crowded, equal_tags, catch_all, multiplicity, cut_off,
    tokens_family, every S >= 63, n = 15 .. 17, the shapes and test_strided_sample_and_128_columns_per_block[table];
  * `bend` never true in the token kernel (Lp = L): 28 -- phantom, crowded_dups, multiplicity, tokens_family, padded_reference, S = 63 ..
    1 024 under `tokens` (and `noindex` where it takes the tokens), the cluster-job test's transposed block under tokens | noindex;
  * kTokEq never set by the encoder: the same 28;
  * `(uint64_t)i < cnt` -> `<=` in the sketch fill: 94 -- every test that sketches a read shorter than its sketch or longer than a
    chunk, test_sketch_chunk_and_sort_edges at all four sizes and test_more_sequences_than_sketch_blocks among them;
  * `rankb < S` dropped from the match (the defect above): the 7 named there."""
import numpy as np
import pytest

from tests import _mash_inputs as mi, _mash_pair_inputs as pi
from tests.test_gpu_dc import _same_dc_state
from tests.test_gpu_mash_place import _same_state

pytestmark = pytest.mark.gpu

KERNELS = ("table", "tokens", "noindex", "literal")
PAIR_KERNELS = ("table", "tokens", "literal")
CANDIDATES = [(15, False), (16, False), (17, False), (15, True), (16, True), (17, True)]
BUILDERS = dict(pi.TABLE_BUILDERS)
BUILDERS.update(pi.TOKEN_BUILDERS)
BUILDERS.update({f"S={S}": (lambda S=S: pi.sizes(S)) for S in pi.SKETCH_SIZES})
BUILDERS.update({f"n={n}{',outlier' if o else ''}": (lambda n=n, o=o: pi.candidates(n, o)) for n, o in CANDIDATES})

_ORACLE = {}       # builder -> (oracle sketches, {row: oracle distances}), computed once and left unchanged
_MATRIX = {}       # (builder, kernel) -> the device's matrix


def _context(monkeypatch, kernel):
    import dipper_amd
    monkeypatch.setenv("DPR_MASH_KERNEL", kernel)      # (read at every sketch / distance call)
    d = dipper_amd.Dipper(0)
    d.set_nj_mode(0)                                   # the plain slot-space matrix
    return d


def _matrix(d, k):
    from dipper_amd import capi
    d.dist_matrix(capi.SRC_MASH, 0, k)
    M = d.matrix()
    assert np.array_equal(M, M.T) and np.all(np.diag(M) == 0)
    return M


def _oracle(orc, name, case, rows=None):
    if name not in _ORACLE:
        sk = mi.oracle_sketches(orc, case.reads, case.k, case.S)
        ref = mi.oracle_rows(orc, sk, case.k, range(1, case.n) if rows is None else rows)
        sk.setflags(write=False)
        for v in ref.values():
            v.setflags(write=False)
        _ORACLE[name] = (sk, ref)
    return _ORACLE[name]


def _device_matrix(orc, monkeypatch, name, kernel):
    """sketches equal the oracle's, the conditions hold on them, no index is built, the mirrored matrix is symmetric with a zero
    diagonal"""
    if (name, kernel) not in _MATRIX:
        case = pi.case(name, BUILDERS[name])
        want, _ = _oracle(orc, name, case)
        d = _context(monkeypatch, kernel)
        try:
            d.set_reads(case.reads)
            sk = d.sketch(k=case.k, S=case.S)
            assert d.mash_index_info()["built"] == 0
            M = _matrix(d, case.k)
        finally:
            d.close()
        assert np.array_equal(sk, want)
        print(name, kernel, case.conditions(sk))
        M.setflags(write=False)
        _MATRIX[name, kernel] = M
    return _MATRIX[name, kernel]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(BUILDERS))
def test_rows_against_the_oracle(orc, monkeypatch, name, kernel):
    """every builder under every kernel choice: all rows against the oracle's literal merge"""
    M = _device_matrix(orc, monkeypatch, name, kernel)
    mi.assert_rows(M, _oracle(orc, name, pi.case(name, BUILDERS[name]))[1])


@pytest.mark.parametrize("name", list(BUILDERS))
def test_pair_kernels_bit_for_bit(orc, monkeypatch, name):
    """the same integer counts go through the same expression in all three kernels"""
    Ms = [_device_matrix(orc, monkeypatch, name, kernel) for kernel in PAIR_KERNELS]
    for M, kernel in zip(Ms[1:], PAIR_KERNELS[1:]):
        assert np.array_equal(M.view(np.uint64), Ms[0].view(np.uint64)), kernel


def test_phantom_pairs_in_both_roles(orc, monkeypatch):
    """The pairs of the padding defect by themselves: with the padded tip as the column the table kernel's count is the oracle's,
    not the one more that the restatement without the rank bound gives; with the roles swapped the bound changes nothing."""
    case = pi.case("phantom", BUILDERS["phantom"])
    sk, _ = _oracle(orc, "phantom", case)
    M = _device_matrix(orc, monkeypatch, "phantom", "table")
    differs = 0
    for i, j in case.pairs:
        bounded, unbounded = (pi.mash_distance(pi.table_pair(sk[j], sk[i], bound=b)["inter"], case.S, case.k) for b in (True, False))
        assert np.isclose(M[i, j], bounded, rtol=1e-12, atol=0), (i, j, M[i, j], bounded, unbounded)
        differs += bounded != unbounded
    assert differs >= 10


@pytest.mark.parametrize("kernel", KERNELS)
def test_shapes_and_placement_batches(orc, monkeypatch, kernel):
    """1 100 tips at S = 1 024: three column blocks and 138 row groups of the table kernel (the last of 4 rows, many wholly below a
    column block), 18 row tiles of the token kernel at 8 columns per block, tiles across the diagonal; then placement: two batches (the
    second starts at row 2 + 1 024 and has 74 rows), and under the token kernel five batches of 256 rows."""
    from dipper_amd import capi
    case = pi.case("shapes", pi.shapes)
    want, ref = _oracle(orc, "shapes", case, case.rows)
    n = case.n
    d = _context(monkeypatch, kernel)
    try:
        d.set_reads(case.reads)
        sk = d.sketch(k=case.k, S=case.S)
        assert d.mash_index_info()["built"] == 0
        M = _matrix(d, case.k)
        got = d.place_run(capi.SRC_MASH, n, k=case.k) if kernel in ("table", "tokens") else None
        batches = d.place_policy()[0] if got else 0
        if kernel == "tokens":
            monkeypatch.setenv("DPR_PLACE_BATCH", "256")
            small = d.place_run(capi.SRC_MASH, n, k=case.k)
            small_batches = d.place_policy()[0]
    finally:
        d.close()
    assert np.array_equal(sk, want)
    print(kernel, case.conditions(sk))
    assert pi.cols_per_block(n, n) == 8 == pi.cols_per_block(256, n)
    mi.assert_rows(M, ref)
    _MATRIX["shapes", kernel] = M
    if got:
        state = orc.place_run(M)
        assert batches == 2
        _same_state(got, state, n)
        if kernel == "tokens":
            assert small_batches == 5
            _same_state(small, state, n)


def test_shapes_bit_for_bit(orc, monkeypatch):
    for kernel in PAIR_KERNELS:
        if ("shapes", kernel) not in _MATRIX:
            test_shapes_and_placement_batches(orc, monkeypatch, kernel)
    for kernel in PAIR_KERNELS[1:]:
        assert np.array_equal(_MATRIX["shapes", kernel].view(np.uint64), _MATRIX["shapes", "table"].view(np.uint64)), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_strided_sample_and_128_columns_per_block(orc, monkeypatch, kernel):
    """8 200 clonal tips at S = 8: the token counts are sampled with a stride of 2 (the strided copy), the reference is evaluated on
    every 32nd tip, the token kernel walks 128 columns per block over 129 row tiles; 30 rows are read back"""
    from dipper_amd import capi
    case = pi.case("strided_sample", pi.strided_sample)
    want, ref = _oracle(orc, "strided_sample", case, case.rows)
    d = _context(monkeypatch, kernel)
    try:
        d.set_reads(case.reads)
        sk = d.sketch(k=case.k, S=case.S)
        assert d.mash_index_info()["built"] == 0
        d.dist_matrix(capi.SRC_MASH, 0, case.k)
        rows = {i: d.matrix_row(i) for i in case.rows}
    finally:
        d.close()
    assert np.array_equal(sk, want)
    print(kernel, case.conditions(sk))
    for i in case.rows:
        assert rows[i][i] == 0.0
        ok = np.isclose(rows[i][:i], ref[i], rtol=1e-12, atol=0)
        assert ok.all(), (i, np.flatnonzero(~ok)[:5])
        for j in case.rows:
            assert rows[i][j] == rows[j][i]


@pytest.mark.parametrize("kernel", KERNELS)
def test_cluster_jobs_and_the_transposed_block(orc, monkeypatch, kernel):
    """divide and conquer on a backbone of 24 reads with six families of four queries, each family one cluster that holds the pair
    of the padding defect with the padded tip as the earlier member: the cluster jobs (mash_dist_lookup_kernel<true>, whatever the
    kernel choice) and the transposed query x backbone block (the chosen kernel) against the oracle on the verified matrix"""
    from dipper_amd import capi
    case = pi.case("dc_family", pi.dc_family)
    want, ref = _oracle(orc, "dc_family", case)
    n, B = case.n, case.B
    d = _context(monkeypatch, kernel)
    try:
        d.set_reads(case.reads)
        sk = d.sketch(k=case.k, S=case.S)
        M = _matrix(d, case.k)
        got = d.dc_run(capi.SRC_MASH, n, B, k=case.k)
    finally:
        d.close()
    assert np.array_equal(sk, want)
    print(kernel, case.conditions(sk))
    mi.assert_rows(M, ref)
    state = orc.dc_run(M, B, skip_last_backbone=0)
    for i, j in case.edge:
        assert j < i and state["cluster_id"][i] == state["cluster_id"][j] >= 0
    _same_dc_state(got, state, n, B)


@pytest.mark.parametrize("S", [1, 1000, 1024, 4096])
def test_sketch_chunk_and_sort_edges(orc, monkeypatch, S):
    """whole sketches against orc.sketch at the chunk edge (nk = cap - 1, cap, cap + 1, 2 cap, 2 cap + 1 with cap = 16 384 - S), at the
    sort sizes (S + nk = 1 024, 1 025, 2 048, 2 049, 16 384), around k and around a multiple of 32 bases"""
    reads = pi.sketch_reads(S)
    nk = [max(len(r) - 15 + 1, 0) for r in reads]
    cap = pi.kSortCap - S
    assert {cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1} <= set(nk) and {0, 1, 2} <= set(nk)
    assert {t - S for t in (1024, 1025, 2048, 2049, pi.kSortCap) if t - S >= 1} <= set(nk)
    d = _context(monkeypatch, "literal")               # (no index, no token encoding: the sketch kernel alone)
    try:
        d.set_reads(reads)
        sk = d.sketch(k=15, S=S)
    finally:
        d.close()
    want = mi.oracle_sketches(orc, reads, 15, S)
    for q in range(len(reads)):
        assert np.array_equal(sk[q], want[q]), (q, len(reads[q]))


def test_more_sequences_than_sketch_blocks(orc, monkeypatch):
    reads = pi.many_sequences()
    assert len(reads) == 1030 and len(reads[-1]) == 40000
    d = _context(monkeypatch, "literal")
    try:
        d.set_reads(reads)
        sk = d.sketch(k=15, S=1000)
    finally:
        d.close()
    assert np.array_equal(sk, mi.oracle_sketches(orc, reads, 15, 1000))
