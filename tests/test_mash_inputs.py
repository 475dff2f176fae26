"""The inputs of tests/test_gpu_mash_index_edges.py sit where that file needs them -- shown on the oracle's sketches alone, for the
constants of the inverted-index kernel as it stands (chunks of 1 024 tips, dense from 384 entries).  The GPU tests assert the same
conditions again on the device's sketches with the constants the library reports."""
import numpy as np
import pytest

from tests import _mash_inputs as mi

C, DM = 1024, 384


@pytest.fixture(scope="module")
def marker_sketches(orc):
    reads = mi.marker_reads(np.random.default_rng(2055), [C, C, 7], 15, mi.list_length_edges(C, DM))
    return reads, mi.oracle_sketches(orc, reads, 15, 512)


@pytest.fixture(scope="module")
def clonal_sketches(orc):
    return mi.oracle_sketches(orc, mi.clonal_4096(np.random.default_rng(4096)), 15, 4096)


def test_marker_reads_hold_every_list_length(marker_sketches):
    reads, sk = marker_sketches
    assert len(reads) == 2 * C + 7
    S = sk.shape[1]
    # every k-mer of a read of a full chunk is in its sketch
    assert max(len(r) for r in reads[:2 * C]) - 15 + 1 < S
    full = mi.marker_conditions(sk, C, DM)
    assert sorted(full) == [0, 1]
    # the seven tips of the last chunk hold every marker given to seven or more tips: no padding, no list of more than 7 entries
    uniq, cnt = mi.chunk_tables(sk, C)[2]
    assert cnt.max() <= 7 and mi.PAD not in uniq
    # the padding value is the one dense value with a large multiplicity, at many different first positions
    pad = mi.padding_copies(sk[:2 * C])
    assert len(np.unique(pad)) > 100 and pad.max() > 300


def test_marker_reads_meet_every_pair_class(marker_sketches):
    _, sk = marker_sketches
    classes = mi.pair_classes(sk, mi.chunk_tables(sk, C), C, DM, range(1, len(sk)))
    mi.assert_pair_classes(classes)


def test_clonal_4096_reaches_the_limits_of_the_packed_arithmetic(clonal_sketches):
    sk = clonal_sketches
    assert sk.shape == (1030, 4096)
    seen = mi.clonal_conditions(sk, C, DM)
    assert seen["padded_tips"] == 394 and seen["most_copies"] == 4096 - (2000 - 15 + 1)
    n = len(sk)
    rows = sorted(set([1, 2, 63, 64, 65, C - 1, C, C + 1, n - 1] + [int(i) for i in np.random.default_rng(1).integers(1, n, size=30)]))
    mi.assert_pair_classes(mi.pair_classes(sk, mi.chunk_tables(sk, C), C, DM, rows))
    # one position fewer: still every condition but the last position in use
    sk2 = sk[:, :4095]
    uniq, cnt = mi.chunk_tables(sk2[:C], C)[0]
    assert (cnt >= DM).sum() >= 1000


def test_index_counts_count_copies_as_entries():
    """a value twice in each of two sketches is one (chunk, value) pair of four entries"""
    sk = np.array([[1, 1, 5], [1, 1, 7], [2, 7, 7]], dtype=np.uint64)
    assert mi.index_counts(mi.chunk_tables(sk, 2), 4) == (3 + 2, 1)
    assert mi.index_counts(mi.chunk_tables(sk, 4), 3) == (4, 2)
    cl = mi.pair_classes(sk, mi.chunk_tables(sk, 4), 4, 3, [2])
    assert cl == {"dense,dense": 0, "dense,sparse": 0, "sparse,dense": 1, "sparse,sparse": 0, "single": 0}
