"""GPU: the site filter at the library level (sites.hip; dpr_get_msa_site_coverage, dpr_msa_filter_sites) against the NumPy
restatement of tests/_sites_ref.py.

Coverage must equal the reference exactly.  The filter is checked through its contract: context A filters on the device, context
B uploads the host-filtered alignment, and everything the two can be asked -- the integer counts of every row, every distance
matrix, bootstrap replicates -- must be the same bits.  The coverage kernel gives a wavefront every fourth sequence of its block,
a block 248 sequences (two periods of 31 for each of its four wavefronts) and gridDim.y the rest: the sequence counts below sit
around 16, 256, one period of every wavefront (124), one block (248) and the 64-word block edge (L = 2048 / 2049)."""
import numpy as np
import pytest

from tests import _aa_ref, _sites_ref, _util

pytestmark = pytest.mark.gpu

NT_SYM = np.frombuffer(b"ACGTU", dtype=np.uint8)
NT_NOT = np.frombuffer(b"-Nacgtn?", dtype=np.uint8)
AA_SYM = np.frombuffer(b"ARNDCQEGHILKMFPSTWYVarndcqeghilkmfpstwyv", dtype=np.uint8)
AA_NOT = np.frombuffer(b"X*-xBZ", dtype=np.uint8)


@pytest.fixture(scope="module")
def ab():
    import dipper_amd
    a, b = dipper_amd.Dipper(0), dipper_amd.Dipper(0)
    yield a, b
    a.close()
    b.close()


def _upload(d, seqs, alphabet):
    from dipper_amd import capi
    if alphabet == "nt":
        d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
    else:
        d.set_msa_aa(capi.pack_aa_many(seqs))


def _holders(rng, n, counts):
    """bool [n][L] with exactly counts[c] True in column c"""
    L = len(counts)
    rank = rng.random((n, L)).argsort(axis=0).argsort(axis=0)
    return rank < np.asarray(counts)[None, :]


def _paint(rng, base, holds, alphabet):
    """byte strings: base (symbols, uint8 [n][L]) where holds, a not-a-symbol byte elsewhere"""
    a = base.copy()
    bad = ~holds
    a[bad] = rng.choice(NT_NOT if alphabet == "nt" else AA_NOT, size=int(bad.sum()))
    return [r.tobytes() for r in a]


def _coverage_case(rng, n, L, alphabet):
    """every kind of column: nobody, everybody, exactly half (the 500 per mille tie), one below it, anything"""
    kinds = rng.integers(0, 5, size=L)
    counts = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3], [0, n, (n + 1) // 2, max((n + 1) // 2 - 1, 0)],
                       rng.integers(0, n + 1, size=L))
    base = rng.choice(NT_SYM if alphabet == "nt" else AA_SYM, size=(n, L))
    return _paint(rng, base, _holders(rng, n, counts), alphabet), counts


NS = (2, 15, 16, 17, 123, 124, 125, 247, 248, 249, 255, 256, 257)
LS = (1, 31, 32, 33, 2047, 2048, 2049)


def test_one_sequence_is_no_alignment(ab):
    """n = 1 never reaches the filter: dpr_set_msa refuses fewer than two sequences"""
    from dipper_amd import capi
    with pytest.raises(capi.DipperError) as e:
        _upload(ab[0], [b"ACGT"], "nt")
    assert e.value.code == -1


@pytest.mark.parametrize("alphabet", ["nt", "aa"])
def test_coverage_equals_reference(ab, alphabet):
    a, _ = ab
    rng = np.random.default_rng(11 if alphabet == "nt" else 12)
    for n in NS:
        for L in LS:
            if alphabet == "aa" and (n not in (2, 17, 125, 249, 257) or L not in (1, 33, 2049)):
                continue
            seqs, counts = _coverage_case(rng, n, L, alphabet)
            ref = _sites_ref.coverage(seqs, alphabet)
            assert np.array_equal(ref, counts)
            _upload(a, seqs, alphabet)
            got = a.msa_site_coverage()
            assert got.dtype == np.int32 and got.shape == (L,)
            assert np.array_equal(got, ref), (alphabet, n, L, np.flatnonzero(got != ref)[:8])
            # the same columns through the filter: half of the sequences is a tie at 500 per mille for an even n
            k = _sites_ref.keep(ref, n, 500)
            if k.any():
                assert a.msa_filter_sites(500) == int(k.sum()), (alphabet, n, L)
                assert np.array_equal(a.msa_site_coverage(), ref[k]), (alphabet, n, L)


# ---- equivalence: filter on the device (A) == upload of the host-filtered alignment (B) ----------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.where(np.isnan(a), 0, a).view(np.uint64), np.where(np.isnan(b), 0, b).view(np.uint64))


N_EQ = 70          # more than one 64-sequence tile
PM_EQ = 900        # kept columns hold 63 .. 70 of 70 sequences, dropped ones 0 .. 62


def _related(rng, n, L, alphabet):
    if alphabet == "nt":
        s = _util.synth_alignment(rng, n, L, mean_bl=0.02, lo=0.002, hi=0.1)
    else:
        s = _aa_ref.evolve_yule(rng, n, L)
    return np.frombuffer(b"".join(s), dtype=np.uint8).reshape(n, L).copy()


def _eq_case(rng, mask, alphabet, n=N_EQ):
    """an alignment whose kept columns at PM_EQ are exactly `mask` (kept columns still carry a few gaps)"""
    mask = np.asarray(mask, dtype=bool)
    L = len(mask)
    need = -(-PM_EQ * n // 1000)
    counts = np.where(mask, rng.integers(need, n + 1, size=L), rng.integers(0, need, size=L))
    seqs = _paint(rng, _related(rng, n, L, alphabet), _holders(rng, n, counts), alphabet)
    assert np.array_equal(_sites_ref.keep(_sites_ref.coverage(seqs, alphabet), n, PM_EQ), mask)
    return seqs


def _mask_alternating():
    m = np.zeros(700, dtype=bool)
    m[::2] = True                      # every output word draws from two input words
    return m


def _mask_long_run():
    m = np.ones(40 + 66 * 32 + 5 + 50, dtype=bool)
    m[40:40 + 66 * 32 + 5] = False     # one dropped run of more than 64 words inside an output word
    return m


def _mask_count(L, kept, seed):
    m = np.zeros(L, dtype=bool)
    m[np.random.default_rng(seed).choice(L, size=kept, replace=False)] = True
    return m


def _mask_band_to_table():
    m = np.ones(1100, dtype=bool)      # 1100 sites: the band table; 1000 kept: the full table
    m[np.random.default_rng(3).choice(1100, size=100, replace=False)] = False
    return m


NT_MASKS = {
    "alternating": _mask_alternating,
    "long_run": _mask_long_run,
    "kept1": lambda: _mask_count(100, 1, 1),
    "kept32": lambda: _mask_count(100, 32, 2),
    "kept33": lambda: _mask_count(2100, 33, 4),
    "noop": lambda: np.ones(333, dtype=bool),
    "band_to_table": _mask_band_to_table,
}


def _matrices(d, types):
    from dipper_amd import capi
    out = {}
    for dt in types:
        d.dist_matrix(capi.SRC_MSA, dt)
        out[dt] = d.matrix()
    return out


def _check_equal(a, b, n, types, what):
    for row in range(n):
        ua, ma = a.msa_counts(row)
        ub, mb = b.msa_counts(row)
        assert np.array_equal(ua, ub) and np.array_equal(ma, mb), (what, "counts", row)
    ma, mb = _matrices(a, types), _matrices(b, types)
    for dt in types:
        assert _same_bits(ma[dt], mb[dt]), (what, dt)
    return ma


@pytest.mark.parametrize("case", list(NT_MASKS))
def test_filter_equals_upload_of_filtered_nucleotides(ab, case):
    from dipper_amd import capi
    a, b = ab
    mask = NT_MASKS[case]()
    seqs = _eq_case(np.random.default_rng(len(mask)), mask, "nt")
    want = _sites_ref.filtered(seqs, mask)
    _upload(a, seqs, "nt")
    assert a.msa_filter_sites(PM_EQ) == int(mask.sum()) == len(want[0])
    _upload(b, want, "nt")
    assert np.array_equal(a.msa_site_coverage(), b.msa_site_coverage())
    base = _check_equal(a, b, N_EQ, (1, 2, 4, 9, 10), case)
    assert np.isfinite(base[1]).any()
    # bootstrap replicates draw columns as a function of L': the same replicate on both sides
    for r in (0, 1):
        a.msa_resample(77, r)
        b.msa_resample(77, r)
        assert np.array_equal(a.msa_boot_weights(len(want[0])), capi.msa_boot_weights(77, r, len(want[0])))
        for dt in (2, 4):
            assert _same_bits(_matrices(a, (dt,))[dt], _matrices(b, (dt,))[dt]), (case, "replicate", r, dt)
    a.msa_resample(77, -1)
    b.msa_resample(77, -1)
    assert _same_bits(_matrices(a, (2,))[2], base[2]), (case, "replicate -1")


def test_filter_equals_upload_of_filtered_protein(ab):
    a, b = ab
    mask = _mask_count(200 + 70 * 32 + 300, 1400, 9)
    mask[200:200 + 70 * 32] = False      # a dropped run of 70 words between scattered columns
    seqs = _eq_case(np.random.default_rng(21), mask, "aa")
    want = _sites_ref.filtered(seqs, mask)
    _upload(a, seqs, "aa")
    assert a.msa_filter_sites(PM_EQ) == int(mask.sum())
    _upload(b, want, "aa")
    m = _check_equal(a, b, N_EQ, (1, 8), "protein")
    assert np.isfinite(m[1]).any()


def test_filter_twice_and_upload_after_filter(ab):
    """a second, stricter filter works on the filtered alignment; set_msa after a filter is a fresh upload"""
    a, b = ab
    rng = np.random.default_rng(8)
    seqs = _eq_case(rng, _mask_count(500, 300, 5), "nt")
    cov = _sites_ref.coverage(seqs, "nt")
    k1 = _sites_ref.keep(cov, N_EQ, PM_EQ)
    k2 = _sites_ref.keep(cov, N_EQ, 1000)
    assert 0 < k2.sum() < k1.sum()
    _upload(a, seqs, "nt")
    assert a.msa_filter_sites(PM_EQ) == int(k1.sum())
    assert a.msa_filter_sites(1000) == int(k2.sum())
    _upload(b, _sites_ref.filtered(seqs, k2), "nt")
    _check_equal(a, b, N_EQ, (2,), "twice")
    other = _eq_case(rng, _mask_count(1300, 900, 6), "nt", n=40)
    _upload(a, other, "nt")
    _upload(b, other, "nt")
    assert a.msa_site_coverage().shape == (1300,)
    _check_equal(a, b, 40, (1, 2), "fresh upload")


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_alignment_as_it_was(ab):
    from dipper_amd import capi
    a, _ = ab
    rng = np.random.default_rng(14)
    n, L = 20, 300
    counts = rng.integers(0, n, size=L)      # no column is held by everybody
    seqs = _paint(rng, _related(rng, n, L, "nt"), _holders(rng, n, counts), "nt")
    _upload(a, seqs, "nt")
    before = _matrices(a, (1, 2))
    for bad in (0, 1001, -5):
        with pytest.raises(capi.DipperError) as e:
            a.msa_filter_sites(bad)
        assert e.value.code == -1
    with pytest.raises(capi.DipperError) as e:
        a.msa_filter_sites(1000)
    assert e.value.code == -1 and f"best coverage: {int(counts.max())} of {n}" in str(e.value)
    assert np.array_equal(a.msa_site_coverage(), counts)
    after = _matrices(a, (1, 2))
    for dt in (1, 2):
        assert _same_bits(before[dt], after[dt])
    # a replicate is active: the state error, and the replicate stays
    a.msa_resample(5, 0)
    with pytest.raises(capi.DipperError) as e:
        a.msa_filter_sites(500)
    assert e.value.code == -3
    a.msa_resample(5, -1)
    assert a.msa_filter_sites(500) == int(_sites_ref.keep(counts, n, 500).sum())


def test_no_alignment_is_a_state_error():
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        with pytest.raises(capi.DipperError) as e:
            d.msa_filter_sites(500)
        assert e.value.code == -3
        with pytest.raises(capi.DipperError) as e:
            d.msa_site_coverage()
        assert e.value.code == -3
    finally:
        d.close()


# ---- threshold ties --------------------------------------------------------------------------------------------------------------
def test_threshold_ties(ab):
    a, _ = ab
    rng = np.random.default_rng(2)
    # n = 8, 500 per mille: cov 4 is kept (4000 >= 4000), cov 3 dropped
    counts = np.array([4, 3, 8, 0, 4, 5, 3, 4] * 9)
    seqs = _paint(rng, rng.choice(NT_SYM, size=(8, len(counts))), _holders(rng, 8, counts), "nt")
    _upload(a, seqs, "nt")
    assert np.array_equal(a.msa_site_coverage(), counts)
    assert a.msa_filter_sites(500) == int((counts >= 4).sum())
    assert np.array_equal(a.msa_site_coverage(), counts[counts >= 4])
    # n = 3: cov 2 is dropped at 667 per mille (2000 < 2001) and kept at 666 (2000 >= 1998)
    counts = np.array([3, 2, 1, 2, 3, 0, 2] * 5)
    seqs = _paint(rng, rng.choice(NT_SYM, size=(3, len(counts))), _holders(rng, 3, counts), "nt")
    _upload(a, seqs, "nt")
    assert a.msa_filter_sites(667) == int((counts == 3).sum())
    _upload(a, seqs, "nt")
    assert a.msa_filter_sites(666) == int((counts >= 2).sum())
    assert np.array_equal(a.msa_site_coverage(), counts[counts >= 2])
