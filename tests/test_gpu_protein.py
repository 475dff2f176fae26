"""GPU: protein alignments (msa_aa.hip behind dpr_set_msa_aa) against the NumPy reference of tests/_aa_ref.py.

The pair tile is 64 x 64 with 16-word (512-site) stages; a stage in which no sequence of the tile has a not-a-residue position
skips the X plane, and useful comes from per-sequence totals.  Every builder below is asserted on the reference for the regime it
is meant to produce, then checked under one rule: integer counts exactly, type 1 bit for bit, types 2 / 7 / 8 with the
reference's NaN / +inf pattern and every finite cell within relative 1e-11 (the project's bound for distances through log,
DESIGN.md section 3), the block hook and row-sharded ranks bit for bit the one-rank matrix."""
import numpy as np
import pytest

from tests import _aa_ref, _util
from tests.test_gpu_msa_edges import _hook_shapes

pytestmark = pytest.mark.gpu

TYPES = (1, 2, 7, 8)
RTOL = 1e-11


def _density(L, n, rate, seed=0, runs=False, chars=b"-"):
    rng = np.random.default_rng(1000 * seed + 7 * L + n)
    seqs = _aa_ref.to_bytes(_aa_ref.related(rng, n, L))
    if rate > 0:
        _aa_ref.scatter(rng, seqs, rate, chars=chars, runs=runs)
    return [bytes(s) for s in seqs]


def _one_empty(L=2080, n=65):
    seqs = _density(L, n, 0.03, seed=1)
    seqs[40] = b"-" * L
    return seqs


def _empty_block(L=2080, n=65):
    seqs = [bytearray(s) for s in _density(L, n, 0.0, seed=2)]
    for s in seqs:
        s[500:1100] = b"-" * 600          # covers the whole second stage (sites 512..1023)
    return [bytes(s) for s in seqs]


def _last_word(L=2080, n=65):
    rng = np.random.default_rng(3)
    seqs = [bytearray(s) for s in _density(L, n, 0.0, seed=3)]
    for s in seqs:
        for pos in rng.integers(L - 32, L, size=5):
            s[pos] = ord("-")
    return [bytes(s) for s in seqs]


def _mixed_bytes(L=2080, n=65):
    seqs = _density(L, n, 0.05, seed=4, chars=b"XBZ*xbz?.JUO1")
    return [s.lower() if i % 2 else s for i, s in enumerate(seqs)]


def _top_bit(L=2080, n=65):
    """residues 16..19 (code + 1 = 17..20: top plane set) and residue 0 only"""
    rng = np.random.default_rng(5)
    codes = np.array([0, 16, 17, 18, 19], dtype=np.uint8)[_aa_ref.related(rng, n, L, alphabet=5)]
    return [bytes(s) for s in _aa_ref.scatter(rng, _aa_ref.to_bytes(codes), 0.02)]


def _uniform(L=2080, n=65):
    rng = np.random.default_rng(6)
    codes = _aa_ref.related(rng, n, L, lo=0.0, hi=0.4)
    assert np.all(np.bincount(codes.ravel(), minlength=20) > 0)
    return [bytes(s) for s in _aa_ref.to_bytes(codes)]


def _saturated(L=2080, n=33):
    """sequences 1 and 2 share no residue at any site; 3 and 4 differ at about 90 % of the sites; 5 has no residue at all"""
    rng = np.random.default_rng(8)
    codes = _aa_ref.related(rng, n, L)
    codes[2] = (codes[1] + rng.integers(1, 20, size=L, dtype=np.uint8)) % 20
    codes[4] = codes[3]
    hit = rng.random(L) < 0.9
    codes[4, hit] = (codes[3, hit] + rng.integers(1, 20, size=int(hit.sum()), dtype=np.uint8)) % 20
    seqs = [bytes(s) for s in _aa_ref.scatter(rng, _aa_ref.to_bytes(codes), 0.01)]
    seqs[5] = b"-" * L
    return seqs


def _has_x(ref, lo=1):
    return np.sum(ref["codes"] >= 20) >= lo


# name -> (builder, what the reference must show for the builder to be in its regime)
CASES = {}
for _L in (1, 31, 32, 33, 511, 512, 513, 1024, 1025, 2080, 2090):      # around a word, a stage (16 words = 512 sites), two stages, a partial quad
    CASES[f"L{_L}"] = ((lambda L=_L: _density(L, 33, 0.03)), lambda ref: ref["codes"].shape[0] == 33)
for _n in (2, 3, 31, 32, 33, 63, 64, 65, 129):
    CASES[f"n{_n}"] = ((lambda n=_n: _density(2080, n, 0.03)), lambda ref: _has_x(ref))
CASES["clean"] = (lambda: _density(2080, 65, 0.0), lambda ref: not _has_x(ref) and np.all(ref["useful"] == 2080))
for _rate in (0.001, 0.03, 0.3):
    CASES[f"scatter{_rate}"] = ((lambda r=_rate: _density(2080, 65, r, seed=9)),
                                lambda ref, r=_rate: 0.5 * r < np.mean(ref["codes"] >= 20) < 1.5 * r)
CASES["runs"] = (lambda: _density(2080, 65, 0.03, seed=10, runs=True), lambda ref: _has_x(ref, 200))
CASES["one_empty"] = (_one_empty, lambda ref: np.all(ref["useful"][40] == 0) and np.all(np.isnan(ref[1][40, :40])))
CASES["empty_block"] = (_empty_block, lambda ref: np.all(ref["useful"] == 2080 - 600))
CASES["last_word"] = (_last_word, lambda ref: _has_x(ref) and np.all(ref["codes"][:, :2048] < 20))
CASES["mixed_bytes"] = (_mixed_bytes, lambda ref: _has_x(ref, 1000))
CASES["top_bit"] = (_top_bit, lambda ref: set(np.unique(ref["codes"])) == {0, 16, 17, 18, 19, 255})
CASES["uniform"] = (_uniform, lambda ref: not _has_x(ref))
CASES["saturated"] = (_saturated, lambda ref: ref["match"][2, 1] == 0 and ref[7][2, 1] == np.inf and np.isnan(ref[2][2, 1])
                      and np.isnan(ref[8][2, 1]) and 0.88 < ref[1][4, 3] < 0.92 and np.all(np.isnan(ref[7][5, :5])))

_SEQS, _REF, _GPU = {}, {}, {}


def _seqs(case):
    if case not in _SEQS:
        _SEQS[case] = CASES[case][0]()
    return _SEQS[case]


def _ref(case):
    """codes, integer counts and the four reference matrices, once per case"""
    if case not in _REF:
        codes = _aa_ref.encode(_seqs(case))
        useful, match = _aa_ref.counts(codes)
        r = {"codes": codes, "useful": useful, "match": match}
        for dt in TYPES:
            r[dt] = _aa_ref.matrix(useful, match, dt)
        for v in r.values():
            v.setflags(write=False)
        _REF[case] = r
    return _REF[case]


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def _upload(d, case):
    from dipper_amd import capi
    codes = capi.pack_aa_many(_seqs(case))
    assert np.array_equal(codes, _ref(case)["codes"])
    d.set_msa_aa(codes)


def _matrices(d, case):
    from dipper_amd import capi
    _upload(d, case)
    out = {}
    for dt in TYPES:
        d.dist_matrix(capi.SRC_MSA, dt)
        out[dt] = d.matrix()
    return out


def _fast(gpu, case):
    if case not in _GPU:
        _GPU[case] = _matrices(gpu, case)
    return _GPU[case]


def _same_bits(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.where(np.isnan(a), 0, a).view(np.uint64), np.where(np.isnan(b), 0, b).view(np.uint64))


@pytest.mark.parametrize("case", list(CASES))
def test_counts_and_matrix_against_reference(gpu, case):
    ref = _ref(case)
    n = ref["codes"].shape[0]
    lo = np.tril_indices(n, -1)
    # the builder is in its regime; every case has a finite cell, the saturated ones +inf and NaN as well
    assert CASES[case][1](ref), case
    assert np.isfinite(ref[8][lo]).any(), case
    if case == "saturated":
        assert np.isposinf(ref[7][lo]).any() and np.isnan(ref[7][lo]).any() and np.isnan(ref[8][lo]).any()
    M = _fast(gpu, case)
    _upload(gpu, case)
    for row in (1, 63, 64, n - 1):
        if row < n:
            u, m = gpu.msa_counts(row)
            assert np.array_equal(u, ref["useful"][row, :row]) and np.array_equal(m, ref["match"][row, :row]), (case, row)
    for dt in TYPES:
        G, R = M[dt], ref[dt]
        assert _same_bits(G, G.T), (case, dt)
        assert np.all(np.diag(G) == 0), (case, dt)
        if dt == 1:
            assert _same_bits(G, R), (case, dt)
            continue
        assert np.array_equal(np.isnan(G), np.isnan(R)), (case, dt)
        assert np.array_equal(np.isposinf(G), np.isposinf(R)) and not np.isneginf(G).any() and not np.isneginf(R).any(), (case, dt)
        fin = np.isfinite(R)
        err = np.abs(G[fin] - R[fin])
        worst = float(np.max(err / np.maximum(np.abs(R[fin]), np.finfo(np.float64).tiny))) if err.size and err.max() > 0 else 0.0
        print(f"{case} type {dt}: largest relative difference {worst:.3e}")
        assert np.all(err <= RTOL * np.abs(R[fin])), (case, dt, worst)


HOOK_CASES = [c for c in CASES if not c.startswith("n") or c in ("n65", "n129")]


@pytest.mark.parametrize("case", HOOK_CASES)
def test_block_hook_equals_matrix(gpu, case):
    """msa_dist_block (placement, --add, fixed-backbone placement) in both orientations: bit for bit the matrix off the diagonal"""
    M = _fast(gpu, case)
    n = len(_seqs(case))
    _upload(gpu, case)
    shapes = list(_hook_shapes(n))
    assert shapes
    for dt in TYPES:
        for row0, nrows, ncols in shapes:
            blk, _ = gpu.msa_dist_block(row0, nrows, ncols, dist_type=dt)
            blk_t, _ = gpu.msa_dist_block(row0, nrows, ncols, dist_type=dt, transposed=True)
            want = M[dt][row0:row0 + nrows, :ncols].copy()
            r = np.arange(nrows)
            on = row0 + r < ncols
            want[r[on], row0 + r[on]] = blk[r[on], row0 + r[on]]
            assert _same_bits(blk, want), (case, dt, row0, nrows, ncols)
            assert _same_bits(blk_t, want.T), (case, dt, row0, nrows, ncols, "transposed")


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("case", ["scatter0.03", "n129"])
def test_row_sharded_ranks_equal_one_rank(gpu, case, world):
    import dipper_amd
    M = _fast(gpu, case)
    d = dipper_amd.Dipper(0, virtual_world=world)
    try:
        P = _matrices(d, case)
        for dt in TYPES:
            assert _same_bits(P[dt], M[dt]), (case, world, dt)
    finally:
        d.close()


def test_refusals_and_alphabet_switch(gpu):
    """nucleotide models, bootstrap replicates and divide-and-conquer refuse a protein alignment with DPR_ERR_ARG; types 7-8
    refuse a nucleotide alignment; each upload replaces the other alphabet's alignment"""
    import dipper_amd
    from dipper_amd import capi
    rng = np.random.default_rng(11)
    nuc = _util.synth_alignment(rng, 70, 700, mean_bl=5e-3, lo=1e-4, hi=5e-2, invalid_frac=0.02)
    gpu.set_msa(capi.pack4_many(nuc), 700)
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    before = gpu.matrix()
    for dt in (capi.DIST_POISSON, capi.DIST_KIMURA):
        with pytest.raises(dipper_amd.DipperError) as ei:
            gpu.dist_matrix(capi.SRC_MSA, dt)
        assert ei.value.code == -1
    _upload(gpu, "n65")
    for dt in (3, 4, 5, 6):
        with pytest.raises(dipper_amd.DipperError) as ei:
            gpu.dist_matrix(capi.SRC_MSA, dt)
        assert ei.value.code == -1 and "nucleotide" in str(ei.value)
        with pytest.raises(dipper_amd.DipperError) as ei:
            gpu.msa_dist_block(0, 10, 10, dist_type=dt)
        assert ei.value.code == -1
    with pytest.raises(dipper_amd.DipperError) as ei:
        gpu.dist_matrix(capi.SRC_MSA, 9)
    assert ei.value.code == -1
    with pytest.raises(dipper_amd.DipperError) as ei:
        gpu.msa_resample(1, 0)
    assert ei.value.code == -1 and "protein" in str(ei.value)
    with pytest.raises(dipper_amd.DipperError) as ei:
        gpu.dc_run(capi.SRC_MSA, 65, 10, dist_type=1)
    assert ei.value.code == -1 and "protein" in str(ei.value)
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)                      # the context still works after the refusals
    assert _same_bits(gpu.matrix(), _fast(gpu, "n65")[8])
    gpu.set_msa(capi.pack4_many(nuc), 700)
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    assert _same_bits(gpu.matrix(), before)
    gpu.msa_resample(1, 0)                                               # and a nucleotide alignment resamples again
    gpu.msa_resample(1, -1)


@pytest.fixture(scope="module")
def evolved():
    seqs = _aa_ref.evolve_yule(np.random.default_rng(12), 200, 600)
    useful, match = _aa_ref.counts(_aa_ref.encode(seqs))
    assert np.all(np.isfinite(_aa_ref.matrix(useful, match, 8))) and np.all(np.isfinite(_aa_ref.matrix(useful, match, 7)))
    return seqs


def test_nj_on_kimura_distances(gpu, orc, evolved):
    from dipper_amd import capi
    gpu.set_msa_aa(capi.pack_aa_many(evolved))
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)
    M = gpu.matrix()
    assert np.all(np.isfinite(M))
    ref = orc.nj_run(np.tril(M, -1))
    res = gpu.nj_run()
    assert res["iters"] == ref["iters"] == len(evolved) - 2
    assert np.array_equal(res["merge_x"], ref["merge_x"]) and np.array_equal(res["merge_y"], ref["merge_y"])
    assert np.array_equal(res["bl_x"], ref["bl_x"]) and np.array_equal(res["bl_y"], ref["bl_y"])


def test_placement_on_poisson_distances(gpu, orc, evolved):
    from dipper_amd import capi
    from tests.test_gpu_mash_place import _same_state
    n = len(evolved)
    gpu.set_msa_aa(capi.pack_aa_many(evolved))
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_POISSON)
    M = gpu.matrix()
    got = gpu.place_run(capi.SRC_MSA, n, dist_type=capi.DIST_POISSON)
    _same_state(got, orc.place_run(M), n)
