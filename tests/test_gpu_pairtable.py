"""GPU: the pair-table distance types 9 (TN93), 10 (LogDet) and 11 (paralinear) of nucleotide alignments against the
high-precision reference of tests/_pairtable_ref.py.

The counting body runs in the 32 x 32 tile of msa.hip (2 x 2 pairs per thread, 16-word = 512-site stages), so the shapes sit at
a word, a stage, a partial word quad and at tile edges 32 and 64.  Per case and type: the whole matrix under the reference's
rule (regular cells within 1e-11 relative + 1e-14 absolute, the exact NaN / +inf pattern, near-singular cells of type 9 skipped and
counted), a bitwise symmetric matrix, and the block hook, row-sharded ranks, a bootstrap replicate, both NJ plans,
divide-and-conquer and fixed-backbone placement bit for bit the one-rank result."""
import numpy as np
import pytest

from tests import _pairtable_ref as R, _util
from tests.test_gpu_msa_edges import _hook_shapes

pytestmark = pytest.mark.gpu

TYPES = R.TYPES

CASES = {}
for _L in (1, 31, 32, 33, 511, 512, 513, 1025):               # a word, a 16-word stage, a partial quad
    CASES[f"L{_L}"] = lambda L=_L: _util.msa_density(L, 33, 0.03)
for _n in (2, 3, 31, 32, 33, 63, 64, 65, 129):                 # tile edges 32 and 64, partial tiles
    CASES[f"n{_n}"] = lambda n=_n: _util.msa_density(2080, n, 0.03)
for _rate in (0.001, 0.3):
    CASES[f"scatter{_rate}"] = lambda r=_rate: _util.msa_density(2080, 65, r)
CASES["runs"] = lambda: _util.msa_density(2090, 65, 0.03, runs=True)
CASES["single_gaps"] = lambda: _util.msa_single_gaps(2080)
CASES["gc0.7"] = lambda: _util.msa_composition(2080, 65, 0.7)
CASES["gc0.3"] = lambda: _util.msa_composition(3000, 40, 0.3)
CASES["drift"] = lambda: R.msa_drift(2080, 40)

_SEQS, _REF, _GPU = {}, {}, {}


def _seqs(case):
    if case not in _SEQS:
        _SEQS[case] = CASES[case]()
    return _SEQS[case]


def _ref(case):
    if case not in _REF:
        _REF[case] = R.reference(_seqs(case))
    return _REF[case]


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def _upload(d, seqs):
    from dipper_amd import capi
    d.set_msa(capi.pack4_many(seqs), len(seqs[0]))


def _matrices(d, seqs):
    from dipper_amd import capi
    _upload(d, seqs)
    out = {}
    for dt in TYPES:
        d.dist_matrix(capi.SRC_MSA, dt)
        out[dt] = d.matrix()
    return out


def _fast(gpu, case):
    if case not in _GPU:
        _GPU[case] = _matrices(gpu, _seqs(case))
    return _GPU[case]


def _same_bits(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.where(np.isnan(a), 0, a).view(np.uint64), np.where(np.isnan(b), 0, b).view(np.uint64))


def test_constants():
    from dipper_amd import capi
    assert (capi.DIST_TN93, capi.DIST_LOGDET, capi.DIST_PARALINEAR) == (9, 10, 11)


@pytest.mark.parametrize("case", list(CASES))
def test_matrix_against_reference(gpu, case):
    ref = _ref(case)
    n = ref["n"]
    if case == "drift":
        # the composition drifts: row and column marginals differ in (at least half of) the cross-group pairs, and no table is
        # singular, so a body that labels the bases of one side wrongly shows in the determinant's sign
        h = n // 2
        cross = [R.margins(ref["F"][(r, c)]) for r in range(h, n) for c in range(h)]
        assert sum(rr != cc for _, rr, cc in cross) >= len(cross) / 2
        assert all(np.all(ref[t][0][np.tril_indices(n, -1)] == R.REGULAR) for t in TYPES)
    if case.startswith("gc"):
        lo = np.tril_indices(n, -1)
        assert np.isnan(ref[9][1][lo]).any() and np.isposinf(ref[10][1][lo]).any() and np.isnan(ref[11][1][lo]).any()
    M = _fast(gpu, case)
    for dt in TYPES:
        G = M[dt]
        assert G.shape == (n, n)
        assert _same_bits(G, G.T), (case, dt)
        assert np.all(np.diag(G) == 0), (case, dt)
        assert not np.isneginf(G).any(), (case, dt)
        R.check_matrix(G, ref, dt, case)


HOOK_CASES = [c for c in CASES if not c.startswith("n") or c in ("n65", "n129")]


@pytest.mark.parametrize("case", HOOK_CASES)
def test_block_hook_equals_matrix(gpu, case):
    """msa_dist_block (placement, --add, fixed-backbone placement) in both orientations: bit for bit the matrix off the diagonal"""
    M = _fast(gpu, case)
    n = len(_seqs(case))
    _upload(gpu, _seqs(case))
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
@pytest.mark.parametrize("case", ["gc0.7", "n129"])
def test_row_sharded_ranks_equal_one_rank(gpu, case, world):
    import dipper_amd
    M = _fast(gpu, case)
    d = dipper_amd.Dipper(0, virtual_world=world)
    try:
        P = _matrices(d, _seqs(case))
        for dt in TYPES:
            assert _same_bits(P[dt], M[dt]), (case, world, dt)
    finally:
        d.close()


def test_resample_equals_host_replicate(gpu):
    """after msa_resample the matrix is the matrix of an upload of the host-built replicate alignment"""
    from dipper_amd import capi
    from tests.test_gpu_bootstrap import replicate_seqs
    seqs = _seqs("runs")
    seed = 11
    want = _matrices(gpu, replicate_seqs(seqs, seed, 0))
    _upload(gpu, seqs)
    gpu.msa_resample(seed, 0)
    try:
        for dt in TYPES:
            gpu.dist_matrix(capi.SRC_MSA, dt)
            got = gpu.matrix()
            assert _same_bits(got, want[dt]), dt
            assert not _same_bits(got, _fast(gpu, "runs")[dt]), dt
    finally:
        gpu.msa_resample(seed, -1)


def test_rejected_types_and_message(gpu):
    """7 and 8 stay protein-only, 12 is unknown; the message names the valid set"""
    import dipper_amd
    from dipper_amd import capi
    _upload(gpu, _seqs("n33"))
    for dt in (7, 8, 12):
        with pytest.raises(dipper_amd.DipperError) as ei:
            gpu.dist_matrix(capi.SRC_MSA, dt)
        assert ei.value.code == -1 and "1-6, 9" in str(ei.value) and "11" in str(ei.value)
        with pytest.raises(dipper_amd.DipperError) as ei:
            gpu.msa_dist_block(0, 10, 10, dist_type=dt)
        assert ei.value.code == -1


def test_nj_plans_agree_on_paralinear_distances():
    """129 tips: the pruned and the streaming plan write the same merge log from the type-11 matrix"""
    import dipper_amd
    from dipper_amd import capi
    seqs = R.msa_drift(2080, 129, seed=1)
    logs = []
    for mode in (1, 0):
        d = dipper_amd.Dipper(0)
        try:
            d.set_nj_mode(mode)
            _upload(d, seqs)
            d.dist_matrix(capi.SRC_MSA, capi.DIST_PARALINEAR)
            M = d.matrix()
            assert np.all(np.isfinite(M)) and np.all(M[~np.eye(129, dtype=bool)] > 0)
            logs.append(d.nj_run())
        finally:
            d.close()
    a, b = logs
    assert a["iters"] == b["iters"] == 127
    for key in ("merge_x", "merge_y"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("bl_x", "bl_y"):
        assert _same_bits(a[key], b[key]), key
    assert a["last_d"] == b["last_d"]


def test_dc_run_tn93(gpu, orc):
    """divide-and-conquer at the smallest shape of test_gpu_dc.py: assignment blocks and cluster jobs take type 9, and two
    virtual ranks return the same arrays"""
    from dipper_amd import capi
    from tests.test_gpu_dc import _same_dc_state
    n, B, L = 60, 25, 1500
    rng = np.random.default_rng(n)
    seqs = _util.synth_alignment(rng, n, L, mean_bl=5e-3, lo=1e-4, hi=5e-2)
    _upload(gpu, seqs)
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_TN93)
    M = gpu.matrix()
    assert np.all(np.isfinite(M))
    got = gpu.dc_run(capi.SRC_MSA, n, B, dist_type=capi.DIST_TN93)
    ref = orc.dc_run(M, B, skip_last_backbone=1)
    _same_dc_state(got, ref, n, B)
    two = gpu.dc_run(capi.SRC_MSA, n, B, dist_type=capi.DIST_TN93, flags=capi.dc_virtual_ranks(2))
    _same_dc_state(two, ref, n, B)
    live = 4 * n - 4
    for key in ("cluster_id", "head", "e", "nxt", "belong", "len"):
        m = n if key == "cluster_id" else 2 * n if key == "head" else live
        assert np.array_equal(two[key][:m], got[key][:m]), key


def test_place_fixed_run_tn93(gpu, orc):
    """fixed-backbone placement at the smallest shape of test_gpu_place_fixed.py, against the oracle on the type-9 rows"""
    from dipper_amd import capi
    from tests import test_gpu_place_fixed as pf
    m, c = 3, 1
    pf.load_msa(gpu, orc, m, c)
    got = gpu.place_fixed_run(capi.SRC_MSA, capi.DIST_TN93)
    rows, _ = gpu.msa_dist_block(m, c, m, capi.DIST_TN93)
    assert np.all(np.isfinite(rows))
    pf.same(got, pf.oracle(orc, m, rows))
