"""GPU: the aligned-sequence pair kernels (msa.hip) against the oracle at every tile, stage and gap edge.

The type-1/2 tile (64 x 64) has data-dependent paths: clean 16-word stages that skip the not-a-base planes, per-wavefront word
masks that pick a clean, one-sided or two-sided body, quad-word staging with a partial last quad, a full (useful, match) table up
to 1 024 sites and a 16-row band table above, and a per-sequence stage bitmap in which stages from 63 on share bit 63.  Types 3-6
run on a 32 x 32 tile with their own counters.  Every builder of tests/_util.py is checked for all six types under one rule
(_util.assert_msa_dist): the matrix path against the oracle, the block hook in both orientations against the matrix, the kernel
with the fast paths and the band table switched off against the kernel with them, and row-sharded ranks against one rank."""
import os

import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu

TYPES = (1, 2, 3, 4, 5, 6)

CASES = {}
for _L in (2080, 2048, 2090):                              # W32 = 65 (L % 32 == 0, a partial stage), no padding, W32 = 2 mod 4
    CASES[f"single_gaps_L{_L}"] = (lambda L=_L: _util.msa_single_gaps(L))
for _L in (32256, 32768, 33000, 40961):                    # 63 stages, 64 without padding, 65, 81 with L % 32 == 1
    CASES[f"stage63_L{_L}"] = (lambda L=_L: _util.msa_stage63_gaps(L))
for _L in (1024, 1025, 3000):                              # the full table, the band just above it, the band
    CASES[f"band_L{_L}"] = (lambda L=_L: _util.msa_band_edges(L))
for _L in (1, 31, 32, 33, 511, 512, 513):                  # one word; around the first use of the stage bitmap
    CASES[f"short_L{_L}"] = (lambda L=_L: _util.msa_density(L, 33, 0.03))
for _rate in (0.001, 0.03, 0.3):
    CASES[f"scatter{_rate}"] = (lambda r=_rate: _util.msa_density(2080, 65, r))
CASES["runs0.03"] = lambda: _util.msa_density(2090, 65, 0.03, runs=True)
for _n in (2, 3, 31, 32, 33, 63, 64, 65, 129):
    CASES[f"n{_n}"] = (lambda n=_n: _util.msa_density(2080, n, 0.03))
CASES["gc70"] = lambda: _util.msa_composition(2080, 65, 0.7)
CASES["at70"] = lambda: _util.msa_composition(3000, 40, 0.3)

_SEQS, _ORC, _GPU = {}, {}, {}


def _seqs(case):
    if case not in _SEQS:
        _SEQS[case] = CASES[case]()
    return _SEQS[case]


def _packed(case):
    from dipper_amd import capi
    return capi.pack4_many(_seqs(case))


def _oracle(orc, case, dt):
    """the oracle's strict lower triangle, once per alignment and type"""
    if (case, dt) not in _ORC:
        s = _seqs(case)
        _ORC[case, dt] = orc.msa_dist_lower_mt(orc.pack4_many(s), len(s[0]), dt)
    return _ORC[case, dt]


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()
    print("\nlargest ulp distance from the oracle per type:", dict(sorted(_util.MSA_ULP_SEEN.items())))


def _matrices(d, case, env=None):
    """the uploaded alignment's six matrices (a fresh upload; env: switches read by the upload)"""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = _seqs(case)
        d.set_msa(_packed(case), len(s[0]))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    from dipper_amd import capi
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
def test_matrix_against_oracle(gpu, orc, case):
    """diagonal tiles and mirrored lower tiles of dist_matrix, every type, against the oracle"""
    M = _fast(gpu, case)
    n = len(_seqs(case))
    lo = np.tril_indices(n, -1)
    for dt in TYPES:
        assert _same_bits(M[dt], M[dt].T), (case, dt)
        assert np.all(np.diag(M[dt]) == 0), (case, dt)
        _util.assert_msa_dist(M[dt][lo], _oracle(orc, case, dt)[lo], dt, case)


def _hook_shapes(n):
    for row0 in (0, 1, 31, 63, 64, 65):
        for nrows in (1, 33, 64, 65):
            if row0 + nrows > n:
                continue
            for ncols in sorted({1, row0, n}):
                if ncols >= 1:
                    yield row0, nrows, ncols


HOOK_CASES = [c for c in CASES if not c.startswith("n") or c in ("n65", "n129")]


@pytest.mark.parametrize("case", HOOK_CASES)
def test_block_hook_equals_matrix(gpu, case):
    """msa_dist_block (placement, --add and the divide-and-conquer assignment call it) in both orientations: bit for bit the
    matrix, except the diagonal, where the hook has no rule and returns the pair's own distance"""
    M = _fast(gpu, case)
    s = _seqs(case)
    n = len(s)
    gpu.set_msa(_packed(case), len(s[0]))
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
            if on.any():      # the pair of a sequence with itself: 0 (or NaN when it has no base at all) under either sign
                diag = blk[r[on], row0 + r[on]]
                assert np.all((diag == 0) | np.isnan(diag)), (case, dt, diag)


@pytest.mark.parametrize("case", list(CASES))
def test_fast_paths_and_band_off_equal(gpu, case):
    """DPR_MSA_NO_FAST (no stage bitmap: every word takes the seven-operation body) and DPR_MSA_NO_BAND (no band table) set
    before the upload: every type bit for bit the same"""
    M = _fast(gpu, case)
    P = _matrices(gpu, case, {"DPR_MSA_NO_FAST": "1", "DPR_MSA_NO_BAND": "1"})
    for dt in TYPES:
        assert _same_bits(P[dt], M[dt]), (case, dt)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("case", ["single_gaps_L2080", "scatter0.03"])
def test_row_sharded_ranks_equal_one_rank(gpu, case, world):
    """row-sharded virtual ranks (each rank's pair tiles over its own rows) give the one-rank matrix bit for bit, every type"""
    import dipper_amd
    M = _fast(gpu, case)
    s = _seqs(case)
    d = dipper_amd.Dipper(0, virtual_world=world)
    try:
        d.set_msa(_packed(case), len(s[0]))
        from dipper_amd import capi
        for dt in TYPES:
            d.dist_matrix(capi.SRC_MSA, dt)
            assert _same_bits(d.matrix(), M[dt]), (case, world, dt)
    finally:
        d.close()
