"""GPU parity of the divide-and-conquer mode (dpr_dc_run) where tests/test_gpu_dc.py does not go: its eight tests share one regime
(gap-free alignments, finite distances well below 2, no exact ties, backbones of 25 tips and more, cluster sizes left to chance).
The check is that file's _same_dc_state everywhere: the whole state against orc.dc_run on the GPU's own matrix, bit for bit.  Every
test first asserts, on that same oracle result, that its input is in the regime it claims (tests/_dc_inputs.py; shown on the CPU with
the oracle's own distances by tests/test_dc_inputs.py), and prints it.

  sizes       clusters of exactly 1, 2, 31, 32, 33, 54, 55, 63, 64, 65 and 129 members in one run: dc_cluster_kernel<1> | <16> at
              64 | 65, the row tiles of the job list at 32 | 33 and 64 | 65, 10 + m columns at 64 | 65, odd and even row strides;
              distance types 2, 4 and 9 (the 64-tile, the 32-tile, the pair-table tile); a memory group per cluster; three ranks
  gapped      gaps, N and lower-case letters, shared deletions: the job front-end of the aligned distances beyond its fast path
  duplicates  70 and 33 exact copies of two backbone tips: equal candidates in the wave and LDS merge of dc_cluster_kernel<16>
  tiny        backbones of 3, 4 and 5 tips (-1 list entries: the -inf row of the scan, column ids of -1 in the job list), and of
              40 tips with 1, 64 and 65 queries (a chunk closed by its 64 entries, a partial query group)
  saturated   NaN, +inf and distances >= 2, an all-gap query, a backbone tip of N or of noise: equal to the oracle where it places
              everything below 2, DPR_ERR_NOCAND where it would split slot 0, and the context usable afterwards
  mash        Mash clusters of 8, 9, 64, 65, 503 and 504 members: a second row group, the 16-wavefront kernel, a second column job

What a one-line slip in the library does here (built and run, one at a time):
  dc_cluster_kernel<16> merges the wave winners by add alone, without "then the smallest position": 10 tests fail (every sizes
              case, both duplicates cases, the three mash cases);
  dc_table_build lets an absent list entry point at the chunk's first distance row instead of the row of -inf: both
              test_backbone_of_40_with_a_far_tip cases and one saturated case fail.  Nothing else can: an absent entry holds the path
              length 2.0, so the wrong candidate is distance - 2.0 and never exceeds a maximum that starts at 0 while distances stay
              below 2 (_dc_inputs.absent_entry_flips counts, from the oracle alone, the assignments that depend on it).
(A forced fast stage path in the job front-end of the aligned distances is no index-safe mutant: padding words then count as
matches, the counts pass the alignment length and index the distance tables out of range.)

Superset and subset: the superset's matrix comes from the GPU, the oracle's assignment on it trims the input, the subset is uploaded
again and its own matrix is what the oracle runs on."""
import numpy as np
import pytest

from tests import _dc_inputs as inp
from tests.test_gpu_dc import _same_dc_state

pytestmark = pytest.mark.gpu

NOCAND_TEXT = "no eligible edge with pendant length < 2"


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Entry:
    """a trimmed input: case, packed (the subset, as uploaded), n, M (the GPU's matrix of the subset), ref (the oracle's run on M)"""


def _same_matrix(a, b):
    return np.array_equal(np.tril(a, -1), np.tril(b, -1), equal_nan=True)


def msa_entry(gpu, orc, key, make, dist_type=2):
    """the trimmed input of a builder under a distance type, computed once per module"""
    def build():
        from dipper_amd import capi
        x = Entry()
        x.case = case = make()
        gpu.set_msa(capi.pack4_many(case.seqs), case.L)
        gpu.dist_matrix(capi.SRC_MSA, dist_type)
        M = gpu.matrix()
        keep = case.trim(inp.assignment(orc, M, case.B, case.skip_last))
        x.seqs = [case.seqs[t] for t in keep]
        x.packed, x.n, x.dist_type = capi.pack4_many(x.seqs), len(keep), dist_type
        load(gpu, x)
        gpu.dist_matrix(capi.SRC_MSA, dist_type)
        x.M = gpu.matrix()
        assert _same_matrix(x.M, inp.submatrix(M, keep))                     # distances are pairwise
        x.ref = orc.dc_run(x.M, case.B, skip_last_backbone=case.skip_last)
        return x
    return cached((key, dist_type), build)


def load(gpu, x):
    gpu.set_msa(x.packed, x.case.L)


def run(gpu, x, extra_flags=0):
    from dipper_amd import capi
    return gpu.dc_run(capi.SRC_MSA, x.n, x.case.B, dist_type=x.dist_type, flags=x.case.flags() | extra_flags)


# ---- cluster sizes at the seams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist_type,mode", [(2, "plain"), (4, "plain"), (9, "plain"), (2, "budget 0"), (2, "3 ranks")])
def test_size_families(gpu, orc, monkeypatch, dist_type, mode):
    from dipper_amd import capi
    x = msa_entry(gpu, orc, "sizes", inp.size_families, dist_type)
    B = x.case.B
    assert x.n == 729
    inp.size_conditions(x.ref, B)
    want_table = inp.table_stats(orc.dc_run(x.M, B, skip_last_backbone=x.case.skip_last, backbone_only=True), B)
    assert want_table["max_leaves"] == inp.MAX_LEAVES and want_table["max_entries"] == inp.MAX_ENTRIES      # chunks closed either way
    load(gpu, x)
    if mode == "budget 0":
        monkeypatch.setenv("DPR_DC_BUDGET_MB", "0")
    got = run(gpu, x, capi.dc_virtual_ranks(3) if mode == "3 ranks" else 0)
    table = gpu.dc_table_stats()
    print(f"sizes type {dist_type} {mode}: cluster sizes {inp.sizes_of(x.ref['cluster_id'], B)}, largest add {x.ref['trace'][2:, 2].max():.3g}, "
          f"table {table}, groups {got['stats']['groups']}, jobs {got['stats']['jobs']}")
    assert table == {k: want_table[k] for k in table}
    _same_dc_state(got, x.ref, x.n, B)
    assert got["stats"]["max_cluster"] == 129 and got["stats"]["clusters"] == 11
    if mode == "budget 0":
        assert got["stats"]["groups"] == got["stats"]["clusters"]


# ---- gaps and ambiguity codes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist_type", [2, 4])
@pytest.mark.parametrize("L", [500, 1000, 1100])
def test_gapped(gpu, orc, L, dist_type):
    x = msa_entry(gpu, orc, ("gapped", L), lambda: inp.gapped(L), dist_type)
    inp.gapped_conditions(orc, x.seqs, L, x.ref, x.case.B)
    load(gpu, x)
    got = run(gpu, x)
    print(f"gapped L {L} type {dist_type}: n {x.n}, cluster sizes {inp.sizes_of(x.ref['cluster_id'], x.case.B)[-5:]} (largest five)")
    _same_dc_state(got, x.ref, x.n, x.case.B)


# ---- exact ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_duplicates(gpu, orc, world):
    from dipper_amd import capi
    x = msa_entry(gpu, orc, "duplicates", inp.duplicates)
    inp.duplicate_conditions(x.M, x.ref, x.case.B)
    load(gpu, x)
    got = run(gpu, x, capi.dc_virtual_ranks(world) if world > 1 else 0)
    zero = int(np.count_nonzero(x.ref["trace"][x.n - 103:, 2] == 0.0))
    print(f"duplicates world {world}: n {x.n}, cluster sizes {inp.sizes_of(x.ref['cluster_id'], x.case.B)[-3:]} (largest three), {zero} of 103 copies placed with add == 0")
    _same_dc_state(got, x.ref, x.n, x.case.B)


# ---- tiny backbones, and the chunk that closes at 64 entries ---------------------------------------------------------------------------
@pytest.mark.parametrize("skip_last", [0, 1])
@pytest.mark.parametrize("B", [3, 4, 5])
def test_tiny_backbone(gpu, orc, B, skip_last):
    x = msa_entry(gpu, orc, ("tiny", B, skip_last), lambda: inp.tiny_backbone(B, skip_last))
    bb = orc.dc_run(x.M, B, skip_last_backbone=skip_last, backbone_only=True)
    absent = inp.tiny_conditions(bb, x.ref, B, skip_last)
    load(gpu, x)
    got = run(gpu, x)
    table = gpu.dc_table_stats()
    print(f"backbone {B} skip_last {skip_last}: n {x.n}, {absent} absent list entries, cluster sizes {inp.sizes_of(x.ref['cluster_id'], B)}, table {table}")
    want = inp.table_stats(bb, B)
    want = {k: want[k] for k in table}
    assert table == want and table["chunks"] == 1 and table["entries"] == 2 * B - 2
    _same_dc_state(got, x.ref, x.n, B)


@pytest.mark.parametrize("B,far", inp.TINY_FAR)
def test_tiny_backbone_with_a_far_tip(gpu, orc, B, far):
    """where an absent list entry must read the row of -inf and nothing else: see _dc_inputs.far_conditions"""
    x = msa_entry(gpu, orc, ("tiny far", B, far), lambda: inp.tiny_backbone(B, 0, far=far))
    bb = orc.dc_run(x.M, B, skip_last_backbone=0, backbone_only=True)
    hits = inp.far_conditions(x.M, bb, x.ref, B)
    load(gpu, x)
    got = run(gpu, x)
    print(f"backbone {B}, tip {far} far: n {x.n}, {hits} queries beyond 2.1 from the first row's tip, cluster sizes {inp.sizes_of(x.ref['cluster_id'], B)}")
    assert gpu.dc_table_stats()["chunks"] == 1
    _same_dc_state(got, x.ref, x.n, B)


@pytest.mark.parametrize("nq", [1, 64, 65])
def test_backbone_of_40(gpu, orc, nq):
    x = msa_entry(gpu, orc, ("bb40", nq), lambda: inp.backbone40(nq))
    B = x.case.B
    assert x.n == B + nq
    inp.placed_everything(x.ref, x.n)
    load(gpu, x)
    got = run(gpu, x)
    table = gpu.dc_table_stats()
    print(f"backbone 40, {nq} queries: table {table}")
    want = inp.table_stats(orc.dc_run(x.M, B, skip_last_backbone=x.case.skip_last, backbone_only=True), B)
    want = {k: want[k] for k in table}
    assert table == want
    assert table["chunks"] == 2 and table["max_entries"] == 64 and table["entries"] == 78
    _same_dc_state(got, x.ref, x.n, B)


@pytest.mark.parametrize("far", inp.FAR40)
def test_backbone_of_40_with_a_far_tip(gpu, orc, far):
    """a backbone tip of noise that is the first distance row of a scan chunk: where an absent list entry must read the row of
    -inf and no other (on distances below 2 any row gives the same result: _dc_inputs.absent_entry_flips)"""
    x = msa_entry(gpu, orc, ("bb40 far", far), lambda: inp.backbone40(65, far=far))
    B = x.case.B
    inp.placed_everything(x.ref, x.n)
    assert np.all(x.ref["trace"][B:, 2] < 2.0)
    bb = orc.dc_run(x.M, B, skip_last_backbone=1, backbone_only=True)
    assert far in inp.table_stats(bb, B)["first_leaves"]
    flips = inp.absent_entry_flips(bb, B, x.M, 1)
    print(f"backbone 40, tip {far} far: {flips} of 65 assignments depend on the row of -inf")
    assert flips >= 5
    load(gpu, x)
    _same_dc_state(run(gpu, x), x.ref, x.n, B)


def test_table_stats_getter():
    """dpr_get_dc_table_stats: argument errors, zeros before the first dc_run of a context"""
    import ctypes as C

    import dipper_amd
    from dipper_amd import capi
    L = capi.load_library()
    out = (C.c_int64 * 4)()
    assert L.dpr_get_dc_table_stats(None, out) == -1                         # DPR_ERR_ARG
    d = dipper_amd.Dipper(0)
    try:
        assert L.dpr_get_dc_table_stats(d.h, None) == -1
        assert d.dc_table_stats() == dict(entries=0, chunks=0, max_entries=0, max_leaves=0)
    finally:
        d.close()


# ---- saturated and empty pairs -----------------------------------------------------------------------------------------------------------
def saturated_entry(gpu, orc, param):
    L, seed, variant, redrawn = param
    x = msa_entry(gpu, orc, ("saturated",) + tuple(param), lambda: inp.saturated(L, seed, variant, redrawn))
    if not hasattr(x, "regime"):
        inp.saturated_conditions(x.M, x.case.B)
        x.regime = inp.regime(x.M, x.ref, x.case.B)
    return x


def a_placeable_entry(gpu, orc):
    for param in inp.SATURATED:
        x = saturated_entry(gpu, orc, param)
        if x.regime == "placeable":
            return x
    raise AssertionError("no placeable input among the saturated ones")


@pytest.mark.parametrize("param", inp.SATURATED, ids=lambda p: "-".join(str(v) for v in p))
def test_saturated(gpu, orc, param):
    """The branch is picked from the oracle's result on the GPU's matrix, never from the library's."""
    from dipper_amd import capi
    x = saturated_entry(gpu, orc, param)
    B = x.case.B
    rows = x.M[B:, :B]
    print(f"saturated {param}: {x.regime}; {int(np.isnan(rows).sum())} NaN, {int(np.isinf(rows).sum())} inf, "
          f"{int(np.count_nonzero(np.isfinite(rows) & (rows >= 2)))} finite >= 2; {int(np.count_nonzero(x.ref['cluster_id'][B:] == 0))} queries assigned to slot 0")
    assert x.regime in ("placeable", "no candidate")
    load(gpu, x)
    if x.regime == "placeable":
        _same_dc_state(run(gpu, x), x.ref, x.n, B)
        return
    for extra in (0, capi.dc_virtual_ranks(2)):                              # the error must arrive, not a merged half-state
        with pytest.raises(capi.DipperError) as ei:
            run(gpu, x, extra)
        assert ei.value.code == -4 and NOCAND_TEXT in str(ei.value), str(ei.value)
        good = a_placeable_entry(gpu, orc)                                   # the context is still usable
        load(gpu, good)
        _same_dc_state(run(gpu, good), good.ref, good.n, good.case.B)
        load(gpu, x)


def test_saturated_inputs_meet_both_regimes(gpu, orc):
    seen = {param: saturated_entry(gpu, orc, param).regime for param in inp.SATURATED}
    print("saturated regimes on the GPU's matrices:", seen)
    assert set(seen.values()) == {"placeable", "no candidate"}, seen


# ---- reads -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [1, 2, 3])
def test_mash_families(gpu, orc, which):
    from dipper_amd import capi

    def matrix_of(reads):
        gpu.set_reads(reads)
        gpu.sketch(k=15, S=1000, fetch=False)
        gpu.dist_matrix(capi.SRC_MASH, 0, 15)
        return gpu.matrix()

    def build():
        x = Entry()
        x.case = case = inp.mash_families(which)
        M = matrix_of(case.seqs)
        keep = case.trim(inp.assignment(orc, M, case.B, 0))
        x.reads, x.n = [case.seqs[t] for t in keep], len(keep)
        x.M = matrix_of(x.reads)
        assert _same_matrix(x.M, inp.submatrix(M, keep))
        x.ref = orc.dc_run(x.M, case.B, skip_last_backbone=0)
        return x
    x = cached(("mash", which), build)
    B = x.case.B
    assert x.n == B + sum(x.case.sizes)
    inp.mash_conditions(x.ref, B, x.case.sizes)
    gpu.set_reads(x.reads)
    gpu.sketch(k=15, S=1000, fetch=False)
    got = gpu.dc_run(capi.SRC_MASH, x.n, B, k=15)
    print(f"mash case {which}: n {x.n}, cluster sizes {inp.sizes_of(x.ref['cluster_id'], B)}, jobs {got['stats']['jobs']}")
    _same_dc_state(got, x.ref, x.n, B)
    assert got["stats"]["max_cluster"] == max(x.case.sizes) and got["stats"]["clusters"] == len(x.case.sizes)
    assert got["stats"]["jobs"] == inp.jobs_expected(x.case.sizes)           # (case 3: one more than its row groups)
