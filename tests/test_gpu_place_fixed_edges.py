"""GPU parity of the placement on a fixed backbone (dpr_place_fixed_set / _run) where tests/test_gpu_place_fixed.py cannot go:
its oracle, orc_place_run, has a (slot 0, add 2) default tuple the definition does not have, so that file keeps every distance
<= 0.5 and every backbone <= 300 tips.  Here the reference is the definition itself (tests/_pfix_ref.py, NumPy float64, held
against the oracle by tests/test_pfix_ref.py), fed with the distance rows the GPU itself used, and the comparison is bit for bit
(NaN positions equal whatever their payload):

  divergent   queries far from the backbone, finite distances up to JC 3.76: add >= 2, every clamp branch of the scan on
              winning edges, winning edges of length 0, short and long (up to 1.0) backbone edges;
  saturated   +inf rows (p = 0.75 exactly under JC), NaN rows (p > 0.75, no common site), rows mixing them with finite values,
              at positions 0, 63, 64 and last of a batch, batch sizes 0 / 1 / 64 / 100;
  mash        reads that share no k-mer with the backbone;
  chunks      backbones of 1 500 and 6 000 tips: 47 and 188 scan chunks, so the 16 wavefronts of the reduce step loop 3 and 12
              times (its unrolled body of 4 and the remainder), ties across every chunk.

Every test first asserts from the rows and the reference alone that its input is in the regime it claims (tests/_pfix_inputs.py).
Both scan forms run everywhere (DPR_PFIX_CARRY unset and 1), Mash input included."""
import hashlib

import numpy as np
import pytest

from tests import _jplace, _pfix_inputs, _pfix_ref
from tests.conftest import dirty_device_memory
from tests.test_gpu_mash_place import _reads

pytestmark = pytest.mark.gpu
SITES = _pfix_inputs.SITES


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


def backbone(m, kind):
    return cached(("nwk", m, kind), lambda: _jplace.random_backbone(np.random.default_rng(100 + m), m, kind))


def ref_state(orc, nwk, m):
    """the importer's state with its closest lists (sized for m + 1 tips: node ids do not enter the arithmetic)"""
    def make():
        st, _ = _jplace.backbone_arrays(orc, nwk, m + 1)
        orc.place_init_lists(m + 1, m, st)
        return st
    return cached(("state", nwk), make)


def reference(orc, nwk, m, rows):
    """the reference for these rows, computed once per (backbone, rows); the key is a digest, not the rows"""
    return cached(("ref", nwk, hashlib.sha1(rows.tobytes()).digest()), lambda: _pfix_ref.place(ref_state(orc, nwk, m), m, rows))


def slim(p, keep):
    """a cached reference of a large case keeps the winners and the `add` rows of the engineered queries (what the conditions
    and the comparison read), not the (query, edge) tables and masks: ~130 MB at 512 x 11 998"""
    if not isinstance(p.add, dict):
        p.add = {q: p.add[q].copy() for q in keep}
        p.frac = p.took = None
    return p


def load_msa(d, orc, nwk, seqs, m, batch):
    from dipper_amd import capi
    n = len(seqs)
    d.set_msa(cached(("p4", id(seqs)), lambda: (seqs, capi.pack4_many(seqs)))[1], SITES)
    d.set_place_fixed_batch(batch)
    d.place_fixed_set(m, n, cached(("arrays", nwk, n), lambda: _jplace.backbone_arrays(orc, nwk, n)[0]))


def both_forms(d, monkeypatch, p, dist_type, what, mash_k=None):
    from dipper_amd import capi
    run = (lambda: d.place_fixed_run(capi.SRC_MSA, dist_type)) if mash_k is None else (lambda: d.place_fixed_run(capi.SRC_MASH, 0, k=mash_k))
    monkeypatch.delenv("DPR_PFIX_CARRY", raising=False)
    _pfix_ref.assert_same(run(), p, what + " re-evaluate")
    monkeypatch.setenv("DPR_PFIX_CARRY", "1")
    _pfix_ref.assert_same(run(), p, what + " carry")


# ---- divergent queries, finite distances --------------------------------------------------------------------------------------------
# (m, long edges, dist_type, seed, mean branch length of the backbone sequences, order of the query kinds): seeds chosen on the CPU so
# that the conditions hold.  A 6-tip backbone has ten edges, and a long edge takes a clamp only from distances that differ by more
# than its length: these cases get their winning edges from more queries of the far kind (2), whose JC distances scatter most.
EVEN, FAR = (0, 1, 2, 3), (0, 2, 2, 1, 2, 2, 3, 2)
DIVERGENT = [(6, False, 2, 28, 6e-3, FAR), (6, True, 2, 197, 0.2, FAR), (40, False, 2, 1, 6e-3, EVEN), (40, False, 1, 109, 5e-2, EVEN),
             (300, False, 2, 6, 6e-3, EVEN)]


# p-distances are multiples of 1/200 and scatter too little for that: these inputs evolve on the backbone tree itself
# (_pfix_inputs.divergent_on_tree).  (m, seed, clamp branches not asked of WINNING edges)
DIVERGENT_P = [(6, 46, ("dis1<0", "dis2>L")), (300, 11, ())]


@pytest.mark.parametrize("m,seed,not_on_winners", DIVERGENT_P)
def test_divergent_p_distances(gpu, orc, monkeypatch, m, seed, not_on_winners):
    """`dis1 < 0` (with it `dis2 > L`) on a winning edge of the 6-tip backbone is not asked.  On an edge where it fires the query
    is closer to the lists of the `belong` side than the edge is long, and then an edge on that side has a pendant length no
    larger: for a cherry below the edge, add = dis2 - L on the edge and dis2 - L - (the leaf's length) on the leaf's edge, an
    exact tie for leaves of length 0, which the lower slot (the leaf's: post-order) wins.  Larger backbones get past this
    because a closest list holds five leaves, so the two edges see different leaves; with 6 tips every list holds every tip of its
    side.  Under JC the tie is broken either way by the last bit of the logarithms; under the p-distance it is exact.  Beyond
    the argument: 6 000 rows of arbitrary multiples of 1/200 on each of 400 seeded 6-tip backbones, and 8 000 generated inputs,
    gave no such winner.  Everything else is asserted, and the comparison with the reference runs on all 120 queries."""
    c = 120
    nwk = _pfix_inputs.divergent_backbone(m, seed, False)
    seqs = cached(("divp", m, seed), lambda: _pfix_inputs.divergent_on_tree(m, c, seed, nwk))
    load_msa(gpu, orc, nwk, seqs, m, 64)
    rows, _ = gpu.msa_dist_block(m, c, m, 1)
    p = reference(orc, nwk, m, rows)
    _pfix_inputs.divergent_conditions(p, rows, 1, not_on_winners)
    both_forms(gpu, monkeypatch, p, 1, f"divergent p-distance m {m}")


@pytest.mark.parametrize("m,long_edges,dist_type,seed,mean_bl,kinds", DIVERGENT)
def test_divergent_finite_distances(gpu, orc, monkeypatch, m, long_edges, dist_type, seed, mean_bl, kinds):
    c = 120
    nwk = _pfix_inputs.divergent_backbone(m, seed, long_edges)
    seqs = cached(("div", m, long_edges, seed, kinds), lambda: _pfix_inputs.divergent(m, c, seed, mean_bl, nwk, orc, kinds))
    load_msa(gpu, orc, nwk, seqs, m, 64)
    rows, _ = gpu.msa_dist_block(m, c, m, dist_type)
    p = reference(orc, nwk, m, rows)
    _pfix_inputs.divergent_conditions(p, rows, dist_type)
    both_forms(gpu, monkeypatch, p, dist_type, f"divergent m {m}")


# ---- saturated and empty pairs -----------------------------------------------------------------------------------------------------
C_SAT = 130
POSITIONS = {"plain": {"inf": 0, "nan": 63, "gaps": 64, "clade": C_SAT - 1},
             "gapped": {"half": 0, "gaps": 63, "inf": 64, "nan": C_SAT - 1}}


def saturated_input(orc, m, variant):
    return cached(("sat", m, variant), lambda: _pfix_inputs.engineered(m, C_SAT, 400 + m, backbone(m, "random"), orc, gapped=variant == "gapped",
                                                                        positions=POSITIONS[variant]))


@pytest.mark.parametrize("batch", [0, 1, 64, 100])
@pytest.mark.parametrize("variant", ["plain", "gapped"])
@pytest.mark.parametrize("m", [40, 300])
def test_saturated_and_empty_pairs(gpu, orc, monkeypatch, m, variant, batch):
    """+inf against everybody (best add +inf, frac NaN, the lowest eligible slot), NaN against everybody (add 0 on every edge), +inf
    against one clade only, NaN against every other tip; 130 queries are no multiple of the 64 of a workgroup"""
    nwk, inp = backbone(m, "random"), saturated_input(orc, m, variant)
    load_msa(gpu, orc, nwk, inp.seqs, m, batch)
    rows, _ = gpu.msa_dist_block(m, C_SAT, m, 2)
    p = reference(orc, nwk, m, rows)
    _pfix_inputs.engineered_conditions(inp, p, rows)
    both_forms(gpu, monkeypatch, p, 2, f"m {m} {variant} batch {batch}")


def test_saturated_rows_in_poisoned_memory(orc, monkeypatch):
    """device memory full of 0xFF (NaN as fp64) before the context's allocations: the answer is the reference's all the same"""
    import dipper_amd
    from dipper_amd import capi
    m, variant = 40, "plain"
    nwk, inp = backbone(m, "random"), saturated_input(orc, m, variant)
    capi.load_library()
    dirty_device_memory(2 << 30, 0xFF)
    d = dipper_amd.Dipper(0)
    try:
        load_msa(d, orc, nwk, inp.seqs, m, 64)
        rows, _ = d.msa_dist_block(m, C_SAT, m, 2)
        p = reference(orc, nwk, m, rows)
        _pfix_inputs.engineered_conditions(inp, p, rows)
        both_forms(d, monkeypatch, p, 2, "poisoned")
    finally:
        d.close()


# ---- unrelated reads under Mash ----------------------------------------------------------------------------------------------------
def test_mash_reads_that_share_no_kmer(gpu, orc, monkeypatch):
    from dipper_amd import capi
    m, c = 40, 70
    rng = np.random.default_rng(77)
    reads = _reads(rng, m + c, 1500, 2500)
    alien = [m + 0, m + 5, m + 63, m + 64, m + c - 1]
    for q, r in zip(alien, _reads(rng, len(alien), 1500, 2500, related=False)):
        reads[q] = r
    nwk = backbone(m, "random")
    gpu.set_reads(reads)
    gpu.sketch(k=15, S=1000, fetch=False)
    gpu.dist_matrix(capi.SRC_MASH, 0, 15)
    rows = np.ascontiguousarray(gpu.matrix()[m:, :m])
    gpu.set_place_fixed_batch(64)
    gpu.place_fixed_set(m, m + c, _jplace.backbone_arrays(orc, nwk, m + c)[0])
    # the regime: the unrelated rows hold the kernel's maximum (or a value that is not finite) in every cell, the others do not
    top = np.nanmax(np.where(np.isfinite(rows), rows, -np.inf))
    is_alien = np.zeros(c, dtype=bool)
    is_alien[[q - m for q in alien]] = True
    assert np.all(~np.isfinite(rows[is_alien]) | (rows[is_alien] == top))
    assert np.all(rows[~is_alien] < top) and top >= 0.3
    p = reference(orc, nwk, m, rows)
    both_forms(gpu, monkeypatch, p, 0, "mash", mash_k=15)


# ---- more chunks than the reduce step has wavefronts ----------------------------------------------------------------------------------
C_BIG = 512            # (200 ordinary queries give ~80 distinct winning slots on these backbones: raised to the most allowed)
BIG = {"gaps": 0, "inf": 63, "tip2": 64, "tiplast": C_BIG - 1}


@pytest.mark.parametrize("batch", [64, 0])
# (seed and mean branch length of the alignment chosen on the CPU; the test prints the number of distinct winning slots)
@pytest.mark.parametrize("m,kind,min_chunks,seed,mean_bl", [(1500, "random", 47, 6, 5e-2), (1500, "caterpillar", 47, 5, 5e-2), (6000, "random", 188, 6500, 2e-2)])
def test_many_chunks(gpu, orc, monkeypatch, m, kind, min_chunks, seed, mean_bl, batch):
    """>= 47 chunks: every wavefront of the reduce step takes three; >= 188: its unrolled body and the remainder both run.  The
    all-NaN query ties at add = 0 on every edge of every chunk and the all-inf one at +inf: the globally lowest eligible slot."""
    assert (2 * m - 2 + 63) // 64 >= min_chunks and min_chunks > 16 * (2 if m == 1500 else 4)
    nwk = backbone(m, kind)
    inp = cached(("big", m, kind), lambda: _pfix_inputs.engineered(m, C_BIG, seed, nwk, orc, positions=BIG, mean_bl=mean_bl, near_tips=True))
    load_msa(gpu, orc, nwk, inp.seqs, m, batch)
    rows, _ = gpu.msa_dist_block(m, C_BIG, m, 2)
    p = slim(reference(orc, nwk, m, rows), inp.at.values())
    _pfix_inputs.engineered_conditions(inp, p, rows)
    distinct = _pfix_inputs.chunk_conditions(p, m)
    print(f"many chunks: m {m} {kind}, {C_BIG} queries, {distinct} distinct winning slots")
    both_forms(gpu, monkeypatch, p, 2, f"m {m} {kind} batch {batch}")
