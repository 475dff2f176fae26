"""The inputs of tests/test_gpu_dc_edges.py sit where that file needs them -- shown with the oracle's own distances
(orc.msa_dist_lower_mt for alignments, orc.sketch and orc.mash_dist_row for reads), on the CPU.  Each builder of tests/_dc_inputs.py
is run, trimmed by the oracle's assignment, and its condition asserted on the oracle's run of the subset; trimming itself is shown to
be sound: the oracle's cluster_id on the subset is the superset's, restricted."""
import numpy as np
import pytest

from tests import _dc_inputs as inp

JC = 2


def msa_matrix(orc, seqs, L):
    D = orc.msa_dist_lower_mt(orc.pack4_many(seqs), L, JC)
    return D + D.T


def mash_matrix(orc, reads, k=15, S=1000):
    sk = np.array([orc.sketch(orc.pack2(r), len(r), k, S) for r in reads])
    D = np.zeros((len(reads), len(reads)))
    for r in range(1, len(reads)):
        D[r, :r] = orc.mash_dist_row(sk, k, r, r)
    return D + D.T


def trimmed(orc, case, M):
    """(kept tips, their matrix, the oracle's run on it); the assignment of the subset is the superset's, restricted"""
    cl = inp.assignment(orc, M, case.B, case.skip_last)
    keep = case.trim(cl)
    assert np.array_equal(keep[:case.B], np.arange(case.B))
    Ms = inp.submatrix(M, keep)
    ref = orc.dc_run(Ms, case.B, skip_last_backbone=case.skip_last)
    assert np.array_equal(ref["cluster_id"], cl[keep])
    return keep, Ms, ref


def test_size_families(orc):
    case = inp.size_families()
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, case.L))
    assert len(keep) == 729
    inp.size_conditions(ref, case.B)


@pytest.mark.parametrize("L", [500, 1000, 1100])
def test_gapped(orc, L):
    case = inp.gapped(L)
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, L))
    inp.gapped_conditions(orc, [case.seqs[t] for t in keep], L, ref, case.B)
    assert len(keep) >= 400


def test_duplicates(orc):
    case = inp.duplicates()
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, case.L))
    inp.duplicate_conditions(Ms, ref, case.B)


@pytest.mark.parametrize("skip_last", [0, 1])
@pytest.mark.parametrize("B", [3, 4, 5])
def test_tiny_backbone(orc, B, skip_last):
    case = inp.tiny_backbone(B, skip_last)
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, case.L))
    bb = orc.dc_run(Ms, B, skip_last_backbone=skip_last, backbone_only=True)
    absent = inp.tiny_conditions(bb, ref, B, skip_last)
    print(f"backbone {B} skip_last {skip_last}: n {len(keep)}, {absent} absent list entries, sizes {inp.sizes_of(ref['cluster_id'], B)}")


@pytest.mark.parametrize("B,far", inp.TINY_FAR)
def test_tiny_backbone_with_a_far_tip(orc, B, far):
    case = inp.tiny_backbone(B, 0, far=far)
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, case.L))
    bb = orc.dc_run(Ms, B, skip_last_backbone=0, backbone_only=True)
    print(f"backbone {B}, tip {far} far: n {len(keep)}, {inp.far_conditions(Ms, bb, ref, B)} queries beyond 2.1 from the first row's tip")


@pytest.mark.parametrize("far", inp.FAR40)
def test_backbone40_with_a_far_tip(orc, far):
    case = inp.backbone40(65, far=far)
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, case.L))
    inp.placed_everything(ref, len(keep))
    assert np.all(ref["trace"][40:, 2] < 2.0)
    bb = orc.dc_run(Ms, 40, skip_last_backbone=1, backbone_only=True)
    assert far in inp.table_stats(bb, 40)["first_leaves"]
    flips = inp.absent_entry_flips(bb, 40, Ms, 1)
    print(f"backbone 40, tip {far} far: {flips} of 65 assignments depend on the row of -inf")
    assert flips >= 5


@pytest.mark.parametrize("nq", [1, 64, 65])
def test_backbone40(orc, nq):
    case = inp.backbone40(nq)
    keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, case.L))
    assert len(keep) == 40 + nq
    inp.placed_everything(ref, len(keep))


def test_saturated_regimes(orc):
    """with the oracle's distances both regimes occur over the parametrisation of the GPU test, and nothing else does"""
    seen = {}
    for L, seed, variant, redrawn in inp.SATURATED:
        case = inp.saturated(L, seed, variant, redrawn)
        keep, Ms, ref = trimmed(orc, case, msa_matrix(orc, case.seqs, L))
        inp.saturated_conditions(Ms, case.B)
        seen[(L, seed, variant, redrawn)] = inp.regime(Ms, ref, case.B)
    print(seen)
    assert set(seen.values()) == {"placeable", "no candidate"}, seen


@pytest.mark.parametrize("which", [1, 2, 3])
def test_mash_families(orc, which):
    case = inp.mash_families(which)
    keep, Ms, ref = trimmed(orc, case, mash_matrix(orc, case.seqs))
    assert len(keep) == case.B + sum(case.sizes)
    inp.mash_conditions(ref, case.B, case.sizes)
    groups = sum(-(-m // 8) for m in case.sizes)
    assert inp.jobs_expected(case.sizes) == groups + (which == 3)            # a second column job in case 3 only
