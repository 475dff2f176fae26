"""The inputs of tests/test_gpu_mash_pair_edges.py sit where that file needs them -- shown on the oracle's sketches alone -- the constants
of tests/_mash_pair_inputs.py are those of dipper_amd/csrc/mash.hip as it stands, and the two host restatements of that module (the
table kernel's bookkeeping with the rank bound, the token encoding and its pair loop) give the oracle's literal merge on every
builder's pairs.  Run with -s to see every condition with its count."""
import os

import numpy as np
import pytest

from tests import _mash_inputs as mi, _mash_pair_inputs as pi

CANDIDATES = [(15, False), (16, False), (17, False), (15, True), (16, True), (17, True)]
BUILDERS = dict(pi.TABLE_BUILDERS)
BUILDERS.update(pi.TOKEN_BUILDERS)
BUILDERS.update({f"S={S}": (lambda S=S: pi.sizes(S)) for S in pi.SKETCH_SIZES})
BUILDERS.update({f"n={n}{',outlier' if o else ''}": (lambda n=n, o=o: pi.candidates(n, o)) for n, o in CANDIDATES})
BUILDERS.update(shapes=pi.shapes, strided_sample=pi.strided_sample, dc_family=pi.dc_family)
MOST_PAIRS = 400          # pairs per builder that go through the restatements (the condition pairs come first)


@pytest.fixture(scope="module")
def sketched(orc):
    got = {}

    def get(name):
        if name not in got:
            case = pi.case(name, BUILDERS[name])
            sk = mi.oracle_sketches(orc, case.reads, case.k, case.S)
            sk.setflags(write=False)
            got[name] = (case, sk)
        return got[name]
    return get


def test_constants_are_those_of_the_kernel_source():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dipper_amd", "csrc", "mash.hip")
    with open(path) as f:
        found, tags = pi.constants_in_source(f.read())
    assert found == pi.CONSTEXPR
    assert tags == pi.kTagsPerBucket


@pytest.mark.parametrize("name", list(BUILDERS))
def test_conditions_hold_on_the_oracle_sketches(sketched, name):
    case, sk = sketched(name)
    seen = case.conditions(sk)
    print(name, f"{case.n} tips, S = {case.S}:", seen)
    assert all(j < i < case.n for i, j in case.pairs)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_restatements_agree_with_the_literal_merge(orc, sketched, name):
    """table bookkeeping (with rank < S) and token loop against orc_mash_dist, A = the column; a token sequence decodes to its sketch"""
    case, sk = sketched(name)
    pairs = case.pairs[:MOST_PAIRS]
    R = np.unique(sk[pi.reference_choice(sk)[0]]) if case.n <= 2000 else np.unique(sk[0])
    toks = {}
    for q in sorted(set(q for p in pairs for q in p)):
        toks[q] = pi.encode(sk[q], R)
        assert np.array_equal(pi.decode(toks[q], R), sk[q])
        assert len(toks[q]) == pi.token_count(sk[q], R)
    for i, j in pairs:
        want = orc.mash_dist(sk[j], sk[i], case.k)
        table = pi.table_pair(sk[j], sk[i])
        assert not table["phantom"]
        assert np.isclose(pi.mash_distance(table["inter"], case.S, case.k), want, rtol=1e-12, atol=0), (i, j, table)
        inter, uni, _ = pi.token_pair(toks[j], toks[i], case.S)
        assert uni == case.S
        assert np.isclose(pi.mash_distance(inter, uni, case.k), want, rtol=1e-12, atol=0), (i, j, inter)


def test_phantom_builder_separates_the_bounded_and_the_unbounded_restatement(orc, sketched):
    """Without rank < S the first pad of the padded column matches the pad entry behind the row and passes the cut-off: one more than
    the oracle's count on every pair that is on the edge, nothing on the same reads in the other roles."""
    case, sk = sketched("phantom")
    edge = [(i, j) for i, j in case.pairs if pi.phantom_condition(sk[j], sk[i])]
    rest = [p for p in case.pairs if p not in edge]
    assert len(edge) >= 10 and len(rest) >= 10
    for i, j in case.pairs:
        want = orc.mash_dist(sk[j], sk[i], case.k)
        bounded, unbounded = pi.table_pair(sk[j], sk[i]), pi.table_pair(sk[j], sk[i], bound=False)
        assert np.isclose(pi.mash_distance(bounded["inter"], case.S, case.k), want, rtol=1e-12, atol=0)
        if (i, j) in edge:
            assert unbounded["phantom"] and unbounded["inter"] == bounded["inter"] + 1
            assert not np.isclose(pi.mash_distance(unbounded["inter"], case.S, case.k), want, rtol=1e-12, atol=0)
        else:
            assert unbounded["inter"] == bounded["inter"]
    print("phantom:", len(edge), "pairs on the edge,", len(rest), "beside it")


def test_dc_family_keeps_the_phantom_pair_in_one_cluster(orc, sketched):
    """on the oracle's distances: every family is one cluster, the padded tip the earlier member, and the distance the unbounded
    restatement gives for those pairs changes the oracle's trace"""
    case, sk = sketched("dc_family")
    n = case.n
    M = np.zeros((n, n))
    for i, row in mi.oracle_rows(orc, sk, case.k, range(1, n)).items():
        M[i, :i] = row
    M += M.T
    ref = orc.dc_run(M, case.B, skip_last_backbone=0)
    assert ref["next_slot"] == 4 * n - 4
    for i, j in case.edge:
        assert case.B <= j < i and ref["cluster_id"][i] == ref["cluster_id"][j] >= 0
    for i, j in case.edge:
        M[i, j] = M[j, i] = pi.mash_distance(pi.table_pair(sk[j], sk[i], bound=False)["inter"], case.S, case.k)
    assert not np.array_equal(orc.dc_run(M, case.B, skip_last_backbone=0)["trace"], ref["trace"])


def test_sketch_lengths_reach_every_edge():
    for S in (1, 1000, 1024, 4096):
        cap = pi.kSortCap - S
        nk = {max(L - 15 + 1, 0) for L in pi.sketch_lengths(S)}
        assert {cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 0, 1, 2} <= nk
        assert {t - S for t in (1024, 1025, 2048, 2049, pi.kSortCap) if t - S >= 1} <= nk
        assert {63, 64, 65} <= set(pi.sketch_lengths(S))
    reads = pi.many_sequences()
    assert len(reads) > 1024 and len(reads[-1]) - 15 + 1 > 2 * (pi.kSortCap - 1000)


def test_launch_arithmetic():
    assert pi.cols_per_block(1100, 1100) == 8 and pi.cols_per_block(256, 1100) == 8 and pi.cols_per_block(8200, 8200) == 128
    assert pi.sample_step(8191) == 1 and pi.sample_step(8192) == 2 and pi.sample_step(8200) == 2


def test_token_restatement_on_a_hand_made_pair():
    """R = 10 20 30 40.  X = 10 20 20 25 40 40: RUN(0, 2), LIT(20, eq), LIT(25 at rank 2), RUN(3, 1), LIT(40, eq)"""
    R = np.array([10, 20, 30, 40], dtype=np.uint64)
    X = np.array([10, 20, 20, 25, 40, 40], dtype=np.uint64)
    assert pi.encode(X, R) == [(pi.RUN, 0, 2), (pi.LIT, 20, 1, True), (pi.LIT, 25, 2, False), (pi.RUN, 3, 1), (pi.LIT, 40, 3, True)]
    Y = np.array([10, 20, 26, 30, 40, 50], dtype=np.uint64)
    assert pi.encode(Y, R) == [(pi.RUN, 0, 2), (pi.LIT, 26, 2, False), (pi.RUN, 2, 2), (pi.LIT, 50, 4, False)]
    # A = Y, B = X by the literal merge: a = 10 takes b = 10; a = 20 takes both 20; a = 26 passes 25; a = 30; a = 40 takes both 40, then
    # uni = 6: inter = 5.  B's runs end at its first 20 and at its first 40, each time with an extra copy behind (bend twice); 25 and 26
    # are two literals between R[1] and R[2]
    inter, uni, ev = pi.token_pair(pi.encode(Y, R), pi.encode(X, R), 6)
    assert (inter, uni) == (5, 6) and ev["bend"] == 2 and ev["even_lt"] == 1 and ev["even_gt"] == ev["even_eq"] == 0
    assert pi.table_pair(Y, X)["inter"] == 5
