"""BIONJ on the host (no GPU): dpr_nj_variant_host -- the restatement of the streaming loop that the device tests compare with
bit for bit -- against the existing NJ reference (variant 0) and a textbook NumPy BIONJ (variant 1, tests/_bionj_ref.py); the
lambda edge cases; the `--bionj` usage errors of the command."""
import os
import subprocess

import numpy as np
import pytest

from tests import _bionj_ref, _nonfinite, _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


@pytest.fixture(scope="module")
def capi():
    from dipper_amd import capi
    capi.load_library()
    return capi


def _splits(n, log):
    names = [f"t{i}" for i in range(n)]
    nwk = _util.newick_from_merges(names, log["merge_x"], log["merge_y"], log["bl_x"], log["bl_y"], log["last_d"], fmt=repr)
    return _util.splits(nwk, names)


# ---- variant 0: the shared machinery (keys, canonical sums, slot moves) against the NJ reference, bit for bit ------------------
@pytest.mark.parametrize("kind", ["random", "additive_ties"])
@pytest.mark.parametrize("n", [3, 4, 5, 64, 257, 600])
def test_variant0_equals_nj_reference(capi, orc, n, kind):
    rng = np.random.default_rng(100 * n + (kind == "random"))
    D = _bionj_ref.random_matrix(rng, n) if kind == "random" else _util.random_additive_matrix(rng, n, zero_frac=0.4)
    ref = orc.nj_run(np.tril(D, -1))
    got = capi.nj_variant_host(0, D)
    assert got["iters"] == ref["iters"] == n - 2
    for k in ("merge_x", "merge_y", "bl_x", "bl_y"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["last_d"] == ref["last_d"]
    assert np.all(got["lam"] == 0.5)


def test_variant0_partial_run_and_arguments(capi, orc):
    rng = np.random.default_rng(4)
    D = _bionj_ref.random_matrix(rng, 40)
    ref = orc.nj_run(np.tril(D, -1))
    got = capi.nj_variant_host(0, D, max_iters=7)
    assert got["iters"] == 7 and np.array_equal(got["merge_x"], ref["merge_x"][:7]) and np.array_equal(got["bl_y"], ref["bl_y"][:7])
    with pytest.raises(capi.DipperError) as ei:
        capi.nj_variant_host(2, D)
    assert ei.value.code == -1


# ---- variant 1 against the textbook ---------------------------------------------------------------------------------------
def _close(a, b):
    """1e-9 relative, 1e-12 absolute near 0"""
    return abs(a - b) <= max(1e-9 * max(abs(a), abs(b)), 1e-12)


@pytest.mark.parametrize("n,seed", [(5, 5000), (5, 5001), (16, 16000), (16, 16004), (64, 64000), (64, 64003)])
def test_variant1_equals_textbook_bionj(capi, n, seed):
    """Random matrices that are no tree metrics.  The NumPy reference alone says how far the best pair's Q is from the second
    best over the run (the two ties that are identities of the criterion at 4 and 3 nodes aside, see _bionj_ref.bionj): above
    1e-9 both runs must join the same pairs, so the same splits, and lengths and lambda agree to rounding."""
    D = _bionj_ref.random_matrix(np.random.default_rng(seed), n)
    got = capi.nj_variant_host(1, D)
    assert got["iters"] == n - 2
    nodes, last_pair = _bionj_ref.log_nodes(n, got["merge_x"], got["merge_y"])
    assert _bionj_ref.bionj(D)["min_gap"] > 1e-9                      # the reference on its own
    ref = _bionj_ref.bionj(D, follow=nodes)
    print("min gap", ref["min_gap"])
    assert ref["min_gap"] > 1e-9
    assert _splits(n, got) == ref["splits"]
    for t, ((a, b), (ra, rb, la, lb, lam)) in enumerate(zip(nodes, ref["merges"])):
        assert {a, b} == {ra, rb}, t
        if a != ra:                                                    # the reference names the pair the other way round
            la, lb, lam = lb, la, 1.0 - lam
        assert _close(got["bl_x"][t], la) and _close(got["bl_y"][t], lb), (t, got["bl_x"][t], la, got["bl_y"][t], lb)
        assert _close(got["lam"][t], lam), (t, got["lam"][t], lam)
    assert set(last_pair) == set(ref["last"][:2]) and _close(got["last_d"], ref["last"][2])


@pytest.mark.parametrize("n,seed", [(8, 1), (33, 2), (64, 3)])
def test_additive_input_gives_the_generating_tree(capi, n, seed):
    D, true_splits = _bionj_ref.additive_with_tree(np.random.default_rng(seed), n)
    got = capi.nj_variant_host(1, D)
    assert got["iters"] == n - 2
    assert _splits(n, got) == true_splits
    assert _bionj_ref.bionj(D)["splits"] == true_splits
    assert np.all((got["lam"] >= 0.0) & (got["lam"] <= 1.0))


def test_bionj_differs_from_nj_on_a_noisy_matrix(capi):
    """not vacuous: tree metric x lognormal noise, the two algorithms build different trees"""
    n = 24
    rng = np.random.default_rng(0)
    D, _ = _bionj_ref.additive_with_tree(rng, n)
    E = np.tril(rng.normal(size=(n, n)), -1)
    D = D * np.exp(0.25 * (E + E.T))
    nj, bj = capi.nj_variant_host(0, D), capi.nj_variant_host(1, D)
    assert _splits(n, nj) != _splits(n, bj)
    assert _splits(n, bj) == _bionj_ref.bionj(D)["splits"] and _splits(n, nj) == _bionj_ref.bionj(D, variant=0)["splits"]


# ---- lambda edges ---------------------------------------------------------------------------------------------------------
def _cherry(first_far):
    """five taxa: 0 and 1 are close to each other (0.1); one of them is at 10 from the other three, its sibling at 5; the
    others at 8 from each other.  (0, 1) has the smallest Q by far; s = 3 (v_1k - v_0k) = -15 or +15 against 2 r v_01 = 0.6."""
    D = np.full((5, 5), 8.0)
    np.fill_diagonal(D, 0.0)
    a, b = (10.0, 5.0) if first_far else (5.0, 10.0)
    D[0, 2:] = D[2:, 0] = a
    D[1, 2:] = D[2:, 1] = b
    D[0, 1] = D[1, 0] = 0.1
    return D


def test_lambda_clamps_at_0_and_1(capi):
    for first_far, want in ((True, 0.0), (False, 1.0)):
        D = _cherry(first_far)
        got = capi.nj_variant_host(1, D)
        assert (got["merge_x"][0], got["merge_y"][0]) == (0, 1)
        assert got["lam"][0] == want
        ref = _bionj_ref.bionj(D)
        assert ref["merges"][0][:2] == (0, 1) and ref["merges"][0][4] == want


def test_lambda_of_duplicate_taxa_is_one_half(capi):
    """a taxon and its copy: d = v = 0 between them, so the weight is 0 / 0"""
    D, _ = _bionj_ref.additive_with_tree(np.random.default_rng(5), 12)
    n = 13
    D2 = np.zeros((n, n))
    D2[:12, :12] = D
    D2[12, :12] = D2[:12, 12] = D[4]
    got = capi.nj_variant_host(1, D2)
    nodes, _ = _bionj_ref.log_nodes(n, got["merge_x"], got["merge_y"])
    hits = [t for t, pair in enumerate(nodes) if set(pair) == {4, 12}]
    assert len(hits) == 1                                 # the two copies are joined with each other
    assert got["lam"][hits[0]] == 0.5 and got["bl_x"][hits[0]] == 0.0 and got["bl_y"][hits[0]] == 0.0
    assert got["iters"] == n - 2 and not np.any(np.isnan(got["lam"]))


@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_nonfinite_distances_end_without_a_nan_lambda(capi, case):
    n = 100
    name, D = _nonfinite.matrices(n, 31)[case]
    got = capi.nj_variant_host(1, D)
    assert 1 <= got["iters"] <= n - 2, name               # the run ends: at n - 2, or where no candidate is left
    assert not np.any(np.isnan(got["lam"])), name
    assert np.all((got["lam"] >= 0.0) & (got["lam"] <= 1.0))


# ---- the command: usage errors before any GPU call -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()
    d = tmp_path_factory.mktemp("bionj")
    (d / "a.fa").write_text(">a\nACGTACGT\n>b\nACGTACGA\n>c\nACGTACAA\n>d\nACGTAAAA\n")
    (d / "t.nwk").write_text("((a:0.1,b:0.1):0.1,c:0.1);\n")
    return d


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True)


@pytest.mark.parametrize("args,needle", [
    (["-i", "m", "--bionj", "-m", "1"], "--bionj needs conventional NJ"),
    (["-i", "m", "--bionj", "-m", "3"], "--bionj needs conventional NJ"),
    (["-i", "r", "--bionj", "-m", "1"], "--bionj needs conventional NJ"),
    (["-i", "m", "--bionj", "--add", "-t", "T"], "--bionj is not supported with --add"),
    (["-i", "m", "--bionj", "-o", "d"], "--bionj needs tree output"),
    (["-i", "m", "--bionj", "-o", "j", "--add", "-t", "T"], "--bionj"),
    (["-i", "m", "--bionj", "-o", "j"], "--bionj needs tree output"),
    (["-i", "m", "--bionj", "--bootstrap", "3", "-m", "3"], "--bionj needs conventional NJ"),
])
def test_bionj_usage_errors(inputs, tmp_path, args, needle):
    out = tmp_path / "o.nwk"
    args = [str(inputs / "t.nwk") if a == "T" else a for a in args]
    r = run(*args, "-I", str(inputs / "a.fa"), "-O", str(out))
    assert r.returncode == 1 and "\033[31m" in r.stderr and needle in r.stderr, r.stderr[:400]
    assert not out.exists()


def test_help_names_bionj(inputs):
    r = run("-h")
    assert r.returncode == 0
    assert "--bionj" in r.stderr and "BIONJ" in r.stderr
