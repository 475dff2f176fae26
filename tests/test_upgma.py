"""UPGMA / WPGMA without a GPU: the host restatement dpr_upgma_host (the reference of tests/test_gpu_upgma.py) against the NumPy
reference of tests/_upgma_ref.py -- UPGMA from its definition, the mean of the original distances over the member pairs -- and
against a literal Python loop of the contract where ties and non-finite values decide; the properties of the contract, the
command's usage errors and the restatement under host sanitizers in a program of its own."""
import os
import subprocess

import numpy as np
import pytest

from tests import _upgma_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GAP = 1e-9
NAMES = {0: "UPGMA", 1: "WPGMA"}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_log(got, ref, exact_heights=True):
    assert np.array_equal(got["merge_x"], ref["merge_x"]) and np.array_equal(got["merge_y"], ref["merge_y"]), (got["merge_x"], ref["merge_x"])
    if exact_heights:
        same = (bits(got["height"]) == bits(ref["height"])) | (np.isnan(got["height"]) & np.isnan(ref["height"]))
        assert same.all(), (got["height"], ref["height"])


_ref = {}


def reference(n, linkage):
    """the noisy matrix of size n and the reference's run on it: computed once, shared, never changed"""
    if (n, linkage) not in _ref:
        D = R.noisy_matrix(np.random.default_rng(500 + n), n)
        D.setflags(write=False)
        _ref[(n, linkage)] = (D, R.run(D, linkage))
    return _ref[(n, linkage)]


@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 16, 40])
def test_host_equals_the_reference(n, linkage):
    from dipper_amd import capi
    D, ref = reference(n, linkage)
    # the reference alone first: no step of it is a near-tie that rounding could decide
    assert ref["gap"].min() > GAP, ref["gap"].min()
    got = capi.upgma_host(D, linkage)
    assert_same_log(got, ref, exact_heights=False)
    assert np.allclose(got["height"], ref["height"], rtol=1e-12, atol=0), np.abs(got["height"] / ref["height"] - 1).max()


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "scaled"])
@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
@pytest.mark.parametrize("n", [3, 9, 30])
def test_ultrametric_input_returns_its_tree_and_heights(n, linkage, whole):
    from dipper_amd import capi
    D, clades = R.ultrametric_tree(np.random.default_rng(7 * n + linkage), n, whole)
    got = capi.upgma_host(D, linkage)
    made = R.clades_of_log(n, got["merge_x"], got["merge_y"])
    assert {frozenset(c) for c in made} == set(clades)
    for c, h in zip(made, got["height"]):
        if whole:
            assert h == clades[frozenset(c)], (c, h, clades[frozenset(c)])      # whole numbers: every mean is exact
        else:
            assert abs(h - clades[frozenset(c)]) <= 1e-12 * h
    # heights do not fall along any root path: a node is at least as high as both its children
    node_h = np.concatenate([np.zeros(n), got["height"]])
    for it, (a, b) in enumerate(R.children_of_log(n, got["merge_x"], got["merge_y"])):
        assert node_h[n + it] >= node_h[a] and node_h[n + it] >= node_h[b]


def tie_matrix(n, seed=3):
    return R.symmetric(np.random.default_rng(seed).integers(1, 4, (n, n)).astype(np.float64))


@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
def test_whole_number_ties_follow_the_rule(linkage):
    from dipper_amd import capi
    D = tie_matrix(8)
    ref = R.contract_loop(D, linkage)
    print(NAMES[linkage], "on the 8-taxon tie matrix:", list(zip(ref["merge_x"].tolist(), ref["merge_y"].tolist())), ref["height"].tolist())
    assert_same_log(capi.upgma_host(D, linkage), ref)
    # pinned: the first merge is the smallest (value, i, j), (0, 1) only if D[1][0] is a 1
    i, j = min(((D[b, a], a, b) for a in range(8) for b in range(a + 1, 8)))[1:]
    assert (ref["merge_x"][0], ref["merge_y"][0]) == (i, j)


@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
@pytest.mark.parametrize("n", [2, 5, 12])
def test_all_equal_matrix(n, linkage):
    from dipper_amd import capi
    D = R.symmetric(np.full((n, n), 0.375))
    got = capi.upgma_host(D, linkage)
    assert_same_log(got, R.contract_loop(D, linkage))
    assert np.all(got["merge_x"] == 0) and np.all(got["merge_y"] == 1) and np.all(got["height"] == 0.1875)


def poisoned(n, kind):
    D = R.noisy_matrix(np.random.default_rng(40 + n), n).copy()
    pairs = {"inf": [((5, 2), np.inf), ((n - 1, 3), np.inf)], "nan": [((4, 1), np.nan)],
             "both": [((5, 2), np.inf), ((6, 2), np.nan), ((n - 1, 0), np.nan), ((n - 2, n - 3), np.inf)]}[kind]
    for (a, b), v in pairs:
        D[a, b] = D[b, a] = v
    return D


@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
@pytest.mark.parametrize("kind", ["inf", "nan", "both"])
def test_nonfinite_entries_merge_last(kind, linkage):
    from dipper_amd import capi
    n = 14
    D = poisoned(n, kind)
    got = capi.upgma_host(D, linkage)
    assert len(got["merge_x"]) == n - 1
    assert_same_log(got, R.contract_loop(D, linkage))
    finite = np.isfinite(got["height"])
    first_bad = int(np.argmin(finite))
    assert 0 < first_bad and not finite[first_bad:].any() and finite[:first_bad].all()
    # +inf before NaN among them
    k = np.array([R.key(h) for h in got["height"][first_bad:]], dtype=np.uint64)
    assert np.all(k[:-1] <= k[1:])
    assert (got["merge_x"][-1], got["merge_y"][-1]) == (0, 1)


def test_negative_zero_orders_as_zero():
    from dipper_amd import capi
    D = R.noisy_matrix(np.random.default_rng(2), 6).copy()
    D[1, 0] = D[0, 1] = 0.0
    D[3, 2] = D[2, 3] = -0.0
    D[5, 4] = D[4, 5] = -1e-3      # a negative entry goes first
    for linkage in (0, 1):
        got = capi.upgma_host(D, linkage)
        assert_same_log(got, R.contract_loop(D, linkage))
        assert (got["merge_x"][0], got["merge_y"][0]) == (4, 5)
        assert (got["merge_x"][1], got["merge_y"][1]) == (0, 1) and bits(got["height"][1:2])[0] == 0      # +0.0, by its indices
        assert np.signbit(got["height"][2]) and got["height"][2] == 0.0      # the -0.0 pair next, its height as it comes


def test_two_taxa_and_bad_arguments():
    from dipper_amd import capi
    got = capi.upgma_host(np.array([[0.0, 0.0], [0.5, 0.0]]), 1)
    assert got["merge_x"].tolist() == [0] and got["merge_y"].tolist() == [1] and got["height"].tolist() == [0.25]
    with pytest.raises(capi.DipperError):
        capi.upgma_host(np.zeros((1, 1)), 0)
    for linkage in (-1, 2):
        with pytest.raises(capi.DipperError):
            capi.upgma_host(R.noisy_matrix(np.random.default_rng(1), 5), linkage)
    lib = capi.load_library()
    assert lib.dpr_upgma_host(None, 5, 0, None, None, None) == -1 and b"dpr_upgma_host" in lib.dpr_last_error()
    assert lib.dpr_abi_version() == 1


@pytest.mark.parametrize("linkage,method", [(0, "average"), (1, "weighted")])
@pytest.mark.parametrize("n", [5, 16, 40])
def test_scipy_gives_the_same_clusters_and_heights(n, linkage, method):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    from dipper_amd import capi
    D, ref = reference(n, linkage)
    assert ref["gap"].min() > GAP
    got = capi.upgma_host(D, linkage)
    Z = hier.linkage(squareform(D, checks=False), method=method)
    assert np.allclose(got["height"], Z[:, 2] / 2, rtol=1e-12, atol=0)
    members = [[i] for i in range(n)]
    theirs = []
    for a, b, _, _ in Z:
        members.append(sorted(members[int(a)] + members[int(b)]))
        theirs.append(members[-1])
    assert theirs == R.clades_of_log(n, got["merge_x"], got["merge_y"])


# ---- the command -----------------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_help_text_names_the_options():
    r = run("--help")
    assert r.returncode == 0 and "--upgma " in r.stderr and "--wpgma " in r.stderr and "ultrametric" in r.stderr and "average linkage" in r.stderr


@pytest.mark.parametrize("opt", ["--upgma", "--wpgma"])
@pytest.mark.parametrize("extra,word", [
    (("--bionj",), "--bionj"), (("--nni", "3"), "--nni"), (("--spr", "3"), "--spr"), (("-m", "1"), "-m 2"), (("-m", "3"), "-m 2"),
    (("--add", "-t", "x.nwk"), "--add"), (("-o", "d"), "-o t"), (("-o", "j"), "-o t"), (("-o", "j", "--add", "-t", "x.nwk"), "--add"),
    (("--gpus", "2"), "one GPU"), (("--devices", "0,0"), "one GPU"), (("--rank", "0", "--world", "2", "--rendezvous", "/r"), "one GPU"),
])
def test_usage_errors_before_any_gpu_call(tmp_path, opt, extra, word):
    """decided from the arguments alone: the input file does not even exist"""
    r = run("-i", "m", "-I", str(tmp_path / "none.fa"), "-O", str(tmp_path / "o.nwk"), opt, *extra)
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and word in head and opt in head, r.stderr[:400]
    assert not (tmp_path / "o.nwk").exists()


def test_both_linkages_at_once_are_a_usage_error(tmp_path):
    r = run("-i", "m", "-I", str(tmp_path / "none.fa"), "-O", str(tmp_path / "o.nwk"), "--upgma", "--wpgma")
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and "--upgma" in head and "--wpgma" in head, r.stderr[:400]
    assert not (tmp_path / "o.nwk").exists()


def test_host_restatement_under_address_and_ub_sanitizers():
    """the restatement is plain C++ in a header of its own: a driver with its own main, built with -fsanitize=address,undefined
    (`make -C dipper_amd/csrc upgma_asan`), runs noisy, tied, all-equal, non-finite and refused inputs without a report"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "upgma_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([os.path.join(ROOT, "dipper_amd", "bin", "upgma_check_asan")], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 70 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
