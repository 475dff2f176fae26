"""The minimum spanning forest of the distances without a GPU: the host Kruskal dpr_mst_host (the reference of tests/test_gpu_mst.py)
against two independent NumPy statements (a Kruskal and a Boruvka in the device's round structure, tests/_mst_ref.py), as bits; the
closed forms; the single-linkage dendrogram against the minimax path distances; refused arguments; the restatement under host
sanitizers.

Nothing here has a tolerance: i, j and label are integers, d is the entry itself and is compared as uint64; the dendrogram is checked
on matrices whose entries are multiples of 1 / 1024, where every sum of branches is exact."""
import os
import subprocess

import numpy as np
import pytest

from tests import _mst_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [2, 3, 17, 130]


def host(D):
    from dipper_amd import capi
    return capi.mst_host(D)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(R.MATRICES))
def test_host_kruskal_equals_both_numpy_statements(name, n):
    D = R.matrix(name, n)
    got, ref = host(D), R.kruskal(D)
    R.same(got, ref)
    other, rounds = R.boruvka(D)
    R.same(other, ref)
    assert 1 <= rounds <= int(np.ceil(np.log2(n))) + 1
    assert len(got["i"]) == n - R.summary(got["label"])["components"]
    assert (got["i"] > got["j"]).all() and np.isfinite(got["d"]).all()
    k = R.key(got["d"]).astype(object)
    assert all((k[t], got["i"][t], got["j"][t]) < (k[t + 1], got["i"][t + 1], got["j"][t + 1]) for t in range(len(k) - 1))
    if name in ("constant", "chain"):
        i, j = R.closed_form(name, n)
        assert np.array_equal(got["i"], i) and np.array_equal(got["j"], j)
        assert rounds == 1
    if name == "hierarchy":
        assert rounds == int(np.floor(np.log2(n)))      # a level a round; the group left over beyond a power of two joins with its level
    if name == "nonfinite":
        s = R.summary(got["label"])
        assert s["components"] >= 3 - (n == 2) and s["singletons"] >= 1 and got["label"][1] == 1


def test_signed_zeros_tie_by_i_then_j_and_keep_their_sign():
    D = np.ones((5, 5))
    for (a, b), v in {(1, 0): 0.0, (2, 0): -0.0, (2, 1): -0.0, (3, 0): -0.0, (4, 3): 0.0}.items():
        D[a, b] = D[b, a] = v
    np.fill_diagonal(D, 0.0)
    got = host(D)
    assert got["i"].tolist() == [1, 2, 3, 4] and got["j"].tolist() == [0, 0, 0, 3]      # (2, 1) joins tips (1, 0) and (2, 0) joined already
    assert np.signbit(got["d"]).tolist() == [False, True, True, False] and (got["d"] == 0).all()
    R.same(got, R.kruskal(D))


def test_negative_distances_are_ordinary_values():
    D = R.negative(17)
    got = host(D)
    assert (got["d"] < 0).any() and (np.diff(got["d"]) > 0).all()
    assert got["d"][0] == D[np.tril_indices(17, -1)].min()


def test_two_tips():
    for v, edges in ((0.3, 1), (-0.0, 1), (-2.5, 1), (np.nan, 0), (np.inf, 0), (-np.inf, 0)):
        D = np.array([[0.0, v], [v, 0.0]])
        got = host(D)
        R.same(got, R.kruskal(D))
        assert len(got["i"]) == edges and got["label"].tolist() == ([0, 0] if edges else [0, 1])
        if edges:
            assert (got["i"][0], got["j"][0]) == (1, 0) and got["d"].view(np.uint64)[0] == np.array([v]).view(np.uint64)[0]


@pytest.mark.parametrize("n", [2, 3, 17, 130, 200])
@pytest.mark.parametrize("name", R.EXACT)
def test_dendrogram_paths_are_the_minimax_path_distances(name, n):
    from dipper_amd import capi
    D = R.matrix(name, n)
    f = host(D)
    assert len(f["i"]) == n - 1
    log = capi.mst_dendrogram_host(n, f["i"], f["j"], f["d"])
    assert np.array_equal(log["height"], 0.5 * f["d"])
    live = n - np.arange(n - 1)
    assert (0 <= log["merge_x"]).all() and (log["merge_x"] < log["merge_y"]).all() and (log["merge_y"] < live).all()      # the strict rule of a merge log
    parent, length = capi.tree_from_upgma(log["merge_x"], log["merge_y"], log["height"])
    assert len(parent) == 2 * n - 1 and parent[-1] == -1
    P, depth = R.tree_paths(n, parent, length)
    M = R.minimax(D)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(P[off], M[off])
    assert (depth == depth[0]).all() and depth[0] == 0.5 * f["d"][-1]      # ultrametric: every tip at the root's height


def test_a_disconnected_forest_has_no_dendrogram():
    from dipper_amd import capi
    D = R.nonfinite(17)
    f = host(D)
    assert len(f["i"]) < 16
    with pytest.raises(capi.DipperError) as ei:
        capi.mst_dendrogram_host(17, f["i"], f["j"], f["d"])
    assert ei.value.code == -1
    g = host(R.chain(5))
    with pytest.raises(capi.DipperError) as ei:      # four edges that do not span five tips: one of them twice
        capi.mst_dendrogram_host(5, [1, 2, 2, 4], [0, 1, 1, 3], g["d"])
    assert ei.value.code == -1


def test_bad_arguments_are_refused():
    from dipper_amd import capi
    with pytest.raises(capi.DipperError) as ei:
        host(np.zeros((1, 1)))      # n = 1
    assert ei.value.code == -1
    lib = capi.load_library()
    D = R.matrix("noisy", 10)
    n, rows = capi._lower_rows(D)
    i, j, d = np.full(n, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32), np.full(n, -5.0)
    label, E = np.full(n, -5, dtype=np.int32), np.full(1, -5, dtype=np.int64)
    pr, pi, pj, pd, pe, pl = (a.ctypes.data_as(t) for a, t in ((rows, capi.c_f64p), (i, capi.c_i32p), (j, capi.c_i32p), (d, capi.c_f64p),
                                                               (E, capi.c_i64p), (label, capi.c_i32p)))
    for args in ((None, n, pi, pj, pd, pe, pl), (pr, 1, pi, pj, pd, pe, pl), (pr, 0, pi, pj, pd, pe, pl), (pr, n, None, pj, pd, pe, pl),
                 (pr, n, pi, None, pd, pe, pl), (pr, n, pi, pj, None, pe, pl), (pr, n, pi, pj, pd, None, pl), (pr, n, pi, pj, pd, pe, None)):
        assert lib.dpr_mst_host(*args) == -1
    assert (i == -5).all() and (j == -5).all() and (d == -5.0).all() and (label == -5).all() and E[0] == -5      # nothing was written
    assert lib.dpr_mst_host(pr, n, pi, pj, pd, pe, pl) == 0 and E[0] == n - 1 and (label == 0).all()
    mx, my, h = np.full(n, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32), np.full(n, -5.0)
    px, py, ph = mx.ctypes.data_as(capi.c_i32p), my.ctypes.data_as(capi.c_i32p), h.ctypes.data_as(capi.c_f64p)
    for args in ((1, pi, pj, pd, 0, px, py, ph), (n, pi, pj, pd, n - 2, px, py, ph), (n, None, pj, pd, n - 1, px, py, ph),
                 (n, pi, pj, pd, n - 1, None, py, ph), (n, pi, pj, pd, n - 1, px, py, None)):
        assert lib.dpr_mst_dendrogram_host(*args) == -1
    assert (mx == -5).all() and (my == -5).all() and (h == -5.0).all()
    assert lib.dpr_mst_dendrogram_host(n, pi, pj, pd, n - 1, px, py, ph) == 0 and (mx[n - 2], my[n - 2]) == (0, 1)


def test_host_side_under_address_and_ub_sanitizers():
    """the restatement is plain C++ in a header of its own: a driver with its own main, built with -fsanitize=address,undefined
    (`make -C dipper_amd/csrc mst_asan`), checks the Kruskal forest against Prim from the first tip of every component under the same
    order, on ties, non-finite entries, signed zeros and negative entries, then the dendrogram's log and the refused arguments, without
    a report"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "mst_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "dipper_amd", "bin", "mst_check_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 24 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
