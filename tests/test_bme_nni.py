"""Balanced minimum evolution NNI search without a GPU: the host restatement dpr_bme_nni_host (the reference of
tests/test_gpu_bme_nni.py) against the textbook NumPy reference of tests/_bme_ref.py -- Pauplin's closed form for L, direct sums
for the edge lengths, differences of two L for the gains -- plus the properties of the contract, the command's usage errors and
the restatement under host sanitizers in a program of its own."""
import os
import subprocess

import numpy as np
import pytest

from tests import _bme_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GAP = 1e-9
FALLBACK_SEED = 1003      # found by fallback_search below (its fourth seed)


def start_log(kind, n, D):
    from dipper_amd import capi
    if kind == "caterpillar":
        return R.caterpillar_log(n)
    if kind == "balanced":
        return R.balanced_log(n)
    g = capi.nj_variant_host(1 if kind == "bionj" else 0, D)
    assert g["iters"] == n - 2
    return g["merge_x"], g["merge_y"]


def random_tree(rng, n):
    """a random merge log, its tree, positive edge lengths and the additive distances they generate"""
    mx, my = np.zeros(n - 2, dtype=np.int32), np.zeros(n - 2, dtype=np.int32)
    for it in range(n - 2):
        x, y = sorted(rng.choice(n - it, size=2, replace=False))
        mx[it], my[it] = x, y
    kids, top = R.tree_from_merges(n, mx, my)
    length = rng.uniform(0.05, 1.0, size=2 * n - 2)
    length[n - 1] = 0.0
    return (mx, my), kids, top, length, additive(n, kids, top, length)


def additive(n, kids, top, length):
    adj = R.adjacency(n, kids, top)
    par = R.parents(n, kids, top)
    w = lambda a, b: length[a] if par[a] == b and a != n - 1 else length[b]
    D = np.zeros((n, n))
    for i in range(n):
        stack = [(i, -1, 0.0)]
        while stack:
            v, p, d = stack.pop()
            if v < n:
                D[i, v] = d
            stack += [(u, v, d + w(u, v)) for u in adj[v] if u != p]
    return D


def log_from_tree(n, kids, top):
    """a merge log of the tree (kids, top): its internal nodes below `top` in post-order (node numbers change, the tree does not)"""
    order, stack = [], [int(top)]
    while stack:
        v = stack.pop()
        if v >= n:
            order.append(v)
            stack += [int(c) for c in kids[v - n]]
    real, mx, my = list(range(n)), [], []
    name = {v: v for v in range(n)}
    for it, v in enumerate(reversed(order)):
        x, y = sorted(real.index(name[int(c)]) for c in kids[v - n])
        mx.append(x)
        my.append(y)
        name[v] = n + it
        real[x] = n + it
        real[y] = real[-1]
        real.pop()
    return np.array(mx, dtype=np.int32), np.array(my, dtype=np.int32)


def splits_of(n, kids, top):
    tips = {}
    for v in range(n):
        tips[v] = frozenset([v])

    def clade(v):
        if v not in tips:
            a, b = (int(c) for c in kids[v - n])
            tips[v] = clade(a) | clade(b)
        return tips[v]

    return {clade(v) for v in range(n, 2 * n - 2)}


# ---- the host restatement against the textbook reference ----------------------------------------------------------------------
@pytest.mark.parametrize("start", ["nj", "bionj", "caterpillar", "balanced"])
@pytest.mark.parametrize("n,seed", [(5, 11), (8, 12), (16, 13), (40, 14)])
def test_host_equals_textbook_reference(n, seed, start):
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(seed), n)
    mx, my = start_log(start, n, D)
    kids, top = R.tree_from_merges(n, mx, my)
    rounds = 4
    ref = R.search(n, kids, top, D, rounds)
    # the comparison of moves means something only where the reference alone is clear of every tie
    assert ref["gap"] > GAP, ref["gap"]
    full = capi.bme_nni_host(D, mx, my, rounds)
    assert full["rounds"] == len(ref["picked"]) and full["fallbacks"] == ref["fallbacks"]
    assert full["moves"] == sum(len(p) for p in ref["picked"])
    for r, (rk, rt) in enumerate(ref["trees"]):
        got = capi.bme_nni_host(D, mx, my, r)
        assert np.array_equal(got["kids"], rk) and got["top"] == rt, r                    # the same moves in every round
        assert got["rounds"] == r
        assert abs(got["L_rounds"][-1] - ref["L"][r]) <= 1e-12 * abs(ref["L"][r]), (r, got["L_rounds"][-1], ref["L"][r])
        assert np.array_equal(got["L_rounds"], full["L_rounds"][: r + 1])
        assert np.max(np.abs(got["len"] - R.edge_lengths(n, rk, rt, D))) <= 1e-9
        ev = capi.bme_eval_host(D, rk, rt)
        assert np.array_equal(ev["len"], got["len"]) and ev["L"] == got["L_rounds"][-1]
        cand, _ = R.candidates(n, rk, rt, D)
        assert set(np.flatnonzero(ev["move"]).tolist()) == set(cand)
        for v, (g1, g2) in R.gains(n, rk, rt, D).items():
            assert abs(ev["gain"][v] - max(g1, g2)) <= 1e-9, (r, v)
        for v, (m, g) in cand.items():
            assert ev["move"][v] == m
        if r < len(ref["picked"]):
            assert all(ev["move"][v] == m for v, m in ref["picked"][r])


def test_pauplin_length_is_the_sum_of_the_edge_lengths():
    """the two closed forms of the reference agree with each other (9 tips, as the contract was checked)"""
    rng = np.random.default_rng(5)
    (_, _), kids, top, _, _ = random_tree(rng, 9)
    D = R.random_matrix(rng, 9)
    assert abs(R.pauplin(9, kids, top, D) - R.edge_lengths(9, kids, top, D).sum()) < 1e-12


@pytest.mark.parametrize("n", [4, 9, 30])
def test_additive_distances_no_move_and_the_generating_lengths(n):
    from dipper_amd import capi
    (mx, my), kids, top, length, D = random_tree(np.random.default_rng(20 + n), n)
    got = capi.bme_nni_host(D, mx, my, 10)
    assert (got["rounds"], got["moves"], got["fallbacks"], got["candidates0"]) == (0, 0, 0, 0)
    assert np.array_equal(got["kids"], kids) and got["top"] == top
    assert np.max(np.abs(got["len"] - length)) <= 1e-9


@pytest.mark.parametrize("n,move", [(6, 1), (12, 2), (30, 1)])
def test_one_interchange_on_an_additive_tree_is_undone_in_one_round(n, move):
    from dipper_amd import capi
    rng = np.random.default_rng(40 + n)
    _, kids, top, length, D = random_tree(rng, n)
    par = R.parents(n, kids, top)
    v = int(rng.choice([u for u in range(n, 2 * n - 2) if par[u] != n - 1]))
    wrong = R.moved(n, kids, top, v, move)
    assert splits_of(n, wrong, top) != splits_of(n, kids, top)
    mx, my = log_from_tree(n, wrong, top)
    k0, t0 = R.tree_from_merges(n, mx, my)
    assert splits_of(n, k0, t0) == splits_of(n, wrong, top)
    got = capi.bme_nni_host(D, mx, my, 10)
    assert (got["rounds"], got["moves"], got["fallbacks"]) == (1, 1, 0)
    assert splits_of(n, got["kids"], got["top"]) == splits_of(n, kids, top)
    assert abs(got["L_rounds"][1] - length.sum()) <= 1e-9


def test_no_rounds_returns_the_input_topology_with_its_lengths():
    from dipper_amd import capi
    n = 50
    D = R.random_matrix(np.random.default_rng(3), n)
    mx, my = R.balanced_log(n)
    kids, top = R.tree_from_merges(n, mx, my)
    got = capi.bme_nni_host(D, mx, my, 0)
    assert np.array_equal(got["kids"], kids) and got["top"] == top and got["rounds"] == 0 and got["moves"] == 0
    assert got["candidates0"] > 0 and len(got["L_rounds"]) == 1
    assert abs(got["L_rounds"][0] - R.pauplin(n, kids, top, D)) <= 1e-12 * got["L_rounds"][0]


@pytest.mark.parametrize("start", ["nj", "caterpillar", "balanced"])
def test_length_falls_strictly_round_by_round(start):
    from dipper_amd import capi
    n = 120
    D = R.random_matrix(np.random.default_rng(8), n)
    mx, my = start_log(start, n, D)
    got = capi.bme_nni_host(D, mx, my, 200)
    L = got["L_rounds"]
    assert got["rounds"] >= 1 and len(L) == got["rounds"] + 1 and np.all(np.diff(L) < 0)
    assert got["moves"] >= got["rounds"]
    kids, top = got["kids"], got["top"]
    assert abs(L[-1] - R.pauplin(n, kids, top, D)) <= 1e-12 * L[-1]
    # a round limit cuts the same sequence short
    part = capi.bme_nni_host(D, mx, my, 1)
    assert part["rounds"] == 1 and np.array_equal(part["L_rounds"], L[:2])


def fallback_input(seed):
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(seed), 120)
    g = capi.nj_variant_host(0, D)
    return D, g["merge_x"], g["merge_y"]


def fallback_search(first=1000, seeds=50):
    """how FALLBACK_SEED was found: the first of at most 50 seeds at 120 taxa whose search from the NJ tree needs the fallback"""
    from dipper_amd import capi
    for seed in range(first, first + seeds):
        if capi.bme_nni_host(*fallback_input(seed), 100)["fallbacks"]:
            return seed
    return None


def test_recorded_input_needs_the_fallback():
    """simultaneous rounds are not always monotone: on this input one round's moves together do not lower L, the best one alone
    does, by its gain"""
    from dipper_amd import capi
    D, mx, my = fallback_input(FALLBACK_SEED)
    got = capi.bme_nni_host(D, mx, my, 100)
    assert got["fallbacks"] >= 1 and got["rounds"] >= 2 and np.all(np.diff(got["L_rounds"]) < 0)
    # the round before the first single-move round ends on a tree whose best gain is the step that follows
    moves_per_round = [capi.bme_nni_host(D, mx, my, r)["moves"] for r in range(got["rounds"] + 1)]
    single = [r for r in range(got["rounds"]) if moves_per_round[r + 1] - moves_per_round[r] == 1]
    assert single
    hit = 0
    for r in single:
        before = capi.bme_nni_host(D, mx, my, r)
        ev = capi.bme_eval_host(D, before["kids"], before["top"])
        best = np.max(ev["gain"][ev["move"] > 0])
        hit += abs((got["L_rounds"][r] - got["L_rounds"][r + 1]) - best) <= 1e-9
    assert hit >= 1


@pytest.mark.parametrize("bad", ["nan", "inf", "both"])
def test_nonfinite_entries_return_and_move_nothing(bad):
    from dipper_amd import capi
    n = 40
    D = R.random_matrix(np.random.default_rng(6), n)
    if bad in ("nan", "both"):
        D[7, 3] = D[3, 7] = np.nan
    if bad in ("inf", "both"):
        D[30, 2] = D[2, 30] = np.inf
    mx, my = R.balanced_log(n)
    kids, top = R.tree_from_merges(n, mx, my)
    got = capi.bme_nni_host(D, mx, my, 20)
    assert not np.isfinite(got["L_rounds"][0])
    assert (got["rounds"], got["moves"]) == (0, 0) and np.array_equal(got["kids"], kids) and got["top"] == top
    assert np.isfinite(got["len"]).sum() > 0           # edges that no bad pair reaches keep their lengths


@pytest.mark.parametrize("n", [3, 4, 17, 64])
def test_caterpillar_and_balanced_logs(n):
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(n), n)
    for log, depth in ((R.caterpillar_log(n), n - 2), (R.balanced_log(n), int(np.ceil(np.log2(n))))):
        kids, top = R.tree_from_merges(n, *log)
        got = capi.bme_nni_host(D, *log, 0)
        assert np.array_equal(got["kids"], kids) and got["top"] == top
        assert abs(got["L_rounds"][0] - R.pauplin(n, kids, top, D)) <= 1e-12 * got["L_rounds"][0]
        # depth of the hung tree: the caterpillar's grows with n, the balanced tree's with log n
        par = R.parents(n, kids, top)
        deepest = 0
        for v in range(n - 1):
            d = 0
            while v != n - 1:
                v, d = par[v], d + 1
            deepest = max(deepest, d)
        assert deepest >= depth if depth == n - 2 else deepest <= 2 * depth + 2
        done = capi.bme_nni_host(D, *log, 100)
        assert np.all(np.diff(done["L_rounds"]) < 0)


def test_bad_arguments():
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(1), 6)
    mx, my = R.caterpillar_log(6)
    for bx, by in ((mx, my * 0), (mx + 5, my + 5), (my, mx)):
        with pytest.raises(capi.DipperError) as ei:
            capi.bme_nni_host(D, bx, by, 3)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError):
        capi.bme_nni_host(D[:2, :2], mx[:0], my[:0], 3)
    kids, top = R.tree_from_merges(6, mx, my)
    broken = kids.copy()
    broken[0] = broken[1]
    with pytest.raises(capi.DipperError):
        capi.bme_eval_host(D, broken, top)


# ---- the command -----------------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_help_text_names_the_option():
    r = run("--help")
    assert r.returncode == 0 and "--nni arg" in r.stderr and "balanced" in r.stderr and "minimum evolution" in r.stderr


@pytest.mark.parametrize("extra,word", [
    (("--nni", "-1"), "whole number"), (("--nni", "x"), "whole number"), (("--nni", "3", "-m", "1"), "conventional NJ"),
    (("--nni", "3", "-m", "3"), "conventional NJ"), (("--nni", "3", "--add", "-t", "x.nwk"), "--add"), (("--nni", "3", "-o", "d"), "-o t"),
    (("--nni", "3", "-o", "j", "--add", "-t", "x.nwk"), "--add"), (("--nni", "3", "--bootstrap", "5"), "--bootstrap"),
    (("--nni", "3", "--gpus", "2"), "one GPU"), (("--nni", "3", "--devices", "0,0"), "one GPU"),
    (("--nni", "3", "--rank", "0", "--world", "2", "--rendezvous", "/r"), "one GPU"), (("--nni",), "missing"),
])
def test_usage_errors_before_any_gpu_call(tmp_path, extra, word):
    """decided from the arguments alone: the input file does not even exist"""
    r = run("-i", "m", "-I", str(tmp_path / "none.fa"), "-O", str(tmp_path / "o.nwk"), *extra)
    assert r.returncode == 1 and word in r.stderr.split("DIPPER Command Line Arguments")[0], r.stderr[:400]
    assert not (tmp_path / "o.nwk").exists()


# ---- host sanitizers ---------------------------------------------------------------------------------------------------------
def test_host_restatement_under_address_and_ub_sanitizers():
    """the restatement is plain C++ in a header of its own: a driver with its own main, built with -fsanitize=address,undefined
    (`make -C dipper_amd/csrc bme_asan`), runs searches, non-finite inputs and refused inputs without a report"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "bme_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([os.path.join(ROOT, "dipper_amd", "bin", "bme_check_asan"), "12"], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 36 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
    assert any(" fallbacks 0 " not in ln for ln in lines)
