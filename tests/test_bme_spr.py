"""Balanced minimum evolution SPR search without a GPU: the host restatement (dpr_bme_spr_host and its hooks, the reference of
tests/test_gpu_bme_spr.py) against tests/_spr_ref.py, which carries every move out on an adjacency list and takes the difference
of two Pauplin lengths -- no table of subtree averages anywhere -- plus the properties of the contract in include/dipper_hip.h."""
import os
import subprocess

import numpy as np
import pytest

from tests import _bme_ref as R, _spr_ref as S
from tests.test_bme_nni import log_from_tree, random_tree, start_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNI_OPTIMUM = (12, 2002, 0.5)      # tips, seed, noise: found by nni_optimum_search below (its third seed at 12 tips)
TIE_INPUT = (8, 3)                 # tips, seed of the whole-number matrix: found by tie_search below


def tol(D, n):
    """the sums of a gain have O(n) terms of the size of a distance (the NNI test's tolerance has the same form)"""
    return 1e-12 * np.max(D) * n


_cases = {}


def case(n, seed):
    """a random tree, a random matrix, the reference's {(d, w): (gain, k)} and the library's answer for every (d, w)"""
    from dipper_amd import capi
    if (n, seed) not in _cases:
        rng = np.random.default_rng(100 * seed + n)
        _, kids, top, _, _ = random_tree(rng, n)
        D = R.random_matrix(rng, n)
        got = {}
        for d in range(2 * (2 * n - 2)):
            for w in range(2 * n - 2):
                try:
                    got[(d, w)] = capi.bme_spr_gain_host(D, kids, top, d, w)
                except capi.DipperError as e:
                    assert e.code == -1
        _cases[(n, seed)] = (D, kids, top, S.gains(n, kids, top, D), got)
    return _cases[(n, seed)]


CASES = [(n, seed) for n in (4, 5, 6, 9, 12) for seed in (0, 1, 2)]


def argmax(got, d):
    """the contract's best target of d: the greatest gain, then the smaller w; None without a target"""
    mine = [(g, w, k) for (dd, w), (g, k) in got.items() if dd == d and g == g]
    return min(mine, key=lambda t: (-t[0], t[1])) if mine else None


# ---- every move against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", CASES)
def test_every_move_equals_the_difference_of_two_pauplin_lengths(n, seed):
    D, kids, top, ref, got = case(n, seed)
    assert set(got) == set(ref) and len(ref) > 0          # the same targets: edges at q and inside X are none
    assert len({d for d, _ in ref}) <= 3 * (n - 2)
    worst = 0.0
    for dw, (g, k) in got.items():
        assert k == ref[dw][1], dw
        worst = max(worst, abs(g - ref[dw][0]))
    print("largest difference", worst, "bound", tol(D, n))
    assert worst <= tol(D, n)


@pytest.mark.parametrize("n,seed", CASES)
def test_best_target_is_the_argmax_with_the_tie_rule(n, seed):
    from dipper_amd import capi
    D, kids, top, ref, got = case(n, seed)
    ev = capi.bme_spr_eval_host(D, kids, top)
    assert abs(ev["L"] - R.pauplin(n, kids, top, D)) <= tol(D, n)
    for d in range(2 * (2 * n - 2)):
        best = argmax(got, d)
        if best is None:
            assert (ev["gain"][d], ev["w"][d], ev["k"][d]) == (0.0, -1, 0)
        else:
            assert (ev["gain"][d], ev["w"][d], ev["k"][d]) == best, d


@pytest.mark.parametrize("n,seed", [(6, 0), (9, 1), (12, 2)])
def test_path_of_one_edge_is_the_nni_gain(n, seed):
    """move 1 of v (its larger child changes place with its sibling C) carries the smaller child onto the edge above C, move 2 the
    larger one"""
    from dipper_amd import capi
    D, kids, top, ref, got = case(n, seed)
    ev = capi.bme_eval_host(D, kids, top)
    par = R.parents(n, kids, top)
    seen = 0
    for v in range(n, 2 * n - 2):
        p = par[v]
        if p == n - 1:
            continue
        A, B = sorted(int(c) for c in kids[v - n])
        C = [int(c) for c in kids[p - n] if c != v][0]
        g1, k1 = got[(A, C)]
        g2, k2 = got[(B, C)]
        assert k1 == k2 == 1
        assert abs(max(g1, g2) - ev["gain"][v]) <= tol(D, n)
        assert abs(R.gains(n, kids, top, D)[v][0] - g1) <= tol(D, n) and abs(R.gains(n, kids, top, D)[v][1] - g2) <= tol(D, n)
        seen += 1
    assert seen > 0


# ---- the search ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["nj", "bionj", "caterpillar", "balanced"])
@pytest.mark.parametrize("n,seed", [(5, 11), (16, 13), (40, 14), (90, 15)])
def test_search_descends_to_a_tree_without_a_positive_gain(n, seed, start):
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(seed), n)
    mx, my = start_log(start, n, D)
    got = capi.bme_spr_host(D, mx, my, 500)
    assert got["rounds"] < 500 and len(got["L_rounds"]) == got["rounds"] + 1
    assert np.all(np.diff(got["L_rounds"]) < 0)
    assert got["moves"] >= got["rounds"] and got["long_moves"] <= got["moves"] and (got["max_k"] >= 2) == (got["long_moves"] > 0)
    ev = capi.bme_eval_host(D, got["kids"], got["top"])                   # a valid tree, with that function's lengths
    assert np.array_equal(ev["len"], got["len"]) and ev["L"] == got["L_rounds"][-1]
    assert abs(ev["L"] - R.pauplin(n, got["kids"], got["top"], D)) <= tol(D, n)
    sp = capi.bme_spr_eval_host(D, got["kids"], got["top"])
    if got["fallbacks"] == 0:                                                 # it ended by itself: no candidate is left
        assert not np.any(sp["gain"] > 0)
    if start == "caterpillar" and n >= 16:
        assert got["long_moves"] > 0


@pytest.mark.parametrize("n", [3, 4, 17, 64])
def test_zero_rounds_is_the_nni_entry_point_bit_for_bit(n):
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(n), n)
    for log in (R.caterpillar_log(n), R.balanced_log(n)):
        a, b = capi.bme_spr_host(D, *log, 0), capi.bme_nni_host(D, *log, 0)
        assert np.array_equal(a["kids"], b["kids"]) and a["top"] == b["top"]
        assert np.array_equal(a["len"], b["len"]) and np.array_equal(a["L_rounds"], b["L_rounds"])
        assert (a["rounds"], a["moves"], a["fallbacks"], a["long_moves"], a["max_k"]) == (0, 0, 0, 0, 0)


def nni_optimum_input(n, seed, noise):
    """a tree on which the NNI search has ended without a candidate, as a merge log, and its distances"""
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(seed), n, noise=noise)
    done = capi.bme_nni_host(D, *start_log("nj", n, D), 200)
    return D, log_from_tree(n, done["kids"], done["top"])


def nni_optimum_search(n=12, first=2000, seeds=30, noise=0.5):
    """how NNI_OPTIMUM was found: the first seed whose NNI optimum the SPR search leaves by a move past two edges or more"""
    from dipper_amd import capi
    for seed in range(first, first + seeds):
        D, log = nni_optimum_input(n, seed, noise)
        q, s = capi.bme_nni_host(D, *log, 200), capi.bme_spr_host(D, *log, 200)
        if q["candidates0"] == 0 and s["long_moves"] >= 1 and s["L_rounds"][-1] < q["L_rounds"][-1]:
            return seed
    return None


def test_spr_leaves_an_optimum_that_holds_nni():
    from dipper_amd import capi
    n = NNI_OPTIMUM[0]
    D, log = nni_optimum_input(*NNI_OPTIMUM)
    q = capi.bme_nni_host(D, *log, 200)
    assert (q["rounds"], q["candidates0"]) == (0, 0)
    s = capi.bme_spr_host(D, *log, 200)
    assert s["long_moves"] >= 1 and s["max_k"] >= 2 and s["L_rounds"][-1] < q["L_rounds"][-1]
    assert s["L_rounds"][0] == q["L_rounds"][0]
    assert abs(s["L_rounds"][-1] - R.pauplin(n, s["kids"], s["top"], D)) <= tol(D, n)


def python_round(D, n, kids, top):
    """one round of the contract on the library's scan: the selection and the moves carried out by the reference"""
    from dipper_amd import capi
    ev = capi.bme_spr_eval_host(D, kids, top)
    cands = {d: (ev["gain"][d], int(ev["w"][d])) for d in range(len(ev["k"])) if ev["k"][d] and ev["gain"][d] > 0}
    moves = S.all_moves(n, kids, top)
    picked = S.select(cands, moves)
    sets = [set(moves[dw]) for dw in picked]
    assert all(not (a & b) for i, a in enumerate(sets) for b in sets[i + 1:])
    return cands, picked, moves, S.moved(n, kids, top, moves, picked)


@pytest.mark.parametrize("start,n,seed", [("caterpillar", 40, 5), ("balanced", 60, 6), ("nj", 90, 7)])
def test_a_round_applies_the_disjoint_selection(start, n, seed):
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(seed), n)
    mx, my = start_log(start, n, D)
    kids, top = R.tree_from_merges(n, mx, my)
    cands, picked, moves, (nk, nt) = python_round(D, n, kids, top)
    one = capi.bme_spr_host(D, mx, my, 1)
    assert one["candidates0"] == len(cands) and len(picked) >= (2 if start != "nj" else 1)
    if one["fallbacks"] == 0:
        assert one["moves"] == len(picked) and np.array_equal(one["kids"], nk) and one["top"] == nt
        assert one["long_moves"] == sum(len(moves[dw]) - 4 >= 2 for dw in picked)
        assert one["max_k"] == max(len(moves[dw]) - 4 for dw in picked)
    else:
        assert one["moves"] == 1
        fk, ft = S.moved(n, kids, top, moves, picked[:1])
        assert np.array_equal(one["kids"], fk) and one["top"] == ft


# ---- ties ------------------------------------------------------------------------------------------------------------------------
def test_all_equal_distances_give_no_candidate():
    from dipper_amd import capi
    n = 14
    D = np.full((n, n), 2.0)
    np.fill_diagonal(D, 0.0)
    for log in (R.caterpillar_log(n), R.balanced_log(n)):
        got = capi.bme_spr_host(D, *log, 10)
        assert (got["rounds"], got["moves"], got["candidates0"]) == (0, 0, 0)
        kids, top = R.tree_from_merges(n, *log)
        ev = capi.bme_spr_eval_host(D, kids, top)
        assert not np.any(ev["gain"] != 0.0) and 0 < np.count_nonzero(ev["k"]) <= 3 * (n - 2)


def tie_input(n, seed):
    D = S.integer_matrix(np.random.default_rng(seed), n)
    mx, my = R.balanced_log(n)
    return D, mx, my


def tie_search():
    """how TIE_INPUT was found: the first whole-number matrix on the balanced tree of 8 tips with two subtrees whose best targets
    tie, three tied candidates and two moves in the first round"""
    from dipper_amd import capi
    for seed in range(20):
        D, mx, my = tie_input(8, seed)
        kids, top = R.tree_from_merges(8, mx, my)
        ref = S.gains(8, kids, top, D)
        tied_w = sum(1 for d in {d for d, _ in ref} if (lambda g: g[0] > 0 and g.count(g[0]) > 1)(sorted((ref[dw][0] for dw in ref if dw[0] == d), reverse=True)))
        ev = capi.bme_spr_eval_host(D, kids, top)
        pos = [g for g, k in zip(ev["gain"], ev["k"]) if k and g > 0]
        if tied_w >= 2 and len(pos) - len(set(pos)) >= 3 and capi.bme_spr_host(D, mx, my, 1)["moves"] >= 2:
            return seed
    return None


def test_exact_ties_follow_the_rules():
    """whole-number distances on 8 tips: every gain is exact, so the reference's gains are the library's bit for bit, equal gains
    are equal, and both tie rules decide"""
    from dipper_amd import capi
    n = TIE_INPUT[0]
    D, mx, my = tie_input(*TIE_INPUT)
    kids, top = R.tree_from_merges(n, mx, my)
    ref = S.gains(n, kids, top, D)
    ev = capi.bme_spr_eval_host(D, kids, top)
    tied_w = 0
    for d in range(2 * (2 * n - 2)):
        best = argmax({dw: gk for dw, gk in ref.items()}, d)
        if best is None:
            assert ev["k"][d] == 0
            continue
        assert (ev["gain"][d], ev["w"][d], ev["k"][d]) == best, d
        tied_w += best[0] > 0 and sum(1 for dw in ref if dw[0] == d and ref[dw][0] == best[0]) > 1
    pos = [g for g, k in zip(ev["gain"], ev["k"]) if k and g > 0]
    assert tied_w >= 2 and len(pos) - len(set(pos)) >= 3          # (gain, w) and (gain, d) both have ties to decide
    cands, picked, moves, (nk, nt) = python_round(D, n, kids, top)
    one = capi.bme_spr_host(D, mx, my, 1)
    assert one["fallbacks"] == 0 and one["moves"] == len(picked) >= 2
    assert np.array_equal(one["kids"], nk) and one["top"] == nt


# ---- non-finite entries, errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan", "inf", "both"])
def test_nonfinite_entries_return(bad):
    from dipper_amd import capi
    n = 40
    D = R.random_matrix(np.random.default_rng(6), n)
    if bad in ("nan", "both"):
        D[7, 3] = D[3, 7] = np.nan
    if bad in ("inf", "both"):
        D[30, 2] = D[2, 30] = np.inf
    mx, my = R.balanced_log(n)
    got = capi.bme_spr_host(D, mx, my, 20)
    assert not np.isfinite(got["L_rounds"][0]) and got["rounds"] == 0          # L' < L never holds against a non-finite L
    kids, top = R.tree_from_merges(n, mx, my)
    ev = capi.bme_spr_eval_host(D, kids, top)
    assert not np.any(np.isnan(ev["gain"]))                                     # a NaN gain is no target's gain


def test_bad_arguments():
    from dipper_amd import capi
    D = R.random_matrix(np.random.default_rng(1), 6)
    mx, my = R.caterpillar_log(6)
    for bx, by in ((mx, my * 0), (mx + 5, my + 5), (my, mx)):
        with pytest.raises(capi.DipperError) as ei:
            capi.bme_spr_host(D, bx, by, 3)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError):
        capi.bme_spr_host(D[:2, :2], mx[:0], my[:0], 3)
    kids, top = R.tree_from_merges(6, mx, my)
    broken = kids.copy()
    broken[0] = broken[1]
    with pytest.raises(capi.DipperError):
        capi.bme_spr_eval_host(D, broken, top)
    with pytest.raises(capi.DipperError):
        capi.bme_spr_gain_host(D, broken, top, 0, 1)
    for d, w in ((0, 0), (5, 1), (0, 10), (0, -1), (-1, 0), (20, 0), (int(top), 0)):       # no target, out of range, not prunable
        with pytest.raises(capi.DipperError) as ei:
            capi.bme_spr_gain_host(D, kids, top, d, w)
        assert ei.value.code == -1


# ---- host sanitizers ---------------------------------------------------------------------------------------------------------
def test_host_restatement_under_address_and_ub_sanitizers():
    """the restatement is plain C++ in a header of its own: a driver with its own main, built with -fsanitize=address,undefined
    (`make -C dipper_amd/csrc bme_spr_asan`), runs searches, every single move of the small trees, non-finite inputs and refused
    inputs without a report"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "bme_spr_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([os.path.join(ROOT, "dipper_amd", "bin", "bme_spr_check_asan"), "12"], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 36 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
    assert any(" long 0 " not in ln for ln in lines)
