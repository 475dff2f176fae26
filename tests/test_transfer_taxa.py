"""CPU tests of the per-taxon transfer index (`dipper --bootstrap N --bootstrap-taxa FILE`): the host restatement
dpr_transfer_taxa_host against the definition with Python sets, its identities, a planted rogue taxon, the Newick recomputation
the GPU tests use, and the command's usage errors (no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

from tests import _taxa, _tbe, _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
CUTOFFS = (0, 300, 999)


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def shapes(rng, n):
    yield "random", _tbe.random_log(rng, n)
    yield "caterpillar", _tbe.caterpillar_log(n)
    yield "balanced", _tbe.balanced_log(n)


def check_against_sets(n, mx, my, rx, ry, cutoff):
    from dipper_amd import capi
    phi, moved, pairs = capi.transfer_taxa_host(n, mx, my, rx, ry, cutoff)
    exp_moved, exp_pairs, exp_phi = _taxa.taxa_brute(n, mx, my, rx, ry, cutoff)
    assert np.array_equal(moved[:n], exp_moved), (n, cutoff, np.flatnonzero(moved[:n] != exp_moved)[:10])
    assert pairs[0] == exp_pairs, (n, cutoff)
    assert int(moved[:n].sum()) == exp_phi, (n, cutoff)              # sum of moved = sum of phi over the counted pairs
    assert np.array_equal(phi, capi.transfer_support_host(n, mx, my, rx, ry))
    return moved[:n], int(pairs[0])


def test_log_from_merges_restates_the_shapes():
    """node merges -> slot log: the caterpillar 0, 1, .. has the clades {0 .. k}; a log's own merges give the log back"""
    for n in (4, 9, 60):
        mx, my = _taxa.caterpillar_of(list(range(n)))
        assert all(0 <= mx[it] < my[it] < n - it for it in range(n - 2))
        assert _tbe.clades(n, mx, my)[n:] == [frozenset(range(k + 1)) for k in range(1, n - 1)]
    rng = np.random.default_rng(3)
    for n in (4, 5, 17, 80):
        mx, my = _tbe.random_log(rng, n)
        real, pairs = list(range(n)), []
        for it in range(n - 2):
            x, y = int(mx[it]), int(my[it])
            pairs.append((real[x], real[y]))
            real[x] = n + it
            real[y] = real[n - it - 1]
        gx, gy = _taxa.log_from_merges(n, pairs)
        assert np.array_equal(gx, mx) and np.array_equal(gy, my)


def test_host_matches_definition():
    rng = np.random.default_rng(31)
    counted = 0
    for n in list(range(4, 26)) + [47, 64, 65, 128, 211, 300]:
        for _, (mx, my) in shapes(rng, n):
            for rx, ry in (_tbe.random_log(rng, n), _tbe.shared_prefix(rng, n, mx, my), _tbe.caterpillar_log(n), _tbe.balanced_log(n)):
                for cutoff in CUTOFFS:
                    counted += check_against_sets(n, mx, my, rx, ry, cutoff)[1]
            if n > 100:
                break
    assert counted > 1000


def test_cutoff_zero_counts_the_felsenstein_splits():
    """c = 0: a pair is counted iff phi = 0, so moved is all zero and pairs is the split count summed over the branches (the
    root's two children: one branch)"""
    from dipper_amd import capi
    rng = np.random.default_rng(14)
    total = 0
    for n in (5, 8, 17, 40, 120, 300):
        for _ in range(6):
            mx, my = _tbe.random_log(rng, n) if n != 40 else _tbe.balanced_log(n)
            rx, ry = _tbe.shared_prefix(rng, n, mx, my)
            _, moved, pairs = capi.transfer_taxa_host(n, mx, my, rx, ry, 0)
            cnt = capi.split_support(n, mx, my, rx, ry)
            assert not moved.any()
            assert pairs[0] == sum(int(cnt[k]) for k in _taxa.branches(n, mx, my)), n
            total += int(pairs[0])
    assert total > 50


def test_replicate_equal_to_main_moves_nothing():
    from dipper_amd import capi
    rng = np.random.default_rng(2)
    for n in (4, 30, 300, 2000):
        for _, (mx, my) in shapes(rng, n):
            for cutoff in CUTOFFS:
                _, moved, pairs = capi.transfer_taxa_host(n, mx, my, mx, my, cutoff)
                assert not moved.any() and pairs[0] == len(_taxa.branches(n, mx, my))


def test_accumulates_across_replicates():
    from dipper_amd import capi
    rng = np.random.default_rng(6)
    for n in (4, 5, 9, 64, 300):
        mx, my = _tbe.random_log(rng, n)
        reps = [_tbe.shared_prefix(rng, n, mx, my) for _ in range(3)]
        phi, moved, pairs = np.full(max(n - 2, 1), 7, np.int64), np.full(n, 3, np.int64), np.full(1, 11, np.int64)
        for rx, ry in reps:
            capi.transfer_taxa_host(n, mx, my, rx, ry, 300, phi, moved, pairs)
        singles = [capi.transfer_taxa_host(n, mx, my, rx, ry, 300) for rx, ry in reps]
        p = _tbe.p_of(n, mx, my)
        for k in range(n - 2):
            assert phi[k] == 7 + (sum(int(s[0][k]) for s in singles) if p[k] >= 2 else 0)
        assert np.array_equal(moved, 3 + sum(s[1][:n] for s in singles))
        assert pairs[0] == 11 + sum(int(s[2][0]) for s in singles)


def check_rogue(n, mx, my, rx, ry, rogue):
    """the moved tip is the only one with a count, and that count is the sum of phi over the counted pairs"""
    moved, pairs = check_against_sets(n, mx, my, rx, ry, 300)
    sets = _taxa.transfer_sets(n, mx, my, rx, ry, 300)
    assert pairs == len(sets) > 0
    assert moved[rogue] == sum(phi for phi, _ in sets.values()) > 0
    assert all(T <= {rogue} for _, T in sets.values())
    assert not np.delete(moved, rogue).any()
    assert moved[rogue] > np.delete(moved, rogue).max()
    return int(moved[rogue])


def test_planted_rogue_caterpillar():
    """a caterpillar of 60 tips joined in the order 0, 1, .., 59; the replicate takes tip 5 out and puts it back before tip 40"""
    n = 60
    mx, my = _taxa.caterpillar_of(list(range(n)))
    order = [t for t in range(n) if t != 5]
    order.insert(order.index(40), 5)
    rx, ry = _taxa.caterpillar_of(order)
    assert check_rogue(n, mx, my, rx, ry, 5) == 34          # (the clades {0..k}, k = 5 .. 38, lose tip 5)


def test_planted_rogue_random_tree():
    rng = np.random.default_rng(77)
    n, done = 60, 0
    while done < 5:
        mx, my = _tbe.random_log(rng, n)
        tip = int(rng.integers(0, n))
        if tip in _taxa.root_children(n, mx, my):
            continue
        rx, ry = _taxa.prune_regraft(rng, n, mx, my, tip)
        if not any(phi for phi, _ in _taxa.transfer_sets(n, mx, my, rx, ry, 300).values()):
            continue                                             # (regrafted where it was, or next to it)
        check_rogue(n, mx, my, rx, ry, tip)
        done += 1


def test_root_children_count_once():
    """both root children with p >= 2: one branch; against itself every branch is counted once"""
    from dipper_amd import capi
    rng = np.random.default_rng(9)
    seen = {"both": 0, "other": 0}
    for _ in range(200):
        n = int(rng.integers(4, 16))
        mx, my = _tbe.random_log(rng, n)
        a, b = _taxa.root_children(n, mx, my)
        p = _tbe.p_of(n, mx, my)
        listed = sum(1 for k in range(n - 2) if p[k] >= 2)
        both = a >= n and b >= n and p[a - n] >= 2
        seen["both" if both else "other"] += 1
        assert len(_taxa.branches(n, mx, my)) == listed - (1 if both else 0)
        for cutoff in CUTOFFS:
            _, moved, pairs = capi.transfer_taxa_host(n, mx, my, mx, my, cutoff)
            assert pairs[0] == listed - (1 if both else 0) and not moved.any()
        rx, ry = _tbe.random_log(rng, n)
        check_against_sets(n, mx, my, rx, ry, 999)
    assert seen["both"] > 10 and seen["other"] > 10
    mx, my = _tbe.balanced_log(64)                               # 32 + 32 tips at the root
    assert len(_taxa.branches(64, mx, my)) == sum(1 for q in _tbe.p_of(64, mx, my) if q >= 2) - 1


def test_small_n_bad_logs_and_bad_cutoffs():
    from dipper_amd import capi
    for n in (2, 3):
        one = np.zeros(1, np.int32)
        phi, moved, pairs = capi.transfer_taxa_host(n, one, one, one, one, 300)
        assert not phi.any() and not moved.any() and pairs[0] == 0
    mx, my = np.array([2, 0, 0], np.int32), np.array([1, 1, 1], np.int32)     # x > y
    ok_x, ok_y = _tbe.random_log(np.random.default_rng(1), 5)
    for args in ((mx, my, ok_x, ok_y), (ok_x, ok_y, mx, my)):
        with pytest.raises(capi.DipperError) as ei:
            capi.transfer_taxa_host(5, *args)
        assert ei.value.code == -1 and "not a merge log (0 <= x < y < n - it)" in str(ei.value)
    for cutoff in (-1, 1000, 5000):
        with pytest.raises(capi.DipperError) as ei:
            capi.transfer_taxa_host(5, ok_x, ok_y, ok_x, ok_y, cutoff)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError):
        capi.transfer_taxa_host(1, ok_x, ok_y, ok_x, ok_y)


def test_newick_recomputation_matches_merge_logs():
    """taxa_from_newick (what the command tests compare with) sees trees as text only: it equals the merge-log computation, so
    the choice among equally close replicate branches does not depend on how a tree's nodes are numbered"""
    from dipper_amd import capi
    rng = np.random.default_rng(41)
    some = 0
    for n in (4, 5, 12, 37, 90, 200):
        names = ["t%d" % i for i in range(n)]
        ones = np.ones(max(n - 2, 1))
        mx, my = _tbe.random_log(rng, n) if n != 37 else _tbe.balanced_log(n)
        reps = [_tbe.shared_prefix(rng, n, mx, my) for _ in range(3)] + [_tbe.random_log(rng, n), _tbe.balanced_log(n)]
        main = _util.newick_from_merges(names, mx, my, ones, ones, 1.0)
        texts = [_util.newick_from_merges(names, rx, ry, ones, ones, 1.0) for rx, ry in reps]
        for cutoff in CUTOFFS:
            moved, pairs = np.zeros(n, np.int64), np.zeros(1, np.int64)
            for rx, ry in reps:
                capi.transfer_taxa_host(n, mx, my, rx, ry, cutoff, None, moved, pairs)
            got_moved, got_pairs, got_b = _taxa.taxa_from_newick(main, texts, names, cutoff)
            assert np.array_equal(got_moved, moved) and got_pairs == pairs[0], (n, cutoff)
            assert got_b == len(_taxa.branches(n, mx, my))
            some += int(moved.sum())
    assert some > 100
    assert [_taxa.index_text(m, p) for m, p in ((0, 0), (5, 0), (1, 3), (2, 3), (7, 7), (1, 2000000), (3, 2000000))] == \
        ["0.000000", "0.000000", "0.333333", "0.666667", "1.000000", "0.000001", "0.000002"]


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_the_options():
    r = run("-h")
    assert r.returncode == 0 and "--bootstrap-taxa arg" in r.stderr and "--bootstrap-taxa-cutoff arg" in r.stderr


@pytest.mark.parametrize("extra,msg", [
    (["--bootstrap-taxa", "T"], "--bootstrap-taxa needs --bootstrap"),
    (["--bootstrap-taxa-cutoff", "0.3"], "--bootstrap-taxa-cutoff needs --bootstrap-taxa"),
    (["--bootstrap", "5", "--bootstrap-taxa-cutoff", "0.3"], "--bootstrap-taxa-cutoff needs --bootstrap-taxa"),
    (["--bootstrap", "5", "--bootstrap-metric", "tbe", "--bootstrap-taxa-cutoff", "0.3"], "--bootstrap-taxa-cutoff needs --bootstrap-taxa"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "1"], "0 <= x < 1"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "1.0"], "0 <= x < 1"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "-0.1"], "0 <= x < 1"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "0.3000"], "at most three places"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "0.1234"], "at most three places"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "3e-1"], "0 <= x < 1"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", ""], "0 <= x < 1"),
    (["--bootstrap", "5", "--bootstrap-taxa", "T", "--bootstrap-taxa-cutoff", "."], "0 <= x < 1"),
    (["--bootstrap", "5", "--bootstrap-taxa", "SAME"], "must differ from the output file"),
    (["--bootstrap", "5", "--bootstrap-metric", "tbe", "--bootstrap-taxa", "SAME"], "must differ from the output file"),
])
def test_usage_errors_need_no_device(tmp_path, extra, msg):
    p = tmp_path / "a.fa"
    p.write_text(">a\nACGT\n>b\nACGA\n>c\nACCA\n>d\nTCGA\n")
    out, taxa = tmp_path / "o.nwk", tmp_path / "taxa.tsv"
    extra = [str(out) if a == "SAME" else str(taxa) if a == "T" else a for a in extra]
    r = run("-i", "m", "-I", str(p), "-O", str(out), *extra)
    assert r.returncode == 1, r.stderr
    assert "\033[31m" in r.stderr and msg in r.stderr, r.stderr[:400]
    assert "Gpu_ERROR" not in r.stderr and not out.exists() and not taxa.exists()
