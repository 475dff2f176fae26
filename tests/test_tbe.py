"""CPU tests of the transfer bootstrap expectation (`dipper --bootstrap N --bootstrap-metric tbe`): the host restatement
dpr_transfer_support_host against phi from the definition with Python sets, its relations to the split counts, the Newick
recomputation the GPU tests use, and the command's usage errors (no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

from tests import _tbe, _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def shapes(rng, n):
    yield "random", _tbe.random_log(rng, n)
    yield "caterpillar", _tbe.caterpillar_log(n)
    yield "balanced", _tbe.balanced_log(n)


def check_against_brute(n, mx, my, rx, ry):
    from dipper_amd import capi
    got = capi.transfer_support_host(n, mx, my, rx, ry)
    exp = _tbe.phi_brute(n, mx, my, rx, ry)
    for k in range(n - 2):
        assert got[k] == exp.get(k, 0), (n, k, got[k], exp.get(k))
    return got


def test_shapes_are_merge_logs():
    for n in (3, 4, 9, 100):
        for name, (mx, my) in shapes(np.random.default_rng(n), n):
            for it in range(n - 2):
                assert 0 <= mx[it] < my[it] < n - it, (name, n, it)
    A = _tbe.clades(64, *_tbe.balanced_log(64))
    assert max(len(c) for c in A[64:]) == 32        # the root's two children hold 32 tips each
    A = _tbe.clades(40, *_tbe.caterpillar_log(40))
    assert sorted(len(c) for c in A[40:]) == list(range(2, 40))


def test_host_matches_definition():
    rng = np.random.default_rng(21)
    for n in list(range(4, 34)) + [47, 64, 65, 128, 211, 300]:
        for _, (mx, my) in shapes(rng, n):
            for rx, ry in (_tbe.random_log(rng, n), _tbe.shared_prefix(rng, n, mx, my), _tbe.caterpillar_log(n), _tbe.balanced_log(n)):
                check_against_brute(n, mx, my, rx, ry)
            if n > 100:
                break


def test_root_children():
    """the root's two children name one bipartition: both main nodes get the same phi; a leaf child leaves the other node
    (n - 1 tips, p = 1) without a value"""
    from dipper_amd import capi
    rng = np.random.default_rng(8)
    seen = {"leaf": 0, "both": 0}
    for _ in range(300):
        n = int(rng.integers(4, 14))
        mx, my = _tbe.random_log(rng, n)
        rx, ry = _tbe.random_log(rng, n)
        got = check_against_brute(n, mx, my, rx, ry)
        real = list(range(n))
        for it in range(n - 2):
            real[int(mx[it])] = n + it
            real[int(my[it])] = real[n - it - 1]
        a, b = real[0], real[1]
        if a < n or b < n:
            seen["leaf"] += 1
            inner = b if a < n else a
            if inner >= n:
                untouched = np.full(n - 2, 5, np.int64)
                capi.transfer_support_host(n, mx, my, rx, ry, untouched)
                assert untouched[inner - n] == 5
        else:
            seen["both"] += 1
            assert got[a - n] == got[b - n]
    assert seen["leaf"] > 10 and seen["both"] > 10


def test_accumulates_and_leaves_other_entries():
    from dipper_amd import capi
    rng = np.random.default_rng(5)
    for n in (4, 5, 9, 64, 300):
        mx, my = _tbe.random_log(rng, n)
        p = _tbe.p_of(n, mx, my)
        acc = np.full(max(n - 2, 1), 7, np.int64)
        reps = [_tbe.random_log(rng, n) for _ in range(3)]
        for rx, ry in reps:
            capi.transfer_support_host(n, mx, my, rx, ry, acc)
        singles = [capi.transfer_support_host(n, mx, my, rx, ry) for rx, ry in reps]
        for k in range(n - 2):
            assert acc[k] == (7 + sum(int(s[k]) for s in singles) if p[k] >= 2 else 7), (n, k)


def test_zero_exactly_where_the_split_is_counted_and_bounded():
    from dipper_amd import capi
    rng = np.random.default_rng(13)
    zeros = 0
    for n in (5, 8, 17, 40, 120, 300):
        for _ in range(6):
            mx, my = _tbe.random_log(rng, n)
            rx, ry = _tbe.shared_prefix(rng, n, mx, my)
            phi = capi.transfer_support_host(n, mx, my, rx, ry)
            cnt = capi.split_support(n, mx, my, rx, ry)
            p = _tbe.p_of(n, mx, my)
            for k in range(n - 2):
                if p[k] < 2:
                    assert phi[k] == 0 and cnt[k] == 0
                    continue
                assert 0 <= phi[k] <= p[k] - 1, (n, k)
                assert (phi[k] == 0) == (cnt[k] == 1), (n, k)
                zeros += cnt[k]
    assert zeros > 50


def test_replicate_equal_to_main_gives_zero():
    from dipper_amd import capi
    rng = np.random.default_rng(2)
    for n in (4, 30, 300, 2000):
        for _, (mx, my) in shapes(rng, n):
            assert not capi.transfer_support_host(n, mx, my, mx, my)[: n - 2].any()


def test_small_n_and_bad_logs():
    from dipper_amd import capi
    for n in (2, 3):
        one = np.zeros(1, np.int32)
        assert list(capi.transfer_support_host(n, one, one, one, one)) == [0]
    mx, my = np.array([2, 0, 0], np.int32), np.array([1, 1, 1], np.int32)     # x > y
    ok_x, ok_y = _tbe.random_log(np.random.default_rng(1), 5)
    for args in ((mx, my, ok_x, ok_y), (ok_x, ok_y, mx, my)):
        with pytest.raises(capi.DipperError) as ei:
            capi.transfer_support_host(5, *args)
        assert ei.value.code == -1 and "not a merge log (0 <= x < y < n - it)" in str(ei.value)
    mx, my = np.array([0, 0, 0], np.int32), np.array([4, 4, 1], np.int32)     # y >= n - it
    with pytest.raises(capi.DipperError):
        capi.transfer_support_host(5, mx, my, mx, my)
    with pytest.raises(capi.DipperError):
        capi.transfer_support_host(1, ok_x, ok_y, ok_x, ok_y)


def test_newick_recomputation_matches_definition():
    """tbe_expected (what the command tests compare with) against phi_brute, through the Python Newick writer"""
    rng = np.random.default_rng(4)
    for n in (4, 5, 12, 37, 90):
        names = ["t%d" % i for i in range(n)]
        ones = np.ones(max(n - 2, 1))
        mx, my = _tbe.random_log(rng, n)
        reps = [_tbe.shared_prefix(rng, n, mx, my) for _ in range(3)] + [_tbe.random_log(rng, n)]
        main = _util.newick_from_merges(names, mx, my, ones, ones, 1.0)
        texts = [_util.newick_from_merges(names, rx, ry, ones, ones, 1.0) for rx, ry in reps]
        sums = {}
        for rx, ry in reps:
            for k, v in _tbe.phi_brute(n, mx, my, rx, ry).items():
                sums[k] = sums.get(k, 0) + v
        A = _tbe.clades(n, mx, my)
        by_clade = {A[n + k]: k for k in range(n - 2)}
        got = _tbe.tbe_expected(main, texts, names)
        assert len(got) == n - 2
        R = len(reps)
        for clade, lab, exp in got:
            k = by_clade[clade]
            p = min(len(clade), n - len(clade))
            if p < 2:
                assert exp is None
            else:
                den = R * (p - 1)
                assert exp == (200 * (den - sums[k]) + den) // (2 * den), (n, k)


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_the_metric():
    r = run("-h")
    assert r.returncode == 0 and "--bootstrap-metric" in r.stderr and "tbe" in r.stderr and "fbp" in r.stderr


@pytest.mark.parametrize("extra,msg", [
    (["-i", "m", "--bootstrap-metric", "tbe"], "--bootstrap-metric needs --bootstrap"),
    (["-i", "m", "--bootstrap-metric", "fbp"], "--bootstrap-metric needs --bootstrap"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", "TBE"], "fbp or tbe"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", "transfer"], "fbp or tbe"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", ""], "fbp or tbe"),
    (["-i", "d", "--bootstrap", "5", "--bootstrap-metric", "tbe"], "-i m"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", "tbe", "--add", "-t", "x.nwk"], "--add"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", "tbe", "-o", "d"], "-o t"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", "tbe", "-m", "1"], "-m 2"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-metric", "tbe", "-m", "3"], "-m 2"),
    (["-i", "m", "--bootstrap", "0", "--bootstrap-metric", "tbe"], "whole number"),
])
def test_usage_errors_need_no_device(tmp_path, extra, msg):
    p = tmp_path / "a.fa"
    p.write_text(">a\nACGT\n>b\nACGA\n>c\nACCA\n>d\nTCGA\n")
    r = run("-I", str(p), "-O", str(tmp_path / "o.nwk"), *extra)
    assert r.returncode == 1, r.stderr
    assert "\033[31m" in r.stderr and msg in r.stderr, r.stderr[:400]
    assert "Gpu_ERROR" not in r.stderr and not (tmp_path / "o.nwk").exists()
