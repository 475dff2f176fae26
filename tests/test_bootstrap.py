"""CPU tests of the bootstrap support (`dipper --bootstrap N`): the host restatement of the column sample, the split counter
against the Python Newick writer + split reader of tests/_util.py, and the command's usage errors (no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

from tests import _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
U64 = np.uint64


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def mix64(z):
    z = z + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def np_boot_weights(seed, r, L):
    """the sample of the issue, in numpy: key_r = mix64(S ^ mix64(r)); column_t = ((mix64(key_r ^ t) >> 32) * L) >> 32"""
    with np.errstate(over="ignore"):
        key = mix64(np.array([seed], dtype=U64) ^ mix64(np.array([r], dtype=U64)))[0]
        d = mix64(np.arange(L, dtype=U64) ^ key)
        col = ((d >> U64(32)) * U64(L)) >> U64(32)
    return np.bincount(col.astype(np.int64), minlength=L).astype(np.int32)


@pytest.mark.parametrize("L", [1, 31, 32, 33, 700, 10_000, 100_003])
def test_boot_weights_match_numpy(L):
    from dipper_amd import capi
    for seed, r in ((1, 0), (1, 1), (11, 5), (2**64 - 1, 123456), (0x0123456789ABCDEF, 2**40)):
        w = capi.msa_boot_weights(seed, r, L)
        assert w.sum() == L
        assert np.array_equal(w, np_boot_weights(seed, r, L)), (seed, r, L)


def test_boot_weights_depend_on_seed_and_replicate():
    from dipper_amd import capi
    a, b, c = capi.msa_boot_weights(1, 0, 1000), capi.msa_boot_weights(1, 1, 1000), capi.msa_boot_weights(2, 0, 1000)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, capi.msa_boot_weights(1, 0, 1000))


def random_log(rng, n):
    mx, my = np.zeros(max(n - 2, 1), np.int32), np.zeros(max(n - 2, 1), np.int32)
    for it in range(n - 2):
        y = int(rng.integers(1, n - it))
        mx[it], my[it] = int(rng.integers(0, y)), y
    return mx, my


def clades(n, mx, my):
    """tips below every internal node n+k (realID bookkeeping of writeNewickFromMerges) and the root's two children"""
    real = list(range(n))
    below = {t: frozenset([t]) for t in range(n)}
    for it in range(n - 2):
        x, y = int(mx[it]), int(my[it])
        below[n + it] = below[real[x]] | below[real[y]]
        real[x] = n + it
        real[y] = real[n - it - 1]
    return below, (real[0], real[1])


def expected_counts(n, mx, my, rx, ry):
    names = ["t%d" % i for i in range(n)]
    ones = np.ones(max(n - 2, 1))
    rep = _util.splits(_util.newick_from_merges(names, rx, ry, ones, ones, 1.0), names)
    below, _ = clades(n, mx, my)
    full = frozenset(range(n))
    out = np.zeros(max(n - 2, 1), np.int32)
    for k in range(n - 2):
        b = below[n + k]
        if 1 < len(b) < n - 1 and (b if 0 not in b else full - b) in rep:
            out[k] = 1
    return out


def test_split_support_matches_newick_splits():
    from dipper_amd import capi
    rng = np.random.default_rng(3)
    for n in list(range(3, 40)) + [57, 128, 211, 300]:
        for _ in range(4 if n < 100 else 2):
            mx, my = random_log(rng, n)
            rx, ry = random_log(rng, n)
            got = capi.split_support(n, mx, my, rx, ry)
            assert np.array_equal(got[: n - 2], expected_counts(n, mx, my, rx, ry)[: n - 2]), n
            # a replicate that shares part of the main tree: the first merges equal
            cut = int(rng.integers(0, n - 1))
            sx, sy = random_log(rng, n)
            sx[:cut], sy[:cut] = mx[:cut], my[:cut]
            got = capi.split_support(n, mx, my, sx, sy)
            assert np.array_equal(got[: n - 2], expected_counts(n, mx, my, sx, sy)[: n - 2]), n


def test_split_support_accumulates_and_leaves_trivial_entries():
    from dipper_amd import capi
    rng = np.random.default_rng(5)
    for n in (3, 4, 5, 9, 64, 300):
        mx, my = random_log(rng, n)
        below, _ = clades(n, mx, my)
        counts = np.full(max(n - 2, 1), 7, dtype=np.int32)
        capi.split_support(n, mx, my, mx, my, counts)           # the main tree itself: every non-trivial node + 1
        capi.split_support(n, mx, my, mx, my, counts)
        for k in range(n - 2):
            nontrivial = 1 < len(below[n + k]) < n - 1
            assert counts[k] == (9 if nontrivial else 7), (n, k)


def test_split_support_root_children():
    """root children: a leaf and the (trivial) rest, or two internal nodes that name ONE split (each counted once, both
    carry it)"""
    from dipper_amd import capi
    rng = np.random.default_rng(11)
    seen = {"leaf": 0, "both": 0}
    for _ in range(400):
        n = int(rng.integers(4, 12))
        mx, my = random_log(rng, n)
        below, (a, b) = clades(n, mx, my)
        rx, ry = random_log(rng, n)
        got = capi.split_support(n, mx, my, rx, ry)
        exp = expected_counts(n, mx, my, rx, ry)
        assert np.array_equal(got[: n - 2], exp[: n - 2])
        if a < n or b < n:
            seen["leaf"] += 1
            inner = b if a < n else a
            if inner >= n:
                assert len(below[inner]) == n - 1 and got[inner - n] == 0
        else:
            seen["both"] += 1
            assert got[a - n] == got[b - n]
            # the same tree counts its root split once per replicate
            self_counts = capi.split_support(n, mx, my, mx, my)
            assert self_counts[a - n] == 1 and self_counts[b - n] == 1
    assert seen["leaf"] > 10 and seen["both"] > 10


def test_split_support_rejects_bad_logs():
    from dipper_amd import capi
    mx, my = np.array([2, 0, 0], np.int32), np.array([1, 1, 1], np.int32)     # x > y
    with pytest.raises(capi.DipperError):
        capi.split_support(5, mx, my, mx, my)
    mx, my = np.array([0, 0, 0], np.int32), np.array([4, 4, 1], np.int32)     # y >= n - it
    with pytest.raises(capi.DipperError):
        capi.split_support(5, mx, my, mx, my)


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_the_options():
    r = run("-h")
    assert r.returncode == 0 and "--bootstrap " in r.stderr and "--bootstrap-seed" in r.stderr


@pytest.mark.parametrize("extra,msg", [
    (["-i", "d", "--bootstrap", "5"], "-i m"),
    (["-i", "r", "--bootstrap", "5"], "-i m"),
    (["-i", "m", "--bootstrap", "5", "--add", "-t", "x.nwk"], "--add"),
    (["-i", "m", "--bootstrap", "5", "-o", "d"], "-o t"),
    (["-i", "m", "--bootstrap", "5", "-m", "1"], "-m 2"),
    (["-i", "m", "--bootstrap", "5", "-m", "3"], "-m 2"),
    (["-i", "m", "--bootstrap", "0"], "whole number"),
    (["-i", "m", "--bootstrap", "-3"], "whole number"),
    (["-i", "m", "--bootstrap", "ten"], "whole number"),
    (["-i", "m", "--bootstrap", "5x"], "whole number"),
    (["-i", "m", "--bootstrap-seed", "3"], "--bootstrap-seed needs --bootstrap"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-seed", "-1"], "unsigned 64-bit"),
    (["-i", "m", "--bootstrap", "5", "--bootstrap-seed", "18446744073709551616"], "unsigned 64-bit"),
])
def test_usage_errors_need_no_device(tmp_path, extra, msg):
    p = tmp_path / "a.fa"
    p.write_text(">a\nACGT\n>b\nACGA\n>c\nACCA\n>d\nTCGA\n")
    r = run("-I", str(p), "-O", str(tmp_path / "o.nwk"), *extra)
    assert r.returncode == 1, r.stderr
    assert "\033[31m" in r.stderr and msg in r.stderr, r.stderr[:400]
    assert "Gpu_ERROR" not in r.stderr and not (tmp_path / "o.nwk").exists()
