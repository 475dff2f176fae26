"""GPU tests of the per-taxon transfer index: dpr_transfer_taxa (tbe_kernel with the closest node, tbe_moved_kernel) against the
host restatement bit for bit, on every table layout, and `dipper --bootstrap N --bootstrap-taxa FILE` against the report
recomputed from the Newick files of N plain runs on host-written replicate FASTA files."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _taxa, _tbe, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GEN = os.path.join(ROOT, "tools", "bin", "gen_synth")
CUTOFFS = (0, 300, 999)


@pytest.fixture(scope="module")
def dev():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def logs(rng, n, shape):
    if shape == "caterpillar":
        return _tbe.caterpillar_log(n)
    if shape == "balanced":
        return _tbe.balanced_log(n)
    return _tbe.random_log(rng, n)


def compare(dev, n, mx, my, reps, cutoffs=CUTOFFS):
    """device == host for every replicate and cutoff, one call at a time and accumulated; the device's phi_sum is
    dpr_transfer_support's"""
    from dipper_amd import capi
    counted = 0
    for cutoff in cutoffs:
        want = [np.zeros(max(n - 2, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(1, np.int64)]
        got = [np.zeros(max(n - 2, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(1, np.int64)]
        for rx, ry in reps:
            ref = capi.transfer_taxa_host(n, mx, my, rx, ry, cutoff)
            one = dev.transfer_taxa(n, mx, my, rx, ry, cutoff)
            for a, b, what in zip(one, ref, ("phi_sum", "moved", "pairs")):
                assert np.array_equal(a, b), (n, cutoff, what, np.flatnonzero(a != b)[:10])
            for w, r in zip(want, ref):
                w += r
            dev.transfer_taxa(n, mx, my, rx, ry, cutoff, *got)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        if cutoff == 0:
            assert not want[1].any()
        counted += int(want[2][0])
    rx, ry = reps[0]
    assert np.array_equal(dev.transfer_support(n, mx, my, rx, ry), dev.transfer_taxa(n, mx, my, rx, ry, 300)[0])
    return counted


# sizes on both sides of the 64-position word, of the 1024-position tile / 1024-branch chunk of tbe_moved_kernel and of the LDS
# budget step K = 8 -> 4 (32 767 tips)
@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 129, 4097, 30000, 32768])
@pytest.mark.parametrize("shape", ["random", "caterpillar", "balanced"])
def test_kernels_equal_host(dev, n, shape):
    rng = np.random.default_rng(n * 11 + len(shape))
    mx, my = logs(rng, n, shape)
    reps = [_tbe.shared_prefix(rng, n, mx, my), _tbe.random_log(rng, n), (mx, my)]
    if n >= 30000:
        reps = reps[:1]
    counted = compare(dev, n, mx, my, reps)
    if n >= 63:
        assert counted > 0


@pytest.mark.timeout(900)
def test_kernels_at_70001_tips(dev):
    n = 70001
    rng = np.random.default_rng(70)
    mx, my = _tbe.random_log(rng, n)
    assert compare(dev, n, mx, my, [_tbe.shared_prefix(rng, n, mx, my)], cutoffs=(300,)) > 0


@pytest.mark.timeout(900)
@pytest.mark.parametrize("budget", [1, 2, 3, 4, 5, 6, 7, 8, 0])
@pytest.mark.parametrize("n", [65, 300, 4097])
def test_every_table_layout(dev, n, budget):
    """room for `budget` main nodes' tables in LDS (K = 8, 4, 2, 1 nodes per workgroup); 1 byte: the tables in global memory"""
    rng = np.random.default_rng(n + budget)
    mx, my = _tbe.balanced_log(n) if n == 300 else _tbe.random_log(rng, n)
    table = 16 * (n // 64 + 1)
    try:
        dev.set_tbe_lds(1 if budget == 0 else budget * table)
        compare(dev, n, mx, my, [_tbe.shared_prefix(rng, n, mx, my), _tbe.random_log(rng, n)])
    finally:
        dev.set_tbe_lds(0)


def test_main_tree_changes_and_calls_interleave(dev):
    """the device keeps the main tree of the last call, whichever entry made it: another main tree (same or other n) is uploaded
    again, and dpr_transfer_support between two dpr_transfer_taxa calls disturbs neither"""
    from dipper_amd import capi
    rng = np.random.default_rng(18)
    for n in (500, 500, 90, 3000, 500):
        mx, my = _tbe.random_log(rng, n)
        reps = [_tbe.random_log(rng, n), _tbe.shared_prefix(rng, n, mx, my)]
        compare(dev, n, mx, my, reps, cutoffs=(300,))
        phi, moved, pairs = np.zeros(n - 2, np.int64), np.zeros(n, np.int64), np.zeros(1, np.int64)
        plain = np.zeros(n - 2, np.int64)
        for rx, ry in reps:
            dev.transfer_taxa(n, mx, my, rx, ry, 300, phi, moved, pairs)
            dev.transfer_support(n, mx, my, rx, ry, plain)
        want = [np.zeros(n - 2, np.int64), np.zeros(n, np.int64), np.zeros(1, np.int64)]
        for rx, ry in reps:
            capi.transfer_taxa_host(n, mx, my, rx, ry, 300, *want)
        assert np.array_equal(phi, want[0]) and np.array_equal(plain, want[0])
        assert np.array_equal(moved, want[1]) and pairs[0] == want[2][0]


def test_bad_arguments(dev):
    from dipper_amd import capi
    mx, my = np.array([2, 0, 0], np.int32), np.array([1, 1, 1], np.int32)
    ok_x, ok_y = _tbe.random_log(np.random.default_rng(1), 5)
    for args in ((mx, my, ok_x, ok_y), (ok_x, ok_y, mx, my)):
        with pytest.raises(capi.DipperError) as ei:
            dev.transfer_taxa(5, *args)
        assert ei.value.code == -1 and "not a merge log (0 <= x < y < n - it)" in str(ei.value)
    for cutoff in (-1, 1000):
        with pytest.raises(capi.DipperError) as ei:
            dev.transfer_taxa(5, ok_x, ok_y, ok_x, ok_y, cutoff)
        assert ei.value.code == -1
    one = np.zeros(1, np.int32)
    phi, moved, pairs = dev.transfer_taxa(3, one, one, one, one)
    assert not phi.any() and not moved.any() and pairs[0] == 0
    compare(dev, 5, ok_x, ok_y, [(ok_x, ok_y)])


# ---- the command ---------------------------------------------------------------------------------------------------------
def run(*args, timeout=600):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def independent_trees(tmp_path, names, seqs, seed, N, args, tag):
    out = []
    for r in range(N):
        fa, o = tmp_path / f"{tag}_rep{r}.fa", tmp_path / f"{tag}_rep{r}.nwk"
        _util.write_fasta(fa, names, _tbe.replicate_seqs(seqs, seed, r))
        run("-i", "m", "-I", str(fa), "-O", str(o), *args)
        out.append(o.read_text())
    return out


def check_report(path, plain_text, rep_texts, names, N, seed, cutoff):
    """the file against the recomputation from the trees' text: header, rows in input order, moved and index of every taxon"""
    head, rows = _taxa.read_report(path)
    moved, pairs, B = _taxa.taxa_from_newick(plain_text, rep_texts, names, cutoff)
    print(f"taxa report: branches={B} pairs={pairs} of {B * N}, sum moved={int(moved.sum())}, max moved={int(moved.max())}")
    assert head == {"replicates": str(N), "seed": str(seed), "cutoff": "0.%03d" % cutoff, "branches": str(B), "pairs": str(pairs)}
    assert [r[0] for r in rows] == list(names)
    assert [r[1] for r in rows] == [int(v) for v in moved]
    assert [r[2] for r in rows] == [_taxa.index_text(v, pairs) for v in moved]
    return moved, pairs


SMALL_ARGS = ["-d", "2", "--seed", "3", "-m", "2"]       # (the run shuffles its tips; the report numbers them in input order)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """150 tips, GTR+G4+I with gaps; the main tree, 5 independent replicate trees (bootstrap seed 11)"""
    d = tmp_path_factory.mktemp("taxa")
    p = d / "aln.fa"
    r = subprocess.run([GEN, "--tips", "150", "--sites", "600", "--seed", "5", "--mean-bl", "0.02", "--lo", "0.002", "--hi", "0.2",
                        "--model", "gtr+g+i", "--indel-gaps", "--fasta", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, seqs = _tbe.read_fasta(p)
    plain = d / "plain.nwk"
    run("-i", "m", "-I", str(p), "-O", str(plain), *SMALL_ARGS)
    return p, names, plain.read_text(), independent_trees(d, names, seqs, 11, 5, SMALL_ARGS, "s")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("metric", ["tbe", "fbp"])
def test_cli_report_equals_independent_runs(tmp_path, small, metric):
    p, names, plain, reps = small
    boot = ["-i", "m", "-I", str(p), *SMALL_ARGS, "--bootstrap", "5", "--bootstrap-seed", "11", "--bootstrap-metric", metric]
    o0, o1, taxa = tmp_path / "without.nwk", tmp_path / "with.nwk", tmp_path / "taxa.tsv"
    r0 = run(*boot, "-O", str(o0))
    r1 = run(*boot, "-O", str(o1), "--bootstrap-taxa", str(taxa))
    assert o1.read_bytes() == o0.read_bytes() and re.sub(r"\)\d+", ")", o1.read_text()) == plain
    # the stderr lines of the run without the option, apart from times, and one more after the Bootstrap line
    scrub = lambda s: [re.sub(r"[0-9.]+ ms", "T ms", l) for l in s.splitlines()]
    l0, l1 = scrub(r0.stderr), scrub(r1.stderr)
    at = [i for i, l in enumerate(l1) if l.startswith("Bootstrap:")][0]
    assert l1[at + 1].startswith("Transfer index: ") and l1[:at + 1] + l1[at + 2:] == l0
    moved, pairs = check_report(taxa, plain, reps, names, 5, 11, 300)
    assert pairs > 0 and moved.sum() > 0                      # (conditions on the input: the comparison is not about zeros)
    B = int(_taxa.read_report(taxa)[0]["branches"])
    top = sorted(range(len(names)), key=lambda t: (-moved[t], t))[:5]
    assert l1[at + 1] == f"Transfer index: {pairs} of {5 * B} (branch, replicate) pairs within cutoff 0.300; most moved:" + \
        "".join(f" {names[t]} ({moved[t]})" for t in top)
    # another cutoff, parsed as text
    for text, permille in ((".999", 999), ("0", 0), ("0.05", 50)):
        run(*boot, "-O", str(o1), "--bootstrap-taxa", str(taxa), "--bootstrap-taxa-cutoff", text)
        assert o1.read_bytes() == o0.read_bytes()
        check_report(taxa, plain, reps, names, 5, 11, permille)


@pytest.mark.timeout(600)
def test_cli_report_with_the_input_order_kept(tmp_path, small):
    """a negative --seed keeps the input order (the other command tests run shuffled): the same comparison"""
    p, names, _, _ = small
    args = ["-d", "2", "--seed", "-1", "-m", "2"]
    o, plain, taxa = tmp_path / "o.nwk", tmp_path / "plain.nwk", tmp_path / "taxa.tsv"
    run("-i", "m", "-I", str(p), "-O", str(o), *args, "--bootstrap", "2", "--bootstrap-seed", "4", "--bootstrap-taxa", str(taxa),
        "--bootstrap-taxa-cutoff", "0.999")
    run("-i", "m", "-I", str(p), "-O", str(plain), *args)
    _, seqs = _tbe.read_fasta(p)
    moved, pairs = check_report(taxa, plain.read_text(), independent_trees(tmp_path, names, seqs, 4, 2, args, "io"), names, 2, 4, 999)
    assert pairs > 0 and moved.sum() > 0


@pytest.mark.timeout(600)
@pytest.mark.parametrize("devices,N", [("0,0", 5), ("0,0,0", 2)])
def test_cli_ranks_byte_identical(tmp_path, small, devices, N):
    p = small[0]
    args = ["-i", "m", "-I", str(p), *SMALL_ARGS, "--bootstrap", str(N), "--bootstrap-seed", "7", "--bootstrap-metric", "tbe"]
    o1, oG, t1, tG = tmp_path / "one.nwk", tmp_path / "many.nwk", tmp_path / "one.tsv", tmp_path / "many.tsv"
    run(*args, "-O", str(o1), "--bootstrap-taxa", str(t1))
    r = run(*args, "-O", str(oG), "--bootstrap-taxa", str(tG), "--devices", devices)
    assert f"Starting {len(devices.split(','))} ranks" in r.stderr
    assert oG.read_bytes() == o1.read_bytes() and tG.read_bytes() == t1.read_bytes()
    assert int(_taxa.read_report(t1)[0]["pairs"]) > 0


@pytest.mark.timeout(900)
def test_cli_natural_size(tmp_path):
    p = tmp_path / "big.fa"
    r = subprocess.run([GEN, "--tips", "6000", "--sites", "1500", "--seed", "9", "--mean-bl", "0.004", "--lo", "0.0004", "--hi", "0.04",
                        "--model", "gtr+g+i", "--indel-gaps", "--fasta", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = ["-d", "2", "--seed", "1", "-m", "2"]
    o, op, taxa = tmp_path / "tbe.nwk", tmp_path / "plain.nwk", tmp_path / "taxa.tsv"
    run("-i", "m", "-I", str(p), "-O", str(o), *args, "--bootstrap", "2", "--bootstrap-metric", "tbe", "--bootstrap-taxa", str(taxa))
    run("-i", "m", "-I", str(p), "-O", str(op), *args)
    names, seqs = _tbe.read_fasta(p)
    moved, pairs = check_report(taxa, op.read_text(), independent_trees(tmp_path, names, seqs, 1, 2, args, "big"), names, 2, 1, 300)
    assert pairs > 0 and moved.sum() > 0
