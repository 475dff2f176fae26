"""GPU tests of the transfer bootstrap expectation: the device kernel (dpr_transfer_support) against the host restatement bit for
bit, on every table layout, and `dipper --bootstrap N --bootstrap-metric tbe` against TBE recomputed from the Newick files of N
plain runs on host-written replicate FASTA files."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _tbe, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GEN = os.path.join(ROOT, "tools", "bin", "gen_synth")


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


def compare(dev, n, mx, my, reps):
    from dipper_amd import capi
    want = np.zeros(max(n - 2, 1), np.int64)
    got = np.zeros(max(n - 2, 1), np.int64)
    for rx, ry in reps:
        one = dev.transfer_support(n, mx, my, rx, ry)
        ref = capi.transfer_support_host(n, mx, my, rx, ry)
        assert np.array_equal(one, ref), (n, np.flatnonzero(one != ref)[:10])
        want += ref
        dev.transfer_support(n, mx, my, rx, ry, got)
    assert np.array_equal(got, want)
    return want


# sizes on both sides of the 64-position word and of the LDS budget steps (K = 8 up to 32 767 tips, 4 up to 65 535, ...)
@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 127, 128, 129, 4097, 30000, 32767, 32768])
@pytest.mark.parametrize("shape", ["random", "caterpillar", "balanced"])
def test_kernel_equals_host(dev, n, shape):
    rng = np.random.default_rng(n * 7 + len(shape))
    mx, my = logs(rng, n, shape)
    reps = [_tbe.random_log(rng, n), _tbe.shared_prefix(rng, n, mx, my), (mx, my)]
    if n >= 30000:
        reps = reps[1:]
    total = compare(dev, n, mx, my, reps)
    p = np.array(_tbe.p_of(n, mx, my)) if n <= 4097 else None
    if p is not None:
        assert np.all(total[: n - 2][p < 2] == 0)


@pytest.mark.timeout(900)
def test_kernel_above_65536_tips(dev):
    """100 003 tips: two main nodes per workgroup (25 KB of tables each), against the host restatement"""
    n = 100003
    rng = np.random.default_rng(99)
    mx, my = _tbe.random_log(rng, n)
    compare(dev, n, mx, my, [_tbe.shared_prefix(rng, n, mx, my)])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("budget", [1, 2, 4, 8, 0])
@pytest.mark.parametrize("n", [65, 300, 4097, 70001])
def test_every_table_layout(dev, n, budget):
    """K = budget main nodes per workgroup in LDS; 1 byte: the tables in global memory"""
    rng = np.random.default_rng(n + budget)
    mx, my = _tbe.balanced_log(n) if n == 300 else _tbe.random_log(rng, n)
    table = 16 * (n // 64 + 1)
    try:
        dev.set_tbe_lds(1 if budget == 0 else budget * table)
        compare(dev, n, mx, my, [_tbe.shared_prefix(rng, n, mx, my)] + ([_tbe.random_log(rng, n)] if n < 70001 else []))
    finally:
        dev.set_tbe_lds(0)


def test_main_tree_changes_between_calls(dev):
    """the device keeps the main tree of the last call: another main tree (same or other n) is uploaded again"""
    rng = np.random.default_rng(17)
    for n in (500, 500, 90, 3000, 500):
        mx, my = _tbe.random_log(rng, n)
        compare(dev, n, mx, my, [_tbe.random_log(rng, n), _tbe.shared_prefix(rng, n, mx, my)])


def test_bad_logs_and_one_rank_sum(dev):
    from dipper_amd import capi
    mx, my = np.array([2, 0, 0], np.int32), np.array([1, 1, 1], np.int32)
    ok_x, ok_y = _tbe.random_log(np.random.default_rng(1), 5)
    for args in ((mx, my, ok_x, ok_y), (ok_x, ok_y, mx, my)):
        with pytest.raises(capi.DipperError) as ei:
            dev.transfer_support(5, *args)
        assert ei.value.code == -1 and "not a merge log (0 <= x < y < n - it)" in str(ei.value)
    compare(dev, 5, ok_x, ok_y, [(ok_x, ok_y)])
    assert list(dev.comm_sum_i64([1, -2, 3 << 40])) == [1, -2, 3 << 40]      # one rank: nothing to add


# ---- the command ---------------------------------------------------------------------------------------------------------
def run(*args, timeout=600):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def strip_labels(text):
    return re.sub(r"\)\d+", ")", text)


def independent_trees(tmp_path, names, seqs, seed, N, args, tag):
    out = []
    for r in range(N):
        fa, o = tmp_path / f"{tag}_rep{r}.fa", tmp_path / f"{tag}_rep{r}.nwk"
        _util.write_fasta(fa, names, _tbe.replicate_seqs(seqs, seed, r))
        run("-i", "m", "-I", str(fa), "-O", str(o), *args)
        out.append(o.read_text())
    return out


def check_tbe(text, fbp_text, names, rep_texts):
    """labels equal the recomputation; TBE >= FBP everywhere, equal where p = 2; no label where p < 2"""
    got = _tbe.tbe_expected(text, rep_texts, names)
    _, fnodes = _tbe.tree_nodes(fbp_text, names)        # (the same tree: the texts differ in their labels only)
    flabels = [lab for _, _, lab, leaf in fnodes if not leaf]
    assert len(flabels) == len(got)
    n, checked = len(names), 0
    for (clade, lab, exp), flab in zip(got, flabels):
        p = min(len(clade), n - len(clade))
        if exp is None:
            assert lab is None and flab is None
            continue
        assert lab is not None and int(lab) == exp, (lab, exp, p)
        assert int(lab) >= int(flab), (lab, flab, p)
        if p == 2:
            assert int(lab) == int(flab)
        checked += 1
    assert checked > 0


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("tbe")
    p = d / "aln.fa"
    r = subprocess.run([GEN, "--tips", "150", "--sites", "600", "--seed", "5", "--mean-bl", "0.02", "--lo", "0.002", "--hi", "0.2",
                        "--model", "gtr+g+i", "--indel-gaps", "--fasta", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return p


@pytest.mark.timeout(600)
def test_cli_tbe_labels_equal_independent_runs(tmp_path, small):
    args = ["-d", "2", "--seed", "3", "-m", "2"]
    boot = ["--bootstrap", "6", "--bootstrap-seed", "11"]
    ot, of, od, op = (tmp_path / f"{t}.nwk" for t in ("tbe", "fbp", "default", "plain"))
    r = run("-i", "m", "-I", str(small), "-O", str(ot), *args, *boot, "--bootstrap-metric", "tbe")
    line = [l for l in r.stderr.splitlines() if l.startswith("Bootstrap:")][0]
    assert line.startswith("Bootstrap: 6 replicates (seed 11) in ") and ", 1 ranks" in line and "tbe" in line
    r_fbp = run("-i", "m", "-I", str(small), "-O", str(of), *args, *boot, "--bootstrap-metric", "fbp")
    r_def = run("-i", "m", "-I", str(small), "-O", str(od), *args, *boot)
    run("-i", "m", "-I", str(small), "-O", str(op), *args)
    # fbp named or not: the same file, and the same stderr lines apart from times
    assert of.read_bytes() == od.read_bytes()
    scrub = lambda s: [re.sub(r"[0-9.]+ ms", "T ms", l) for l in s.splitlines()]
    assert scrub(r_fbp.stderr) == scrub(r_def.stderr) and "tbe" not in r_def.stderr
    text, plain = ot.read_text(), op.read_text()
    assert strip_labels(text) == plain and text != plain and text != of.read_text()
    names, seqs = _tbe.read_fasta(small)
    check_tbe(text, of.read_text(), names, independent_trees(tmp_path, names, seqs, 11, 6, args, "s"))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("devices,N", [("0,0", 5), ("0,0,0", 2)])
def test_cli_tbe_ranks_byte_identical(tmp_path, small, devices, N):
    args = ["-i", "m", "-I", str(small), "-d", "2", "--seed", "3", "-m", "2", "--bootstrap", str(N), "--bootstrap-seed", "7",
            "--bootstrap-metric", "tbe"]
    o1, oG = tmp_path / "one.nwk", tmp_path / "many.nwk"
    run(*args, "-O", str(o1))
    r = run(*args, "-O", str(oG), "--devices", devices)
    G = len(devices.split(","))
    line = [l for l in r.stderr.splitlines() if l.startswith("Bootstrap:")][0]
    assert f"Starting {G} ranks" in r.stderr and f"{G} ranks" in line and "tbe" in line
    assert oG.read_bytes() == o1.read_bytes()


@pytest.mark.timeout(900)
def test_cli_tbe_natural_size(tmp_path):
    p = tmp_path / "big.fa"
    r = subprocess.run([GEN, "--tips", "6000", "--sites", "1500", "--seed", "9", "--mean-bl", "0.004", "--lo", "0.0004", "--hi", "0.04",
                        "--model", "gtr+g+i", "--indel-gaps", "--fasta", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = ["-d", "2", "--seed", "1", "-m", "2"]
    ot, of, op = tmp_path / "tbe.nwk", tmp_path / "fbp.nwk", tmp_path / "plain.nwk"
    run("-i", "m", "-I", str(p), "-O", str(ot), *args, "--bootstrap", "2", "--bootstrap-metric", "tbe")
    run("-i", "m", "-I", str(p), "-O", str(of), *args, "--bootstrap", "2")
    run("-i", "m", "-I", str(p), "-O", str(op), *args)
    text = ot.read_text()
    assert strip_labels(text) == op.read_text()
    names, seqs = _tbe.read_fasta(p)
    check_tbe(text, of.read_text(), names, independent_trees(tmp_path, names, seqs, 1, 2, args, "big"))
