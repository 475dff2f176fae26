"""`dipper -o p --within T [--clusters FILE]` on the GPU, against the command's own `-o d` file for the same input: the pair file's
lines are exactly the matrix file's entries <= T in (i, j) order with the same number tokens; the clusters file equals a Python
union-find over those lines; the `Pairs:` line's numbers match; `--within 0` names the duplicated sequences; a threshold below every
distance gives the header alone; a clusters file that cannot be written ends the run without a pair file.

T is the midpoint of two adjacent distinct printed values near the lower decile of the matrix file, so the `%.9g` rounding of the
matrix text cannot move a pair across T.  `-i d` reads its file with float precision (as the reference's reader does): there an entry
is the float the reader makes of the token, and the token expected in the pair file is `%.9g` of that float."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
DUPLICATES = [(150, 3), (199, 150), (60, 59)]      # (copy, original): 3 = 150 = 199 and 59 = 60


def run(*args, ok=True):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> the arguments that name the input; every input's -o d file is written once and shared"""
    tmp = tmp_path_factory.mktemp("pairs")
    out = {}
    seqs = _util.synth_alignment(np.random.default_rng(61), n=200, L=300, mean_bl=0.05, lo=0.02, hi=0.15, invalid_frac=0.01)
    for c, o in DUPLICATES:
        seqs[c] = seqs[o]
    names = [f"S{i + 1}" for i in range(len(seqs))]
    _util.write_fasta(str(tmp / "a.fa"), names, seqs)
    out["m"] = ("-i", "m", "-I", str(tmp / "a.fa"), "-d", "2")
    out["coverage"] = ("-i", "m", "-I", str(tmp / "a.fa"), "-d", "2", "--site-coverage", "0.9")
    rng = np.random.default_rng(67)
    aa = [bytes(s) for s in _aa_ref.scatter(rng, [bytearray(s) for s in _aa_ref.evolve_yule(rng, 90, 250)], 0.02)]
    _util.write_fasta(str(tmp / "p.fa"), [f"P{i + 1}" for i in range(len(aa))], aa)
    out["protein"] = ("-i", "m", "-I", str(tmp / "p.fa"), "--protein", "-d", "8")
    reads = _util.synth_reads(np.random.default_rng(71), n=80, L=4000, mean_bl=0.01, lo=0.001, hi=0.05)
    _util.write_fasta(str(tmp / "r.fa"), [f"R{i + 1}" for i in range(len(reads))], reads)
    out["r"] = ("-i", "r", "-I", str(tmp / "r.fa"), "-k", "13", "-s", "400")
    for name in list(out):
        run(*out[name], "-o", "d", "-O", str(tmp / f"{name}.phy"))
    out["d"] = ("-i", "d", "-I", str(tmp / "m.phy"))
    out["tmp"] = tmp
    return out


def matrix_file(inputs, name, orc):
    """(names, rows of tokens) of the -o d file behind an input, and a function token -> (value the command compares, token it prints)"""
    src = "m" if name == "d" else name
    lines = open(inputs["tmp"] / f"{src}.phy").read().split("\n")
    n = int(lines[0])
    rows = [ln.split("\t") for ln in lines[1:n + 1]]
    assert all(len(r) == i + 1 for i, r in enumerate(rows))
    if name == "d":
        def entry(tok):
            v = orc.phylip_value(tok)      # the float the reader makes of the token
            return v, "%.9g" % v
    else:
        def entry(tok):
            return float(tok), tok
    return [r[0] for r in rows], [r[1:] for r in rows], entry


def midpoint_threshold(rows, entry):
    vals = sorted({entry(t)[0] for r in rows for t in r if np.isfinite(entry(t)[0])})
    assert len(vals) >= 20
    k = max(1, len(vals) // 10)
    T = 0.5 * (vals[k - 1] + vals[k])
    assert vals[k - 1] < T < vals[k]
    return T


def expected_lines(names, rows, entry, T):
    out = []
    for i, r in enumerate(rows):
        for j, tok in enumerate(r):
            v, text = entry(tok)
            if v <= T:
                out.append((names[i], names[j], text))
    return out


def union_find(names, pairs):
    idx = {nm: k for k, nm in enumerate(names)}
    parent = list(range(len(names)))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    for a, b, _ in pairs:
        ra, rb = find(idx[a]), find(idx[b])
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = [find(v) for v in range(len(names))]
    rank = {r: k + 1 for k, r in enumerate(sorted(set(roots)))}
    sizes = {}
    for r in roots:
        sizes[r] = sizes.get(r, 0) + 1
    return [rank[r] for r in roots], len(sizes), max(sizes.values()), sum(s == 1 for s in sizes.values())


PAIRS_LINE = re.compile(r"Pairs: (\d+) of (\d+) within (\S+) \((\d+) clusters, largest (\d+), (\d+) singletons\)")
CLUSTERS_HEAD = re.compile(r"# (\d+) sequences, (\d+) pairs within (\S+), (\d+) clusters, largest (\d+), (\d+) singletons")


def read_pairs(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "ID1\tID2\tDistance" and lines[-1] == ""
    return [tuple(ln.split("\t")) for ln in lines[1:-1]]


@pytest.mark.parametrize("name", ["m", "protein", "coverage", "r", "d"])
def test_pair_file_clusters_and_summary_equal_the_matrix_file(tmp_path, inputs, orc, name):
    names, rows, entry = matrix_file(inputs, name, orc)
    n = len(names)
    T = midpoint_threshold(rows, entry)
    want = expected_lines(names, rows, entry, T)
    assert 0 < len(want) < n * (n - 1) // 2
    out, clusters = tmp_path / "pairs.tsv", tmp_path / "clusters.tsv"
    r = run(*inputs[name], "-o", "p", "--within", repr(T), "-O", str(out), "--clusters", str(clusters))
    assert read_pairs(out) == want
    rank, comps, largest, single = union_find(names, want)
    lines = open(clusters).read().split("\n")
    head = CLUSTERS_HEAD.fullmatch(lines[0])
    assert head and lines[-1] == "", lines[0]
    assert [int(v) if k != 2 else v for k, v in enumerate(head.groups())] == [n, len(want), repr(T), comps, largest, single]
    assert [tuple(ln.split("\t")) for ln in lines[1:-1]] == [(nm, str(c)) for nm, c in zip(names, rank)]
    found = [PAIRS_LINE.fullmatch(ln) for ln in r.stderr.split("\n") if ln.startswith("Pairs: ")]
    assert len(found) == 1 and found[0], r.stderr[-1500:]
    assert [int(v) if k != 2 else v for k, v in enumerate(found[0].groups())] == [len(want), n * (n - 1) // 2, repr(T), comps, largest, single]
    # without --clusters: the same pair file, no other file
    alone = tmp_path / "alone"
    alone.mkdir()
    run(*inputs[name], "-o", "p", "--within", repr(T), "-O", str(alone / "pairs.tsv"))
    assert (alone / "pairs.tsv").read_bytes() == out.read_bytes() and os.listdir(alone) == ["pairs.tsv"]


def test_within_zero_lists_exactly_the_duplicated_sequences(tmp_path, inputs, orc):
    out, clusters = tmp_path / "dup.tsv", tmp_path / "dup_clusters.tsv"
    run(*inputs["m"], "-o", "p", "--within", "0", "-O", str(out), "--clusters", str(clusters))
    got = read_pairs(out)
    names, rows, entry = matrix_file(inputs, "m", orc)
    assert got == expected_lines(names, rows, entry, 0.0)
    # S4 = S151 = S200 and S60 = S61, in (i, j) order of the later sequence, then the earlier one
    assert [g[:2] for g in got] == [("S61", "S60"), ("S151", "S4"), ("S200", "S4"), ("S200", "S151")] and all(float(g[2]) == 0 for g in got)
    lines = open(clusters).read().split("\n")
    assert lines[0] == "# 200 sequences, 4 pairs within 0, 197 clusters, largest 3, 195 singletons"
    rank = dict(ln.split("\t") for ln in lines[1:-1])
    assert rank["S4"] == rank["S151"] == rank["S200"] == "4" and rank["S60"] == rank["S61"] == "60" and rank["S1"] == "1"


def test_no_pair_within_the_threshold_gives_the_header_alone(tmp_path, inputs):
    out = tmp_path / "none.tsv"
    r = run(*inputs["r"], "-o", "p", "--within", "1e-9", "-O", str(out))
    assert r.returncode == 0 and out.read_text() == "ID1\tID2\tDistance\n"
    assert "Pairs: 0 of 3160 within 1e-9 (80 clusters, largest 1, 80 singletons)" in r.stderr


def test_unwritable_clusters_file_ends_the_run_without_a_pair_file(tmp_path, inputs):
    out = tmp_path / "pairs.tsv"
    r = run(*inputs["d"], "-o", "p", "--within", "0.1", "-O", str(out), "--clusters", str(tmp_path / "no" / "dir" / "c.tsv"), ok=False)
    assert r.returncode != 0 and "--clusters" in r.stderr and "Pairs:" not in r.stderr and not out.exists()
