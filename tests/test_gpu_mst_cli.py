"""`dipper -o s [--dendrogram FILE]` on the GPU, against Dipper.mst on the same input uploaded from Python: the edge file equals, byte for
byte, the header and one line `name_i<TAB>name_j<TAB>%.9g` per edge in the library's order; the `MST:` line follows from the library's
figures; cutting the file at T gives the --clusters file of `-o p --within T`; the dendrogram is the library's merge log written by the
UPGMA writer, ultrametric and the same bytes in a second run; several components give exit status 1, the edge file and no dendrogram.

`-i d` reads its file with float precision (as the reference's reader does): there an entry is the float the reader makes of the
token, and that is what Python uploads."""
import os
import subprocess

import numpy as np
import pytest

from tests import _fit_ref, _mst_ref as R, _upgma_ref, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
N = 40


def run(*args, status=0):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == status, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, orc):
    """name -> (the arguments that name the input, the names, upload(d) -> (source, dist_type, k))"""
    from dipper_amd import capi
    tmp = tmp_path_factory.mktemp("mst")
    out = {}
    seqs = _util.synth_alignment(np.random.default_rng(91), n=N, L=300, mean_bl=0.05, lo=0.02, hi=0.15, invalid_frac=0.01)
    seqs[30] = seqs[3]      # duplicates: distance 0, ties by input order
    seqs[39] = seqs[30]
    seqs[21] = seqs[20]
    names = [f"S{i + 1}" for i in range(N)]
    _util.write_fasta(str(tmp / "a.fa"), names, seqs)

    def up_m(d):
        d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
        return capi.SRC_MSA, 2, 15
    out["m"] = (("-i", "m", "-I", str(tmp / "a.fa"), "-d", "2"), names, up_m)

    # sequence 6 (G and T only) differs from every other one (A and C only) at every site: under JC no distance to it is a number
    apart = list(seqs)
    apart[5] = bytes(np.frombuffer(b"GT", dtype=np.uint8)[np.arange(len(seqs[0])) % 2])
    for v in range(N):
        if v != 5:
            apart[v] = b"A" * len(seqs[0]) if v % 2 else b"A" * (len(seqs[0]) - 1 - v) + b"C" * (1 + v)
    _util.write_fasta(str(tmp / "apart.fa"), names, apart)

    def up_apart(d):
        d.set_msa(capi.pack4_many(apart), len(apart[0]))
        return capi.SRC_MSA, 2, 15
    out["apart"] = (("-i", "m", "-I", str(tmp / "apart.fa"), "-d", "2"), names, up_apart)

    reads = _util.synth_reads(np.random.default_rng(97), n=N + 2, L=4000, mean_bl=0.01, lo=0.001, hi=0.05)
    _util.write_fasta(str(tmp / "r.fa"), [f"R{i + 1}" for i in range(len(reads))], reads)

    def up_r(d):
        d.set_reads(reads)
        d.sketch(k=13, S=400, fetch=False)
        return capi.SRC_MASH, 1, 13
    out["r"] = (("-i", "r", "-I", str(tmp / "r.fa"), "-k", "13", "-s", "400"), [f"R{i + 1}" for i in range(len(reads))], up_r)

    # a matrix file with ties, zeros off the diagonal and tokens that are not floats exactly
    rng = np.random.default_rng(99)
    n = N + 3
    L = np.round(rng.random((n, n)) * 0.9 + 0.05, 2)
    L[7, 2] = L[9, 2] = L[9, 7] = 0.0
    L[11, 4] = 0.123456789
    toks = [["%.9g" % L[i, j] for j in range(i)] for i in range(n)]
    mnames = [f"M{i + 1}" for i in range(n)]
    with open(tmp / "d.phy", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            f.write("\t".join([mnames[i]] + toks[i]) + "\n")
    lower = np.array([orc.phylip_value(t) for row in toks for t in row], dtype=np.float64)

    def up_d(d):
        d.set_matrix_lower(lower, n)
        return capi.SRC_MATRIX, 1, 15
    out["d"] = (("-i", "d", "-I", str(tmp / "d.phy")), mnames, up_d)
    return out


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def expected(gpu, inputs, name):
    """(the bytes of the edge file, the MST: line, the library's answer)"""
    _, names, upload = inputs[name]
    src, dist_type, k = upload(gpu)
    got = gpu.mst(src, dist_type, k)
    lines = ["ID1\tID2\tDistance\n"] + ["%s\t%s\t%s\n" % (names[a], names[b], "%.9g" % v) for a, b, v in zip(got["i"], got["j"], got["d"])]
    st, length = got["stats"], 0.0
    for v in got["d"].tolist():
        length += v      # in file order, fp64
    line = "MST: %d edges over %d sequences (%d components, largest %d, %d singletons), %d rounds, length %s" % (
        len(got["i"]), len(names), st["components"], st["largest"], st["singletons"], st["rounds"], "%.9g" % length)
    if len(got["i"]):
        line += ", longest edge %s / %s (%s)" % (names[got["i"][-1]], names[got["j"][-1]], "%.9g" % got["d"][-1])
    return "".join(lines).encode(), line, got


def mst_line(r):
    found = [ln for ln in r.stderr.split("\n") if ln.startswith("MST: ")]
    assert len(found) == 1, r.stderr[-1500:]
    return found[0]


@pytest.mark.parametrize("name", ["m", "r", "d"])
def test_the_file_and_the_line_equal_what_python_formats_from_the_library(tmp_path, gpu, inputs, name):
    want, line, got = expected(gpu, inputs, name)
    n = len(inputs[name][1])
    out = tmp_path / "mst.tsv"
    r = run(*inputs[name][0], "-o", "s", "-O", str(out))
    assert out.read_bytes() == want and mst_line(r) == line
    assert len(got["i"]) == n - 1 and got["stats"]["components"] == 1 and os.listdir(tmp_path) == ["mst.tsv"]
    if name == "m":      # the duplicates first, among them by input order: (S22, S21), (S31, S4), (S40, S4)
        assert [ln.split("\t")[:2] for ln in want.decode().split("\n")[1:4]] == [["S22", "S21"], ["S31", "S4"], ["S40", "S4"]]


@pytest.mark.parametrize("T", ["0", "0.05", "0.12", "0.3"])
def test_cutting_the_edges_at_a_threshold_gives_the_clusters_of_the_pairs_within_it(tmp_path, inputs, T):
    args, names, _ = inputs["m"]
    run(*args, "-o", "s", "-O", str(tmp_path / "mst.tsv"))
    run(*args, "-o", "p", "--within", T, "--clusters", str(tmp_path / "c.tsv"), "-O", str(tmp_path / "p.tsv"))
    index = {nm: v for v, nm in enumerate(names)}
    cut = R._Forest(len(names))
    # (the file's nine digits decide as the matrix entry does: no entry of this input lies within 1e-9 of a threshold -- asserted)
    for ln in (tmp_path / "mst.tsv").read_text().split("\n")[1:-1]:
        a, b, v = ln.split("\t")
        assert abs(float(v) - float(T)) > 1e-8 or float(v) == float(T) == 0.0
        if float(v) <= float(T):
            cut.join(index[a], index[b])
    label = cut.labels()
    rank = {int(r): k + 1 for k, r in enumerate(sorted(set(label.tolist())))}
    rows = [ln.split("\t") for ln in (tmp_path / "c.tsv").read_text().split("\n")[1:-1]]
    assert [nm for nm, _ in rows] == names and [int(k) for _, k in rows] == [rank[int(v)] for v in label]
    assert 1 <= len(rank) < len(names)


@pytest.mark.parametrize("name", ["m", "d"])
def test_the_dendrogram_is_the_librarys_merge_log_ultrametric_and_repeatable(tmp_path, gpu, inputs, name):
    from dipper_amd import capi
    want, line, got = expected(gpu, inputs, name)
    names = inputs[name][1]
    n = len(names)
    out, tree = tmp_path / "mst.tsv", tmp_path / "single.nwk"
    r = run(*inputs[name][0], "-o", "s", "--dendrogram", str(tree), "-O", str(out))
    assert out.read_bytes() == want and mst_line(r) == line
    log = capi.mst_dendrogram_host(n, got["i"], got["j"], got["d"])
    text = tree.read_text()
    assert text == _upgma_ref.newick(names, log["merge_x"], log["merge_y"], log["height"])
    assert text.startswith("(") and text.endswith(");\n") and text.count("(") == n - 1
    seen, P, _ = _fit_ref.newick_patristic(text)
    assert sorted(seen) == sorted(names)
    # every tip at the root's height: its farthest tip lies across the root, at twice that height = the longest edge; six printed digits
    # a branch, all branches >= 0, so a sum of them keeps that relative error
    top = float(got["d"][-1])
    assert top > 0 and np.all(np.abs(P.max(axis=1) - top) <= 1e-5 * top)
    again_out, again_tree = tmp_path / "again.tsv", tmp_path / "again.nwk"
    run(*inputs[name][0], "-o", "s", "--dendrogram", str(again_tree), "-O", str(again_out))
    assert again_tree.read_bytes() == tree.read_bytes() and again_out.read_bytes() == want


def test_several_components_write_the_edges_and_no_dendrogram(tmp_path, gpu, inputs):
    want, line, got = expected(gpu, inputs, "apart")
    assert got["stats"]["components"] == 2 and got["stats"]["singletons"] == 1 and got["label"][5] == 5 and len(got["i"]) == N - 2
    out, tree = tmp_path / "mst.tsv", tmp_path / "single.nwk"
    r = run(*inputs["apart"][0], "-o", "s", "--dendrogram", str(tree), "-O", str(out), status=1)
    assert out.read_bytes() == want and mst_line(r) == line and os.listdir(tmp_path) == ["mst.tsv"]
    assert "no dendrogram" in r.stderr and "2 components" in r.stderr
    r = run(*inputs["apart"][0], "-o", "s", "-O", str(out))      # without --dendrogram several components are an answer like any other
    assert out.read_bytes() == want and mst_line(r) == line
