"""`dipper -o n --nearest K` on the GPU, against Dipper.nearest on the same input uploaded from Python: the file equals, byte for byte,
the header and one line `name_i<TAB>rank<TAB>name_j<TAB>%.9g` per real place of every row in input order; the four numbers of the
`Nearest:` line are the counts; the exit status is 0; a second run writes the same bytes.

`-i d` reads its file with float precision (as the reference's reader does): there an entry is the float the reader makes of the
token, and that is what Python uploads."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
N = 40
NEAREST_LINE = re.compile(r"Nearest: (\d+) neighbours of (\d+) sequences \((\d+) asked; (\d+) sequences with fewer, (\d+) with none\)")


def run(*args):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, orc):
    """name -> (the arguments that name the input, the names, upload(d) -> (source, dist_type, k))"""
    from dipper_amd import capi
    tmp = tmp_path_factory.mktemp("nearest")
    out = {}
    seqs = _util.synth_alignment(np.random.default_rng(81), n=N, L=300, mean_bl=0.05, lo=0.02, hi=0.15, invalid_frac=0.01)
    seqs[30] = seqs[3]      # duplicates: distance 0, ties by input order
    seqs[39] = seqs[30]
    seqs[21] = seqs[20]
    names = [f"S{i + 1}" for i in range(N)]
    _util.write_fasta(str(tmp / "a.fa"), names, seqs)

    def up_m(d, permille=0):
        d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
        if permille:
            d.msa_filter_sites(permille)
        return capi.SRC_MSA, 2, 15
    out["m"] = (("-i", "m", "-I", str(tmp / "a.fa"), "-d", "2"), names, up_m)
    out["coverage"] = (("-i", "m", "-I", str(tmp / "a.fa"), "-d", "2", "--site-coverage", "0.8"), names, lambda d: up_m(d, 800))

    rng = np.random.default_rng(83)
    aa = [bytes(s) for s in _aa_ref.scatter(rng, [bytearray(s) for s in _aa_ref.evolve_yule(rng, N + 1, 250)], 0.02)]
    _util.write_fasta(str(tmp / "p.fa"), [f"P{i + 1}" for i in range(len(aa))], aa)

    def up_p(d):
        d.set_msa_aa(capi.pack_aa_many(aa))
        return capi.SRC_MSA, 8, 15
    out["protein"] = (("-i", "m", "-I", str(tmp / "p.fa"), "--protein", "-d", "8"), [f"P{i + 1}" for i in range(len(aa))], up_p)

    reads = _util.synth_reads(np.random.default_rng(87), n=N + 2, L=4000, mean_bl=0.01, lo=0.001, hi=0.05)
    _util.write_fasta(str(tmp / "r.fa"), [f"R{i + 1}" for i in range(len(reads))], reads)

    def up_r(d):
        d.set_reads(reads)
        d.sketch(k=13, S=400, fetch=False)
        return capi.SRC_MASH, 1, 13
    out["r"] = (("-i", "r", "-I", str(tmp / "r.fa"), "-k", "13", "-s", "400"), [f"R{i + 1}" for i in range(len(reads))], up_r)

    # a matrix file with ties, zeros off the diagonal and tokens that are not floats exactly
    rng = np.random.default_rng(89)
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


def expected(gpu, inputs, name, K):
    _, names, upload = inputs[name]
    src, dist_type, k = upload(gpu)
    got = gpu.nearest(src, dist_type, k, K=K)
    lines = ["ID\tRank\tNeighbour\tDistance\n"]
    for i in range(len(names)):
        for r in range(int(got["cnt"][i])):
            lines.append("%s\t%d\t%s\t%s\n" % (names[i], r + 1, names[int(got["j"][i, r])], "%.9g" % got["d"][i, r]))
    return "".join(lines).encode(), got


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


@pytest.mark.parametrize("name,K", [("m", 3), ("protein", 3), ("coverage", 3), ("r", 3), ("d", 3), ("m", 64)])
def test_the_file_equals_what_python_formats_from_the_library(tmp_path, gpu, inputs, name, K):
    want, got = expected(gpu, inputs, name, K)
    n = len(inputs[name][1])
    out = tmp_path / "near.tsv"
    r = run(*inputs[name][0], "-o", "n", "--nearest", str(K), "-O", str(out))
    assert out.read_bytes() == want
    found = [NEAREST_LINE.fullmatch(ln) for ln in r.stderr.split("\n") if ln.startswith("Nearest: ")]
    assert len(found) == 1 and found[0], r.stderr[-1500:]
    cnt = got["cnt"]
    assert [int(v) for v in found[0].groups()] == [int(cnt.sum()), n, K, int((cnt < K).sum()), int((cnt == 0).sum())]
    assert want.count(b"\n") == 1 + int(cnt.sum()) and os.listdir(tmp_path) == ["near.tsv"]
    again = tmp_path / "again.tsv"
    run(*inputs[name][0], "-o", "n", "--nearest", str(K), "-O", str(again))
    assert again.read_bytes() == want
    if K >= n:      # every other sequence, the duplicates first and among them by input order
        assert (cnt == n - 1).all()
        lines = want.decode().split("\n")
        s4 = [ln.split("\t") for ln in lines if ln.startswith("S4\t")]
        assert [(x[2], float(x[3])) for x in s4[:2]] == [("S31", 0.0), ("S40", 0.0)]
        s40 = [ln.split("\t") for ln in lines if ln.startswith("S40\t")]
        assert [(x[2], float(x[3])) for x in s40[:2]] == [("S4", 0.0), ("S31", 0.0)]
