"""GPU: `dipper --protein` end to end -- NJ, -o d, placement, --add -o j and two ranks on one GPU -- against the C ABI on the
same input order (tests/test_gpu_protein.py compares the ABI's distances with the NumPy reference)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def aln(tmp_path_factory):
    """(fasta path, names, sequences): 150 x 700 residues down a Yule tree, a few gaps, lower case and X bytes, folded lines"""
    rng = np.random.default_rng(31)
    n, L = 150, 700
    seqs = [bytearray(s) for s in _aa_ref.evolve_yule(rng, n, L)]
    _aa_ref.scatter(rng, seqs, 0.02, chars=b"-X")
    seqs = [bytes(s).lower() if i % 5 == 0 else bytes(s) for i, s in enumerate(seqs)]
    names = [f"P{i+1}" for i in range(n)]
    fa = tmp_path_factory.mktemp("prot") / "p.fa"
    _util.write_fasta(str(fa), names, seqs, width=60)
    return fa, names, seqs


def _api(seqs, dt):
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    d.set_msa_aa(capi.pack_aa_many(seqs))
    d.dist_matrix(capi.SRC_MSA, dt)
    return d


def test_protein_nj_newick_equals_abi_merge_log(tmp_path, aln):
    fa, names, seqs = aln
    out = tmp_path / "o.nwk"
    r = run("-i", "m", "--protein", "-I", str(fa), "-O", str(out), "-m", "2", "-d", "8", "--seed", "-1")
    assert r.returncode == 0, r.stderr
    assert "Using conventional NJ" in r.stderr
    d = _api(seqs, 8)
    try:
        assert np.all(np.isfinite(d.matrix()))
        res = d.nj_run()
    finally:
        d.close()
    assert out.read_text() == _util.newick_from_merges(names, res["merge_x"], res["merge_y"], res["bl_x"], res["bl_y"], res["last_d"])


def test_protein_two_ranks_write_the_one_rank_newick(tmp_path, aln):
    fa, names, _ = aln
    o1, o2 = tmp_path / "one.nwk", tmp_path / "two.nwk"
    args = ["-i", "m", "--protein", "-I", str(fa), "-m", "2", "-d", "8"]
    r1 = run(*args, "-O", str(o1))
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = run(*args, "-O", str(o2), "--devices", "0,0")
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "Starting 2 ranks" in r2.stderr and "Ranks: 2 (transport ipc" in r2.stderr, r2.stderr[-1500:]
    assert o1.read_bytes() == o2.read_bytes() and o1.read_text().count(",") == len(names) - 1


@pytest.mark.parametrize("dt", [1, 7])
def test_protein_output_distance_matrix(tmp_path, aln, dt):
    fa, names, seqs = aln
    phy = tmp_path / "d.phy"
    r = run("-i", "m", "--protein", "-o", "d", "-I", str(fa), "-O", str(phy), "-d", str(dt))
    assert r.returncode == 0, r.stderr
    d = _api(seqs, dt)
    try:
        M = d.matrix()
    finally:
        d.close()
    lines = phy.read_text().strip().split("\n")
    assert int(lines[0]) == len(names) and [ln.split("\t")[0] for ln in lines[1:]] == names
    for i in range(len(names)):
        assert lines[1 + i].split("\t")[1:] == ["%.9g" % v for v in M[i, :i]], i


def test_protein_placement_equals_oracle_on_abi_matrix(tmp_path, aln, orc):
    fa, names, seqs = aln
    out = tmp_path / "p.nwk"
    r = run("-i", "m", "--protein", "-I", str(fa), "-O", str(out), "-m", "1", "-d", "7", "--seed", "-1")
    assert r.returncode == 0, r.stderr
    assert "k-closest placement mode" in r.stderr
    d = _api(seqs, 7)
    try:
        M = d.matrix()
    finally:
        d.close()
    st = orc.place_run(M)
    assert out.read_text() == _util.newick_from_placement(names, st["head"], st["e"], st["nxt"], st["len"], len(names))


def test_protein_add_tree_and_jplace(tmp_path, aln):
    """--add on a backbone of the first 100 sequences: a tree with every name, and a jplace file that names the model"""
    fa, names, seqs = aln
    m = 100
    fb, bb = tmp_path / "b.fa", tmp_path / "b.nwk"
    _util.write_fasta(str(fb), names[:m], seqs[:m])
    assert run("-i", "m", "--protein", "-I", str(fb), "-O", str(bb), "-m", "2", "-d", "7").returncode == 0
    out = tmp_path / "added.nwk"
    r = run("-i", "m", "--protein", "-I", str(fa), "-O", str(out), "--add", "-t", str(bb), "-d", "7")
    assert r.returncode == 0, r.stderr
    text = out.read_text()
    assert all((nm + ":") in text for nm in names)
    jp = tmp_path / "q.jplace"
    r = run("-i", "m", "--protein", "-I", str(fa), "-O", str(jp), "--add", "-t", str(bb), "-d", "7", "-o", "j")
    assert r.returncode == 0, r.stderr
    doc = json.loads(jp.read_text())
    assert doc["metadata"]["distance"] == "protein Poisson"
    assert sorted(p["n"][0] for p in doc["placements"]) == sorted(names[m:])
