"""GPU: `dipper --complete-deletion` / `--site-coverage X` end to end.  The yardstick is the command itself on the alignment the
test has filtered on the host (tests/_sites_ref.py): the two runs must write the same bytes, whatever builds the tree."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _sites_ref, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
N, L = 60, 300


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


class Aln:
    """an alignment and its completely deleted form as FASTA files"""

    def __init__(self, d, tag, seqs, alphabet, permille=1000):
        self.seqs = [bytes(s) for s in seqs]
        self.names = [f"{tag}{i + 1}" for i in range(len(seqs))]
        self.cov = _sites_ref.coverage(self.seqs, alphabet)
        self.keep = _sites_ref.keep(self.cov, len(seqs), permille)
        self.kept = int(self.keep.sum())
        self.full, self.filtered = str(d / f"{tag}.fa"), str(d / f"{tag}.filtered.fa")
        _util.write_fasta(self.full, self.names, self.seqs, width=70)
        _util.write_fasta(self.filtered, self.names, _sites_ref.filtered(self.seqs, self.keep), width=70)


@pytest.fixture(scope="module")
def nt(tmp_path_factory):
    rng = np.random.default_rng(41)
    seqs = [bytearray(s) for s in _util.synth_alignment(rng, N, L, mean_bl=0.02, lo=0.002, hi=0.1)]
    _aa_ref.scatter(rng, seqs, 0.01, chars=b"-Nn")
    a = Aln(tmp_path_factory.mktemp("sites_nt"), "S", seqs, "nt")
    assert 100 < a.kept < 250
    return a


@pytest.fixture(scope="module")
def prot(tmp_path_factory):
    rng = np.random.default_rng(42)
    seqs = [bytearray(s) for s in _aa_ref.evolve_yule(rng, N, L)]
    _aa_ref.scatter(rng, seqs, 0.01, chars=b"-X*")
    seqs = [bytes(s).lower() if i % 4 == 0 else bytes(s) for i, s in enumerate(seqs)]
    a = Aln(tmp_path_factory.mktemp("sites_aa"), "P", seqs, "aa")
    assert 100 < a.kept < 250
    return a


def _pair(tmp_path, aln, *args, flag=("--complete-deletion",)):
    """(run with the option on the full alignment, run without it on the filtered one) and their output paths"""
    o1, o2 = tmp_path / "option.out", tmp_path / "filtered.out"
    r1 = run("-i", "m", "-I", aln.full, "-O", str(o1), *args, *flag)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = run("-i", "m", "-I", aln.filtered, "-O", str(o2), *args)
    assert r2.returncode == 0, r2.stderr[-2000:]
    return r1, r2, o1, o2


@pytest.mark.parametrize("args", [
    ("-m", "2"),
    ("-m", "2", "--bionj"),
    ("-m", "2", "--upgma"),
    ("-m", "1"),
    ("-m", "2", "-d", "4"),
    ("-m", "2", "--bootstrap", "3"),
], ids=["nj", "bionj", "upgma", "placement", "k2p", "bootstrap3"])
def test_complete_deletion_writes_the_newick_of_the_filtered_alignment(tmp_path, nt, args):
    r1, r2, o1, o2 = _pair(tmp_path, nt, *args)
    assert o1.read_bytes() == o2.read_bytes() and o1.read_text().count(",") == N - 1
    assert f"Sites: kept {nt.kept} of {L} (coverage >= 1 of {N} sequences)\n" in r1.stderr
    assert "Sites:" not in r2.stderr
    if "--bootstrap" in args:
        labels = set(re.findall(r"\)(\d+):", o1.read_text()))      # the support labels are part of the compared bytes
        assert labels and labels <= {"0", "33", "67", "100"}


def test_complete_deletion_changes_the_tree_file(tmp_path, nt):
    """the option is not a no-op on this alignment: pairwise deletion gives other branch lengths"""
    o1, o2 = tmp_path / "a.nwk", tmp_path / "b.nwk"
    assert run("-i", "m", "-I", nt.full, "-O", str(o1), "-m", "2").returncode == 0
    assert run("-i", "m", "-I", nt.full, "-O", str(o2), "-m", "2", "--complete-deletion").returncode == 0
    assert o1.read_bytes() != o2.read_bytes()


def test_site_coverage_threshold(tmp_path_factory, tmp_path):
    """partial deletion: 0.95 of 60 sequences is 57, a tie that is kept"""
    rng = np.random.default_rng(43)
    seqs = [bytearray(s) for s in _util.synth_alignment(rng, N, L, mean_bl=0.02, lo=0.002, hi=0.1)]
    _aa_ref.scatter(rng, seqs, 0.05, chars=b"-")
    a = Aln(tmp_path_factory.mktemp("sites_pm"), "T", seqs, "nt", permille=950)
    assert (a.cov == 57).any() and (a.cov == 56).any() and 0 < a.kept < L
    assert np.array_equal(a.keep, a.cov >= 57)
    r1, _, o1, o2 = _pair(tmp_path, a, "-m", "2", flag=("--site-coverage", "0.950"))
    assert o1.read_bytes() == o2.read_bytes()
    assert f"Sites: kept {a.kept} of {L} (coverage >= 0.95 of {N} sequences)\n" in r1.stderr


def test_complete_deletion_distance_matrix(tmp_path, nt):
    _, _, o1, o2 = _pair(tmp_path, nt, "-o", "d", "-d", "2")
    assert o1.read_bytes() == o2.read_bytes() and o1.read_text().split("\n")[0] == str(N)


def test_complete_deletion_protein(tmp_path, prot):
    r1, _, o1, o2 = _pair(tmp_path, prot, "--protein", "-m", "2", "-d", "8")
    assert o1.read_bytes() == o2.read_bytes() and o1.read_text().count(",") == N - 1
    assert f"Sites: kept {prot.kept} of {L} (coverage >= 1 of {N} sequences)\n" in r1.stderr


def test_complete_deletion_add_jplace(tmp_path, nt):
    """--add -o j: coverage over backbone and queries together; the two metadata fields only with the option"""
    m = 40
    fb, bb = tmp_path / "b.fa", tmp_path / "b.nwk"
    _util.write_fasta(str(fb), nt.names[:m], nt.seqs[:m])
    assert run("-i", "m", "-I", str(fb), "-O", str(bb), "-m", "2", "-d", "2").returncode == 0
    _, _, o1, o2 = _pair(tmp_path, nt, "--add", "-t", str(bb), "-o", "j", "-d", "2")
    d1, d2 = json.loads(o1.read_text()), json.loads(o2.read_text())
    assert d1["placements"] == d2["placements"] and d1["tree"] == d2["tree"] and len(d1["placements"]) == N - m
    assert d1["metadata"]["site_coverage"] == "1" and d1["metadata"]["sites_kept"] == nt.kept
    assert "site_coverage" not in d2["metadata"] and "sites_kept" not in d2["metadata"]
    assert {k: v for k, v in d1["metadata"].items() if k not in ("site_coverage", "sites_kept")} == d2["metadata"]


@pytest.mark.parametrize("extra", [(), ("--bootstrap", "3")], ids=["nj", "bootstrap3"])
def test_two_ranks_write_the_one_rank_bytes(tmp_path, nt, extra):
    o1, o2, o3 = tmp_path / "one.nwk", tmp_path / "two.nwk", tmp_path / "filtered.nwk"
    args = ["-i", "m", "-I", nt.full, "-m", "2", "--complete-deletion", *extra]
    r1 = run(*args, "-O", str(o1))
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = run(*args, "-O", str(o2), "--gpus", "2", "--devices", "0,0")
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "Ranks: 2" in r2.stderr, r2.stderr[-1500:]
    assert r2.stderr.count("Sites: kept") == 1
    assert o1.read_bytes() == o2.read_bytes()
    assert run("-i", "m", "-I", nt.filtered, "-m", "2", *extra, "-O", str(o3)).returncode == 0
    assert o1.read_bytes() == o3.read_bytes()


def test_no_site_kept_is_an_error_without_output(tmp_path):
    rng = np.random.default_rng(44)
    seqs = [bytearray(s) for s in _util.synth_alignment(rng, 12, 90, mean_bl=0.02, lo=0.002, hi=0.1)]
    for c in range(90):
        seqs[c % 12][c] = ord("-")      # a gap in every column: the best column holds 11 of 12
    fa, out = tmp_path / "g.fa", tmp_path / "g.nwk"
    _util.write_fasta(str(fa), [f"G{i}" for i in range(12)], [bytes(s) for s in seqs])
    r = run("-i", "m", "-I", str(fa), "-O", str(out), "-m", "2", "--complete-deletion")
    assert r.returncode == 1, r.stderr[-1500:]
    assert "best coverage: 11 of 12" in r.stderr and "--site-coverage 1" in r.stderr
    assert not out.exists()
    # the threshold the message points to works
    r = run("-i", "m", "-I", str(fa), "-O", str(out), "-m", "2", "--site-coverage", "0.916")
    assert r.returncode == 0 and "Sites: kept 90 of 90" in r.stderr and out.exists()


def test_without_gaps_the_option_changes_nothing(tmp_path):
    """the filter is a no-op on an alignment without gaps: the bytes of the plain command"""
    rng = np.random.default_rng(45)
    seqs = _util.synth_alignment(rng, N, L, mean_bl=0.02, lo=0.002, hi=0.1)
    fa = tmp_path / "c.fa"
    _util.write_fasta(str(fa), [f"C{i}" for i in range(N)], seqs)
    o1, o2 = tmp_path / "plain.nwk", tmp_path / "option.nwk"
    r1 = run("-i", "m", "-I", str(fa), "-O", str(o1), "-m", "2", "-d", "2")
    r2 = run("-i", "m", "-I", str(fa), "-O", str(o2), "-m", "2", "-d", "2", "--complete-deletion")
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-800:], r2.stderr[-800:])
    assert o1.read_bytes() == o2.read_bytes()
    assert "Sites:" not in r1.stderr and f"Sites: kept {L} of {L}" in r2.stderr
