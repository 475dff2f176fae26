"""GPU: `dipper -d 9|10|11` end to end on 200 tips x 1 000 sites -- conventional NJ, two ranks on one GPU, bootstrap labels and
--add -o j (tests/test_gpu_pairtable.py compares the ABI's distances with the reference)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
N, L = 200, 1000


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def aln(tmp_path_factory):
    rng = np.random.default_rng(41)
    seqs = _util.synth_alignment(rng, N, L, mean_bl=2e-2, lo=2e-3, hi=1e-1, invalid_frac=0.01)
    names = [f"S{i+1}" for i in range(N)]
    fa = tmp_path_factory.mktemp("pairtable") / "a.fa"
    _util.write_fasta(str(fa), names, seqs, width=70)
    return fa, names, seqs


def _tips(text):
    return sorted(_util.parse_newick(text)[2].values())


@pytest.mark.parametrize("dt", ["9", "10", "11"])
def test_nj_tree_holds_every_tip(tmp_path, aln, dt):
    fa, names, _ = aln
    out = tmp_path / "o.nwk"
    r = run("-i", "m", "-I", str(fa), "-O", str(out), "-m", "2", "-d", dt)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _tips(out.read_text()) == sorted(names)


def test_two_ranks_write_the_one_rank_newick(tmp_path, aln):
    fa, names, _ = aln
    o1, o2 = tmp_path / "one.nwk", tmp_path / "two.nwk"
    args = ["-i", "m", "-I", str(fa), "-m", "2", "-d", "11"]
    r1 = run(*args, "-O", str(o1))
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = run(*args, "-O", str(o2), "--devices", "0,0")       # --gpus 2 with both ranks on the GPU of the box
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "Starting 2 ranks" in r2.stderr, r2.stderr[-1500:]
    assert o1.read_bytes() == o2.read_bytes() and o1.read_text().count(",") == len(names) - 1


def test_bootstrap_labels(tmp_path, aln):
    fa, names, _ = aln
    out = tmp_path / "b.nwk"
    r = run("-i", "m", "-I", str(fa), "-O", str(out), "-m", "2", "-d", "9", "--bootstrap", "3")
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    assert _tips(re.sub(r"\)\d+", ")", text)) == sorted(names)
    labels = re.findall(r"\)([^:;,()]+)", text)
    assert len(labels) >= len(names) // 2
    assert all(re.fullmatch(r"\d+", lab) and 0 <= int(lab) <= 100 for lab in labels), labels[:8]


def test_add_writes_jplace_naming_the_model(tmp_path, aln):
    fa, names, seqs = aln
    m = 150
    fb, bb = tmp_path / "b.fa", tmp_path / "b.nwk"
    _util.write_fasta(str(fb), names[:m], seqs[:m])
    assert run("-i", "m", "-I", str(fb), "-O", str(bb), "-m", "2", "-d", "10").returncode == 0
    jp = tmp_path / "q.jplace"
    r = run("-i", "m", "-I", str(fa), "-O", str(jp), "--add", "-t", str(bb), "-d", "10", "-o", "j")
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(jp.read_text())
    assert doc["metadata"]["distance"] == "LogDet"
    assert sorted(p["n"][0] for p in doc["placements"]) == sorted(names[m:])
