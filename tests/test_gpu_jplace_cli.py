"""`dipper --add -t BACKBONE -o j`: the jplace file of the command against the C ABI (dpr_place_fixed_set / _run, which
tests/test_gpu_place_fixed.py compares with the oracle) on the same input: 40 backbone tips, 70 queries, 300 sites.

Format: JSON, version 3, the five fields; the tree string is the -t file's text with {k} behind every branch length, k = 0 ..
2m - 3 ascending in post-order.  Placements: per query in input order; a row's edge is compared by the set of leaves below it
(robust to numbering), its lengths exactly (repr round trip of %.17g).  Bootstrap: the rows equal the tally recomputed through
the ABI, replicate by replicate.  Ranks: the same bytes with 2 and 3 rank processes on one device."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _jplace, _util
from tests.test_gpu_mash_place import _reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
M, NQ, SITES = 40, 70, 300
FIELDS = ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


class Case:
    """one input on disk: FASTA (backbone and queries interleaved), backbone tree, and the same by tip index for the ABI"""

    def __init__(self, tmp, kind, nq=NQ, seed=1):
        rng = np.random.default_rng(seed)
        self.kind, self.m, self.n = kind, M, M + nq
        self.nwk = _jplace.random_backbone(rng, M, "random")
        seqs = (_util.synth_alignment(rng, self.n, SITES, mean_bl=6e-3, lo=1e-3, hi=2e-2) if kind == "m"
                else _reads(rng, self.n, 1500, 2500))
        order = rng.permutation(self.n)                      # sequence k is backbone tip k (k < M) or query "Q<k - M>"
        label = lambda k: "B%d" % k if k < M else "Q%d" % (k - M)
        self.fasta = tmp / (kind + "_all.fa")
        _util.write_fasta(self.fasta, [label(k) for k in order], [seqs[k] for k in order], width=70)
        self.tree = tmp / (kind + "_bb.nwk")
        self.tree.write_text(self.nwk + "\n")
        queries = [k for k in order if k >= M]               # input order = tip order m, m + 1, ..
        self.query_names = [label(k) for k in queries]
        self.by_tip = [seqs[k] for k in range(M)] + [seqs[k] for k in queries]
        self.args = ["-i", kind, "-I", str(self.fasta), "--add", "-t", str(self.tree), "-o", "j"] + (["-d", "2"] if kind == "m" else [])

    def abi(self, orc):
        import dipper_amd
        from dipper_amd import capi
        d = dipper_amd.Dipper(0)
        if self.kind == "m":
            d.set_msa(capi.pack4_many(self.by_tip), SITES)
        else:
            d.set_reads(self.by_tip)
            d.sketch(k=15, S=1000, fetch=False)
        self.state, self.leaf_names = _jplace.backbone_arrays(orc, self.nwk, self.n)
        d.place_fixed_set(self.m, self.n, self.state)
        return d

    def place(self, d):
        from dipper_amd import capi
        slot, frac, add = d.place_fixed_run(capi.SRC_MSA, 2) if self.kind == "m" else d.place_fixed_run(capi.SRC_MASH, 0, k=15)
        return [_jplace.row_of(self.state, s, f, a) for s, f, a in zip(slot, frac, add)]


def load(path, case):
    """the file, checked for its format; returns (document, {edge number: leaves below})"""
    doc = json.loads(path.read_text())
    assert doc["version"] == 3 and doc["fields"] == FIELDS
    assert set(doc) == {"version", "tree", "fields", "placements", "metadata"}
    plain, below, labels, _ = _jplace.jplace_edges(doc["tree"])
    assert labels == list(range(2 * case.m - 2))              # each once, ascending in post-order
    assert plain == case.nwk                                  # topology, names, child order and lengths of the -t file
    assert [p["n"] for p in doc["placements"]] == [[nm] for nm in case.query_names]
    meta = json.dumps(doc["metadata"])
    assert doc["metadata"]["software"] == "dipper" and "devices" not in meta and "--" not in meta and str(case.fasta) not in meta
    return doc, below


@pytest.mark.parametrize("kind", ["m", "r"])
def test_placements_equal_the_abi(tmp_path, orc, kind):
    case = Case(tmp_path, kind)
    out = tmp_path / "o.jplace"
    r = run(*case.args, "-O", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    doc, below = load(out, case)
    d = case.abi(orc)
    try:
        ref = case.place(d)
    finally:
        d.close()
    assert len(doc["placements"]) == NQ
    for p, (edge, distal, pendant) in zip(doc["placements"], ref):
        assert len(p["p"]) == 1
        e, lik, lwr, dl, pl = p["p"][0]
        assert below[e] == _jplace.leaves_below_slot(case.state, 2 * edge, case.leaf_names)
        assert (lik, lwr) == (0, 1) and float(dl) == distal and float(pl) == pendant
        assert dl >= 0.0 and pl >= 0.0
    assert doc["metadata"]["distance"] == ("JC" if kind == "m" else "mash")


def test_bootstrap_rows_equal_the_tally_through_the_abi(tmp_path, orc):
    case = Case(tmp_path, "m")
    out, out2 = tmp_path / "b.jplace", tmp_path / "b2.jplace"
    r = run(*case.args, "--bootstrap", "7", "--bootstrap-seed", "3", "-O", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    doc, below = load(out, case)
    assert doc["metadata"]["bootstrap_replicates"] == 7 and doc["metadata"]["bootstrap_seed"] == 3
    d = case.abi(orc)
    try:
        main = case.place(d)
        reps = []
        for rep in range(7):
            d.msa_resample(3, rep)
            reps.append(case.place(d))
    finally:
        d.close()
    several = 0
    for q, p in enumerate(doc["placements"]):
        want = _jplace.tally(main[q], [reps[rep][q] for rep in range(7)])
        assert len(p["p"]) == len(want)
        for (e, lik, lwr, dl, pl), (edge, count, distal, pendant) in zip(p["p"], want):
            assert below[e] == _jplace.leaves_below_slot(case.state, 2 * edge, case.leaf_names)
            assert lik == 0 and float(lwr) == count / 7 and float(dl) == distal and float(pl) == pendant
        assert sum(round(row[2] * 7) for row in p["p"]) == 7
        several += len(want) > 1
    assert several > 0                                        # 300 sites: some query moves in some replicate
    r = run(*case.args, "--bootstrap", "7", "--bootstrap-seed", "4", "-O", str(out2))
    assert r.returncode == 0, r.stderr[-2000:]
    doc2, _ = load(out2, case)
    assert doc2["placements"] != doc["placements"] and doc2["metadata"]["bootstrap_seed"] == 4


@pytest.mark.parametrize("kind,devices,extra,nq", [
    ("m", "0,0", ["--bootstrap", "7", "--bootstrap-seed", "3"], NQ),
    ("r", "0,0,0", [], NQ),
    ("m", "0,0", [], 300),                                    # shares of 256 and 44 queries: both ranks place
])
def test_ranks_write_the_same_bytes(tmp_path, kind, devices, extra, nq):
    case = Case(tmp_path, kind, nq=nq)
    o1, oG = tmp_path / "one.jplace", tmp_path / "ranks.jplace"
    r1 = run(*case.args, *extra, "-O", str(o1))
    assert r1.returncode == 0, r1.stderr[-2000:]
    rG = run(*case.args, *extra, "-O", str(oG), "--devices", devices)
    assert rG.returncode == 0, rG.stderr[-3000:]
    n = len(devices.split(","))
    assert f"Starting {n} ranks" in rG.stderr and f"Ranks: {n} (transport ipc" in rG.stderr, rG.stderr[-1500:]
    assert o1.read_bytes() == oG.read_bytes() and len(json.loads(o1.read_text())["placements"]) == nq


def test_no_output_file_after_a_usage_error(tmp_path):
    case = Case(tmp_path, "m")
    out = tmp_path / "u.jplace"
    r = run(*case.args, "--bootstrap", "5", "--bootstrap-metric", "tbe", "-O", str(out))
    assert r.returncode == 1 and "\033[31m" in r.stderr and not out.exists()
