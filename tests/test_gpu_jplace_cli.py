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


# ---- queries without a finite placement (left out of the file, which stays JSON) -----------------------------------
def _no_constant(name):
    raise AssertionError("not JSON: the bare token %s" % name)


class SaturatedCase:
    """the 40-tip saturated input of tests/test_gpu_place_fixed_edges.py on disk: query 0 is at +inf from every backbone tip (no
    finite placement), 63 and 64 at NaN (add = 0 on the lowest slot: finite), 129 at +inf from one clade only"""

    def __init__(self, tmp, orc):
        from tests import test_gpu_place_fixed_edges as E
        self.m = 40
        self.inp = E.saturated_input(orc, self.m, "plain")
        self.nwk = E.backbone(self.m, "random")
        self.n = len(self.inp.seqs)
        self.names = ["B%d" % k for k in range(self.m)] + ["Q%d" % k for k in range(self.n - self.m)]
        self.fasta, self.tree = tmp / "sat.fa", tmp / "sat.nwk"
        _util.write_fasta(self.fasta, self.names, self.inp.seqs, width=70)
        self.tree.write_text(self.nwk + "\n")
        self.args = ["-i", "m", "-I", str(self.fasta), "--add", "-t", str(self.tree), "-o", "j", "-d", "2"]

    def abi_rows(self, orc, replicates, seed):
        import dipper_amd
        from dipper_amd import capi
        d = dipper_amd.Dipper(0)
        try:
            d.set_msa(capi.pack4_many(self.inp.seqs), SITES_SAT)
            self.state, self.leaf_names = _jplace.backbone_arrays(orc, self.nwk, self.n)
            d.place_fixed_set(self.m, self.n, self.state)
            place = lambda: [_jplace.row_of(self.state, s, f, a) for s, f, a in zip(*d.place_fixed_run(capi.SRC_MSA, 2))]
            main, reps = place(), []
            for rep in range(replicates):
                d.msa_resample(seed, rep)
                reps.append(place())
        finally:
            d.close()
        return main, reps


SITES_SAT = 200
# Query 63 differs from every backbone tip in columns [40, 200) and nowhere else: p = 160/200 in the uploaded alignment (NaN under
# JC: add = 0, placed).  In a replicate that draws those columns exactly 150 times it is at p = 0.75, +inf, from everybody and
# has no finite placement there.  Replicate 0 of this seed is such a one (found on the host: dpr_msa_boot_weights), 1 and 2 are not.
BOOT_SEED, SATURATING_REPLICATE = 16, 0


@pytest.mark.parametrize("replicates", [0, 3])
def test_queries_without_a_finite_placement_are_left_out(tmp_path, orc, replicates):
    from dipper_amd import capi
    case = SaturatedCase(tmp_path, orc)
    extra = ["--bootstrap", str(replicates), "--bootstrap-seed", str(BOOT_SEED)] if replicates else []
    out, out2 = tmp_path / "s.jplace", tmp_path / "s2.jplace"
    r = run(*case.args, *extra, "-O", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(out.read_text(), parse_constant=_no_constant)
    main, reps = case.abi_rows(orc, replicates, BOOT_SEED)
    assert not _jplace.finite_row(main[0]) and main[0][2] == float("inf")           # the regime, from the ABI's own triples
    assert all(_jplace.finite_row(main[q]) and main[q][2] == 0.0 for q in (63, 64))
    differing = [int(capi.msa_boot_weights(BOOT_SEED, rep, SITES_SAT)[40:].sum()) for rep in range(3)]
    assert [k == 150 for k in differing] == [rep == SATURATING_REPLICATE for rep in range(3)], differing
    if replicates:                                        # ... and from the replicates': query 63 is at +inf there, and only there
        assert [_jplace.finite_row(rep[63]) for rep in reps] == [rep != SATURATING_REPLICATE for rep in range(3)]
        assert reps[SATURATING_REPLICATE][63][2] == float("inf")
    want = {case.names[case.m + q]: _jplace.tally(main[q], [rep[q] for rep in reps]) for q in range(len(main))}
    placed = [nm for nm in case.names[case.m:] if want[nm]]
    assert "Q0" not in placed and len(placed) < len(main)
    assert [p["n"] for p in doc["placements"]] == [[nm] for nm in placed]
    _, below, _, _ = _jplace.jplace_edges(doc["tree"])
    short = 0
    for p in doc["placements"]:
        rows = want[p["n"][0]]
        if not replicates:
            rows = [(e, 1, dl, pl) for e, _, dl, pl in rows]
        assert len(p["p"]) == len(rows)
        for (e, lik, lwr, dl, pl), (edge, count, distal, pendant) in zip(p["p"], rows):
            assert below[e] == _jplace.leaves_below_slot(case.state, 2 * edge, case.leaf_names)
            assert lik == 0 and float(lwr) == count / max(replicates, 1) and float(dl) == distal and float(pl) == pendant
        short += sum(row[1] for row in rows) < replicates
    left_out = len(main) - len(placed)
    lines = [ln for ln in r.stderr.splitlines() if "without a finite placement" in ln]
    assert len(lines) == 1 and (": %d (" % left_out) in lines[0] and "Q0" in lines[0], r.stderr[-1500:]
    if replicates:
        assert short > 0                                  # some replicate's placement of a placed query is not finite: its ratios sum to < 1
        q63 = next(p for p in doc["placements"] if p["n"] == ["Q63"])
        assert sum(round(row[2] * replicates) for row in q63["p"]) == replicates - 1
    r2 = run(*case.args, *extra, "-O", str(out2), "--devices", "0,0")
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert out.read_bytes() == out2.read_bytes()
    assert "Starting 2 ranks" in r2.stderr and [ln for ln in r2.stderr.splitlines() if "without a finite placement" in ln] == lines   # once, not per rank
