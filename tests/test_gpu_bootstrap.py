"""GPU tests of the bootstrap support: the device resample against a context given the host-built replicate alignment, and
`dipper --bootstrap N` against N plain runs of the command on host-written replicate FASTA files."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GEN = os.path.join(ROOT, "tools", "bin", "gen_synth")


def replicate_seqs(seqs, seed, r):
    """the replicate alignment: every column c, ascending, repeated w[c] times (bytes)"""
    from dipper_amd import capi
    L = len(seqs[0])
    idx = np.repeat(np.arange(L), capi.msa_boot_weights(seed, r, L))
    return [np.frombuffer(s, dtype=np.uint8)[idx].tobytes() for s in seqs]


@pytest.mark.parametrize("L", [33, 700, 2080, 2500, 33000])
@pytest.mark.parametrize("invalid", [0.0, 0.02])
def test_resample_equals_host_replicate(orc, L, invalid):
    """the resampled planes (and, through msa_restage, their stage bitmap) equal an upload of the host-built replicate, and the
    replicate's distances equal the oracle's on that replicate under _util.assert_msa_dist, every type"""
    import dipper_amd
    from dipper_amd import capi
    rng = np.random.default_rng(L + int(invalid * 1000))
    n = 257 if L < 10000 else 40
    seqs = _util.synth_alignment(rng, n=n, L=L, mean_bl=2e-3, lo=2e-4, hi=2e-2, invalid_frac=invalid)
    seed, r = 11, 3
    a, b = dipper_amd.Dipper(0), dipper_amd.Dipper(0)
    try:
        a.set_msa(capi.pack4_many(seqs), L)
        rep_packed = capi.pack4_many(replicate_seqs(seqs, seed, r))
        b.set_msa(rep_packed, L)
        orig = {}
        for d in range(1, 7):
            a.dist_matrix(capi.SRC_MSA, d)
            orig[d] = a.matrix()
        a.msa_resample(seed, r)
        assert np.array_equal(a.msa_boot_weights(L), capi.msa_boot_weights(seed, r, L))
        for d in range(1, 7):
            a.dist_matrix(capi.SRC_MSA, d)
            b.dist_matrix(capi.SRC_MSA, d)
            Da, Db = a.matrix(), b.matrix()
            assert np.array_equal(np.isnan(Da), np.isnan(Db)) and np.array_equal(Da, Db, equal_nan=True), d
            blk_a, _ = a.msa_dist_block(min(40, n - 1), min(100, n - min(40, n - 1)), n, dist_type=d)
            blk_b, _ = b.msa_dist_block(min(40, n - 1), min(100, n - min(40, n - 1)), n, dist_type=d)
            assert np.array_equal(blk_a, blk_b, equal_nan=True), d
            lo = np.tril_indices(n, -1)
            _util.assert_msa_dist(Da[lo], orc.msa_dist_lower_mt(rep_packed, L, d)[lo], d, f"replicate L={L}")
        for row in (1, min(100, n - 1), n - 1):
            ua, ma = a.msa_counts(row)
            ub, mb = b.msa_counts(row)
            assert np.array_equal(ua, ub) and np.array_equal(ma, mb)
        # the same replicate again (from the replicate state), then back to the uploaded alignment
        a.dist_matrix(capi.SRC_MSA, 2)
        D1 = a.matrix()
        a.msa_resample(seed, 0)
        a.msa_resample(seed, r)
        a.dist_matrix(capi.SRC_MSA, 2)
        assert np.array_equal(a.matrix(), D1, equal_nan=True)
        a.msa_resample(seed, -1)
        for d in (2, 4):
            a.dist_matrix(capi.SRC_MSA, d)
            assert np.array_equal(a.matrix(), orig[d], equal_nan=True), d
        with pytest.raises(capi.DipperError):
            a.msa_boot_weights(L)                     # no replicate active
    finally:
        a.close()
        b.close()


def test_resample_needs_an_alignment():
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        with pytest.raises(capi.DipperError) as ei:
            d.msa_resample(1, 0)
        assert ei.value.code == -3
        assert list(d.comm_sum_i32([1, 2, 3])) == [1, 2, 3]     # one rank: nothing to add
    finally:
        d.close()


# ---- the command ---------------------------------------------------------------------------------------------------------
def run(*args, timeout=600):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def read_fasta(path):
    names, seqs, cur = [], [], []
    for line in open(path, "rb"):
        line = line.strip()
        if line.startswith(b">"):
            if names:
                seqs.append(b"".join(cur))
            names.append(line[1:].split()[0].decode())
            cur = []
        elif line:
            cur.append(line)
    seqs.append(b"".join(cur))
    return names, seqs


def strip_labels(text):
    return re.sub(r"\)\d+", ")", text)


def labelled_nodes(text, names):
    """(split as the side without names[0], label or None, non-trivial?) of every internal node below the root"""
    kids, _, name, root = _util.parse_newick(text)
    assert root not in name                  # the root carries no label
    idx = {nm: i for i, nm in enumerate(names)}
    order, st = [], [root]
    while st:
        v = st.pop()
        order.append(v)
        st.extend(kids[v])
    below = {}
    for v in reversed(order):
        below[v] = frozenset([idx[name[v]]]) if not kids[v] else frozenset().union(*[below[c] for c in kids[v]])
    full, n = frozenset(range(len(names))), len(names)
    return [(below[v] if 0 not in below[v] else full - below[v], name.get(v), 1 < len(below[v]) < n - 1)
            for v in order if kids[v] and v != root]


def check_labels(text, names, rep_splits):
    N = len(rep_splits)
    nodes = labelled_nodes(text, names)
    assert any(nt for _, _, nt in nodes)
    for split, lab, nontrivial in nodes:
        if not nontrivial:
            assert lab is None
            continue
        count = sum(split in s for s in rep_splits)
        assert lab is not None and int(lab) == (200 * count + N) // (2 * N), (lab, count, N)


def independent_splits(tmp_path, names, seqs, seed, N, args, tag):
    out = []
    for r in range(N):
        fa, o = tmp_path / f"{tag}_rep{r}.fa", tmp_path / f"{tag}_rep{r}.nwk"
        _util.write_fasta(fa, names, replicate_seqs(seqs, seed, r))
        run("-i", "m", "-I", str(fa), "-O", str(o), *args)
        out.append(_util.splits(o.read_text(), names))
    return out


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("boot")
    p = d / "aln.fa"
    r = subprocess.run([GEN, "--tips", "150", "--sites", "600", "--seed", "5", "--mean-bl", "0.02", "--lo", "0.002", "--hi", "0.2",
                        "--model", "gtr+g+i", "--indel-gaps", "--fasta", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return p


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dist", ["2", "4"])
def test_cli_labels_equal_independent_runs(tmp_path, small, dist):
    args = ["-d", dist, "--seed", "3", "-m", "2"]
    ob, op = tmp_path / "boot.nwk", tmp_path / "plain.nwk"
    r = run("-i", "m", "-I", str(small), "-O", str(ob), *args, "--bootstrap", "6", "--bootstrap-seed", "11")
    assert "Bootstrap: 6 replicates (seed 11) in " in r.stderr and ", 1 ranks" in r.stderr
    run("-i", "m", "-I", str(small), "-O", str(op), *args)
    text, plain = ob.read_text(), op.read_text()
    assert strip_labels(text) == plain and text != plain
    names, seqs = read_fasta(small)
    check_labels(text, names, independent_splits(tmp_path, names, seqs, 11, 6, args, "d" + dist))
    if dist == "2":
        # the default mode below 30 000 sequences is conventional NJ: the same file
        od = tmp_path / "default.nwk"
        run("-i", "m", "-I", str(small), "-O", str(od), "-d", dist, "--seed", "3", "--bootstrap", "6", "--bootstrap-seed", "11")
        assert od.read_text() == text


@pytest.mark.timeout(600)
@pytest.mark.parametrize("devices,N", [("0,0", 5), ("0,0,0", 2)])
def test_cli_ranks_byte_identical(tmp_path, small, devices, N):
    args = ["-i", "m", "-I", str(small), "-d", "2", "--seed", "3", "-m", "2", "--bootstrap", str(N), "--bootstrap-seed", "7"]
    o1, oG = tmp_path / "one.nwk", tmp_path / "many.nwk"
    run(*args, "-O", str(o1))
    r = run(*args, "-O", str(oG), "--devices", devices)
    G = len(devices.split(","))
    assert f"Starting {G} ranks" in r.stderr and f"{G} ranks" in [l for l in r.stderr.splitlines() if l.startswith("Bootstrap:")][0]
    assert oG.read_bytes() == o1.read_bytes()


@pytest.mark.timeout(900)
def test_cli_natural_size(tmp_path):
    p = tmp_path / "big.fa"
    r = subprocess.run([GEN, "--tips", "6000", "--sites", "1500", "--seed", "9", "--mean-bl", "0.004", "--lo", "0.0004", "--hi", "0.04",
                        "--model", "gtr+g+i", "--indel-gaps", "--fasta", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = ["-d", "2", "--seed", "1", "-m", "2"]
    ob, op = tmp_path / "boot.nwk", tmp_path / "plain.nwk"
    run("-i", "m", "-I", str(p), "-O", str(ob), *args, "--bootstrap", "2")
    run("-i", "m", "-I", str(p), "-O", str(op), *args)
    text = ob.read_text()
    assert strip_labels(text) == op.read_text()
    names, seqs = read_fasta(p)
    check_labels(text, names, independent_splits(tmp_path, names, seqs, 1, 2, args, "big"))
