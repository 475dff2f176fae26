"""`dipper --upgma` / `--wpgma` on the GPU: the rooted Newick text against text assembled here from dpr_upgma_host on the matrix
the command computes (the library's own, the numbers `-o d` prints), for every distance source; that the written tree is
ultrametric; the stderr line; `--bootstrap` with either metric and the per-taxon report against a recomputation from replicate
alignments; the command without the option; several ranks."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _taxa, _tbe, _upgma_ref as R, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
OPT = {0: "--upgma", 1: "--wpgma"}
WORD = {0: "UPGMA", 1: "WPGMA"}


def run(*args, ok=True):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def library_matrix(kind, seqs, dist_type):
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        if kind == "m":
            d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
            d.dist_matrix(capi.SRC_MSA, dist_type)
        elif kind == "aa":
            d.set_msa_aa(capi.pack_aa_many(seqs))
            d.dist_matrix(capi.SRC_MSA, dist_type)
        else:
            d.set_reads(seqs)
            d.sketch(k=15, S=1000, fetch=False)
            d.dist_matrix(capi.SRC_MASH, k=15)
        return d.matrix()
    finally:
        d.close()


@pytest.fixture(scope="module")
def sources(tmp_path_factory, orc):
    """per source: (arguments that name the input, tip names, the matrix the command computes from it)"""
    tmp = tmp_path_factory.mktemp("upgma")
    out = {}
    # -i d: a PHYLIP file, read with float precision
    n = 90
    D = R.noisy_matrix(np.random.default_rng(77), n)
    names = [f"X{i}" for i in range(n)]
    _util.write_phylip_lower(str(tmp / "d.phy"), names, D)
    Dr = np.zeros_like(D)
    for i in range(n):
        for j in range(i):
            Dr[i, j] = Dr[j, i] = orc.phylip_value("%.9g" % D[i, j])
    out["d"] = (("-i", "d", "-I", str(tmp / "d.phy")), names, Dr)
    # -i m: a nucleotide alignment, JC
    seqs = _util.synth_alignment(np.random.default_rng(41), n=120, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    names = [f"S{i+1}" for i in range(len(seqs))]
    _util.write_fasta(str(tmp / "a.fa"), names, seqs)
    out["m"] = (("-i", "m", "-I", str(tmp / "a.fa"), "-m", "2", "-d", "2", "--seed", "-1"), names, library_matrix("m", seqs, 2))
    out["m_seqs"] = seqs
    # -i m --protein -d 8
    aa = _aa_ref.evolve_yule(np.random.default_rng(9), 60, 200)
    names = [f"P{i+1}" for i in range(len(aa))]
    _util.write_fasta(str(tmp / "p.fa"), names, aa)
    out["aa"] = (("-i", "m", "--protein", "-I", str(tmp / "p.fa"), "-m", "2", "-d", "8", "--seed", "-1"), names, library_matrix("aa", aa, 8))
    # -i r: unaligned reads, Mash distances
    reads = _util.synth_reads(np.random.default_rng(5), 40, 3000, mean_bl=2e-2, lo=2e-3, hi=1e-1)
    names = [f"R{i+1}" for i in range(len(reads))]
    _util.write_fasta(str(tmp / "r.fa"), names, reads)
    out["r"] = (("-i", "r", "-I", str(tmp / "r.fa"), "-m", "2", "--seed", "-1"), names, library_matrix("r", reads, 0))
    return out


def root_path_lengths(text, names):
    kids, length, name, root = _util.parse_newick(text)
    assert len(kids[root]) == 2 and root not in name      # rooted and binary at the top, no label on the root
    out = {}
    st = [(root, 0.0)]
    while st:
        v, d = st.pop()
        if not kids[v]:
            out[name[v]] = d
        for c in kids[v]:
            st.append((c, d + length[c]))
    assert sorted(out) == sorted(names)
    return np.array([out[nm] for nm in names])


@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
@pytest.mark.parametrize("src", ["d", "m", "aa", "r"])
def test_newick_text_is_the_host_tree_and_is_ultrametric(tmp_path, sources, src, linkage):
    from dipper_amd import capi
    args, names, M = sources[src]
    n = len(names)
    out = tmp_path / "t.nwk"
    r = run(*args, "-O", str(out), OPT[linkage])
    ref = capi.upgma_host(M, linkage)
    text = out.read_text()
    assert text == R.newick(names, ref["merge_x"], ref["merge_y"], ref["height"])
    assert text.startswith("(") and text.endswith(");\n") and text.count("(") == n - 1
    # every tip at the root's height: six printed digits a branch, summed along a path of at most n - 1 branches
    paths = root_path_lengths(text, names)
    top = float(ref["height"][-1])
    print(WORD[linkage], src, "root height", top, "largest deviation of a root path", np.abs(paths / top - 1).max())
    assert np.all(np.abs(paths - top) <= 1e-5 * top)
    line = [ln for ln in r.stderr.split("\n") if ln.startswith(WORD[linkage] + ": ")]
    assert len(line) == 1 and re.fullmatch(rf"{WORD[linkage]}: {n} tips, root height {re.escape('%g' % top)}, \d+ rows rescanned", line[0]), r.stderr[-600:]
    assert 2 * (n - 2) <= int(line[0].split(", ")[2].split(" ")[0]) <= sum(n - it for it in range(n - 2))
    assert f"Using {WORD[linkage]}" in r.stderr and WORD[1 - linkage] + ":" not in r.stderr


@pytest.mark.parametrize("src", ["m", "aa", "r"])
def test_matrix_output_of_the_command_is_that_matrix(tmp_path, sources, src):
    """`-o d` of the same input prints the matrix the trees above were held to, nine digits a value (-i d: the input is the matrix)"""
    args, names, M = sources[src]
    phy = tmp_path / "d.phy"
    run(*args, "-o", "d", "-O", str(phy))
    lines = phy.read_text().strip().split("\n")
    assert int(lines[0]) == len(names)
    for i, ln in enumerate(lines[1:]):
        f = ln.split("\t")
        assert f[0] == names[i] and f[1:] == ["%.9g" % v for v in M[i, :i]], i


# ---- --bootstrap -------------------------------------------------------------------------------------------------------------
BOOT_SEED, BOOT_N = 11, 5


@pytest.fixture(scope="module")
def replicates(sources):
    """per linkage: the main log and the replicate logs (n - 2 entries each), from replicate alignments built here out of
    capi.msa_boot_weights, the library's distances on them and dpr_upgma_host"""
    from dipper_amd import capi
    seqs, M = sources["m_seqs"], sources["m"][2]
    L = len(seqs[0])
    out = {}
    mats = []
    for r in range(BOOT_N):
        idx = np.repeat(np.arange(L), capi.msa_boot_weights(BOOT_SEED, r, L))
        mats.append(library_matrix("m", [np.frombuffer(s, dtype=np.uint8)[idx].tobytes() for s in seqs], 2))
    for linkage in (0, 1):
        out[linkage] = (capi.upgma_host(M, linkage), [capi.upgma_host(Mr, linkage) for Mr in mats])
    return out


def boot_args(sources, linkage):
    return [*sources["m"][0], OPT[linkage], "--bootstrap", str(BOOT_N), "--bootstrap-seed", str(BOOT_SEED)]


def expected_labels(n, main, reps, metric):
    from dipper_amd import capi
    mx, my = main["merge_x"][: n - 2], main["merge_y"][: n - 2]
    p = _tbe.p_of(n, mx, my)
    if metric == "fbp":
        counts = np.zeros(n - 2, dtype=np.int32)
        for rep in reps:
            capi.split_support(n, mx, my, rep["merge_x"], rep["merge_y"], counts)
        return [int((200 * int(counts[k]) + BOOT_N) // (2 * BOOT_N)) if p[k] >= 2 else None for k in range(n - 2)]
    phi = np.zeros(n - 2, dtype=np.int64)
    for rep in reps:
        capi.transfer_support_host(n, mx, my, rep["merge_x"], rep["merge_y"], phi)
    return [int((200 * (BOOT_N * (p[k] - 1) - int(phi[k])) + BOOT_N * (p[k] - 1)) // (2 * BOOT_N * (p[k] - 1))) if p[k] >= 2 else None
            for k in range(n - 2)]


@pytest.mark.parametrize("linkage", [0, 1], ids=["upgma", "wpgma"])
@pytest.mark.parametrize("metric", ["fbp", "tbe"])
def test_bootstrap_labels(tmp_path, sources, replicates, metric, linkage):
    _, names, _ = sources["m"]
    n = len(names)
    main, reps = replicates[linkage]
    out = tmp_path / "b.nwk"
    r = run(*boot_args(sources, linkage), "--bootstrap-metric", metric, "-O", str(out))
    labels = expected_labels(n, main, reps, metric)
    assert sum(v is not None for v in labels) >= n // 2 and len({v for v in labels if v is not None}) > 3      # (not a comparison of nothing)
    text = out.read_text()
    assert text == R.newick(names, main["merge_x"], main["merge_y"], main["height"], labels)
    assert re.sub(r"\)\d+", ")", text) == R.newick(names, main["merge_x"], main["merge_y"], main["height"])
    assert f"Bootstrap: {BOOT_N} replicates (seed {BOOT_SEED}) in " in r.stderr and f"{WORD[linkage]}: {n} tips, root height " in r.stderr


def test_bootstrap_taxa_report(tmp_path, sources, replicates):
    from dipper_amd import capi
    _, names, _ = sources["m"]
    n = len(names)
    main, reps = replicates[0]
    out, taxa = tmp_path / "b.nwk", tmp_path / "taxa.tsv"
    run(*boot_args(sources, 0), "-O", str(out), "--bootstrap-taxa", str(taxa))
    assert out.read_text() == R.newick(names, main["merge_x"], main["merge_y"], main["height"], expected_labels(n, main, reps, "fbp"))
    mx, my = main["merge_x"][: n - 2], main["merge_y"][: n - 2]
    moved, pairs = np.zeros(n, dtype=np.int64), np.zeros(1, dtype=np.int64)
    for rep in reps:      # (--seed -1: the slots are the input order, the report's numbering)
        capi.transfer_taxa_host(n, mx, my, rep["merge_x"], rep["merge_y"], 300, None, moved, pairs)
    head, rows = _taxa.read_report(taxa)
    B = len(_taxa.branches(n, mx, my))
    assert head == {"replicates": str(BOOT_N), "seed": str(BOOT_SEED), "cutoff": "0.300", "branches": str(B), "pairs": str(int(pairs[0]))}
    assert pairs[0] > 0 and moved.sum() > 0
    assert rows == [(names[t], int(moved[t]), _taxa.index_text(moved[t], int(pairs[0]))) for t in range(n)]


# ---- without the option, several ranks -------------------------------------------------------------------------------------------
def test_without_the_option_nothing_changes(tmp_path, sources):
    from dipper_amd import capi
    args, names, M = sources["m"]
    a, b = tmp_path / "a.nwk", tmp_path / "b.nwk"
    r = run(*args, "-O", str(a))
    at = args.index("-m")
    run(*args[:at], *args[at + 2:], "-O", str(b))      # the default mode below 30 000 sequences
    g = capi.nj_variant_host(0, M)
    assert a.read_text() == _util.newick_from_merges(names, g["merge_x"], g["merge_y"], g["bl_x"], g["bl_y"], g["last_d"])
    assert a.read_bytes() == b.read_bytes()
    assert "UPGMA" not in r.stderr and "WPGMA" not in r.stderr and "Using conventional NJ" in r.stderr


def test_default_mode_at_30000_sequences_names_the_mode(tmp_path):
    """decided once the input is read: 30 000 sequences select placement in the default mode, where no tree is clustered"""
    n = 30000
    rng = np.random.default_rng(1)
    seqs = [bytes(row) for row in np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 24))]]
    fa, out = tmp_path / "many.fa", tmp_path / "o.nwk"
    _util.write_fasta(str(fa), [f"T{i}" for i in range(n)], seqs)
    r = run("-i", "m", "-I", str(fa), "-O", str(out), "--wpgma", ok=False)
    assert r.returncode != 0 and "--wpgma" in r.stderr and "30000 sequences select placement" in r.stderr and "use -m 2" in r.stderr, r.stderr[-600:]
    assert not out.exists() or out.read_text() == ""


def test_several_ranks_are_a_usage_error(tmp_path, sources):
    args, _, _ = sources["m"]
    out = tmp_path / "o.nwk"
    r = run(*args, "-O", str(out), "--upgma", "--devices", "0,0", ok=False)
    assert r.returncode == 1 and "--upgma runs on one GPU" in r.stderr.split("DIPPER Command Line Arguments")[0]
    assert not out.exists()
