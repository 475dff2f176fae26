"""`dipper --fit [--fit-taxa FILE]` on the GPU: the Newick file byte for byte the one written without the option; the `Fit:` line and the
per-taxon file, parsed back, equal to the library's doubles for the same pipeline (17 significant digits round-trip), for matrix and
alignment input under NJ, BIONJ, --nni, --spr, --upgma and --wpgma; the taxa listed in input order under the command's shuffle; a
deliberately misplaced sequence named first among the worst taxa; --protein and --site-coverage; a per-taxon file that cannot be written."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _fit_ref as R, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
VARIANTS = {"nj": (), "bionj": ("--bionj",), "nni": ("--nni", "2"), "spr": ("--spr", "2"), "upgma": ("--upgma",), "wpgma": ("--wpgma",)}


def run(*args, ok=True):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def sources(tmp_path_factory, orc):
    """per source: (arguments that name the input, tip names, a function that loads the same input into a context and builds its matrix)"""
    from dipper_amd import capi
    tmp = tmp_path_factory.mktemp("fit")
    out = {}
    n = 70
    D = R.noisy_matrix(np.random.default_rng(77), n)
    names = [f"X{i}" for i in range(n)]
    _util.write_phylip_lower(str(tmp / "d.phy"), names, D)
    Dr = np.zeros_like(D)      # -i d reads with float precision
    for i in range(n):
        for j in range(i):
            Dr[i, j] = Dr[j, i] = orc.phylip_value("%.9g" % D[i, j])

    def load_d(d):
        d.set_matrix_full(Dr)
        return lambda: d.dist_matrix(capi.SRC_MATRIX)
    out["d"] = (("-i", "d", "-I", str(tmp / "d.phy")), names, load_d)
    seqs = _util.synth_alignment(np.random.default_rng(41), n=80, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    names = [f"S{i+1}" for i in range(len(seqs))]
    _util.write_fasta(str(tmp / "a.fa"), names, seqs)

    def load_m(d):
        d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
        return lambda: d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    out["m"] = (("-i", "m", "-I", str(tmp / "a.fa"), "-m", "2", "-d", "2", "--seed", "-1"), names, load_m)
    out["m_file"] = str(tmp / "a.fa")
    return out


def library_fit(load, variant, n):
    """the command's pipeline through the library: the tree, a fresh matrix where the tree's builder consumed it, the fit"""
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        if variant == "bionj":
            d.set_nj_variant(1)
        build = load(d)
        build()
        if variant in ("upgma", "wpgma"):
            up = d.upgma(1 if variant == "wpgma" else 0)
            tree = capi.tree_from_upgma(up["merge_x"], up["merge_y"], up["height"])
        else:
            nj = d.nj_run()
            build()
            if variant in ("nni", "spr"):
                b = (d.bme_spr if variant == "spr" else d.bme_nni)(nj["merge_x"], nj["merge_y"], 2)
                tree = capi.tree_from_kids(b["kids"], b["top"], b["len"])
            else:
                tree = capi.tree_from_nj(nj["merge_x"], nj["merge_y"], nj["bl_x"], nj["bl_y"], nj["last_d"], n=n)
        return d.tree_fit(*tree)
    finally:
        d.close()


FIT_LINE = re.compile(r"Fit: (\d+) pairs \((\d+) skipped\), SS (\S+), rms (\S+), relative rms (\S+), explained variance (\S+), "
                      r"cophenetic correlation (\S+), worst pair (\S+) / (\S+) \(\|d - p\| = (\S+)\)")


def parse_fit(stderr):
    lines = [ln for ln in stderr.split("\n") if ln.startswith("Fit: ")]
    assert len(lines) == 2, stderr[-1500:]
    m = FIT_LINE.fullmatch(lines[0])
    assert m, lines[0]
    worst = re.fullmatch(r"Fit: worst taxa (.*)", lines[1])
    assert worst, lines[1]
    taxa = [re.fullmatch(r"(\S+) \(rms (\S+)\)", t) for t in worst.group(1).split(", ")]
    assert all(taxa)
    return m.groups(), [(t.group(1), float(t.group(2))) for t in taxa]


def parse_taxa(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "taxon\tpairs\tss\trms\trms_over_tree_rms" and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 5 for r in rows)
    return [r[0] for r in rows], np.array([int(r[1]) for r in rows]), np.array([[float(v) for v in r[2:]] for r in rows])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("src", ["d", "m"])
def test_fit_line_and_taxa_file_are_the_librarys_doubles(tmp_path, sources, src, variant):
    args, names, load = sources[src]
    n = len(names)
    plain, out, taxa = tmp_path / "plain.nwk", tmp_path / "fit.nwk", tmp_path / "taxa.tsv"
    r0 = run(*args, "-O", str(plain), *VARIANTS[variant])
    assert "Fit:" not in r0.stderr
    r = run(*args, "-O", str(out), *VARIANTS[variant], "--fit", "--fit-taxa", str(taxa))
    assert out.read_bytes() == plain.read_bytes()      # the tree file is the one written without the option
    ref = library_fit(load, variant, n)
    g, worst5 = parse_fit(r.stderr)
    assert (int(g[0]), int(g[1])) == (int(ref["n"]), int(ref["skipped"])) and int(g[0]) == n * (n - 1) // 2
    for text, k in zip((g[2], g[3], g[4], g[5], g[6], g[9]), ("ss", "rms", "rms_rel", "explained", "cophenetic", "max_e")):
        assert float(text) == ref[k], (k, text, ref[k])      # 17 digits round-trip
    assert (g[7], g[8]) == (names[ref["worst"][0]], names[ref["worst"][1]])
    tn, pairs, vals = parse_taxa(taxa)
    assert tn == names and np.array_equal(pairs, ref["taxon_pairs"])      # --seed -1 / -i d: slot order is input order
    rms = np.sqrt(ref["taxon_ss"] / ref["taxon_pairs"])
    assert np.array_equal(vals[:, 0], ref["taxon_ss"]) and np.array_equal(vals[:, 1], rms) and np.array_equal(vals[:, 2], rms / ref["rms"])
    order = sorted(range(n), key=lambda t: (-rms[t], t))[:5]
    assert worst5 == [(names[t], rms[t]) for t in order]


def test_taxa_file_is_in_input_order_under_the_shuffle(tmp_path, sources):
    """the default seed shuffles the sequences into slots: the file still lists them as the input does, each pair counted twice"""
    args, names, _ = sources["m"]
    args = args[:-2]      # without `--seed -1`
    taxa = tmp_path / "taxa.tsv"
    r = run(*args, "-O", str(tmp_path / "t.nwk"), "--fit", "--fit-taxa", str(taxa))
    g, _ = parse_fit(r.stderr)
    tn, pairs, vals = parse_taxa(taxa)
    n = len(names)
    assert tn == names and (pairs == n - 1).all() and int(g[0]) == n * (n - 1) // 2
    assert abs(vals[:, 0].sum() - 2 * float(g[2])) <= 1e-12 * float(g[2])


def test_a_misplaced_sequence_is_the_worst_taxon(tmp_path):
    """one taxon's sequence replaced by a copy of a distant one in half of the columns: no place in the tree explains its distances"""
    seqs = _util.synth_alignment(np.random.default_rng(23), n=60, L=2000, mean_bl=4e-2, lo=1e-2, hi=1.5e-1)
    arr = np.array([np.frombuffer(s, dtype=np.uint8) for s in seqs])
    k = 17
    far = int(np.argmax((arr != arr[k]).mean(axis=1)))
    L = arr.shape[1]
    mixed = arr[k].copy()
    mixed[: L // 2] = arr[far, : L // 2]
    seqs = [bytes(mixed) if i == k else s for i, s in enumerate(seqs)]
    names = [f"S{i+1}" for i in range(len(seqs))]
    _util.write_fasta(str(tmp_path / "a.fa"), names, seqs)
    r = run("-i", "m", "-I", str(tmp_path / "a.fa"), "-m", "2", "-d", "2", "-O", str(tmp_path / "t.nwk"), "--fit")
    _, worst5 = parse_fit(r.stderr)
    assert len(worst5) == 5 and worst5[0][0] == names[k], worst5


@pytest.mark.parametrize("extra", [("--protein", "-d", "8"), ("--site-coverage", "0.9")], ids=["protein", "site_coverage"])
def test_fit_with_protein_and_site_filter(tmp_path, extra):
    """valid where --nni is: the tree file unchanged, every pair counted"""
    from tests import _aa_ref
    if extra[0] == "--protein":
        seqs = _aa_ref.evolve_yule(np.random.default_rng(9), 40, 200)
    else:
        seqs = _util.synth_alignment(np.random.default_rng(12), n=40, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1, invalid_frac=0.02)
    names = [f"S{i+1}" for i in range(len(seqs))]
    _util.write_fasta(str(tmp_path / "a.fa"), names, seqs)
    args = ("-i", "m", "-I", str(tmp_path / "a.fa"), "-m", "2", *extra)
    run(*args, "-O", str(tmp_path / "plain.nwk"))
    r = run(*args, "-O", str(tmp_path / "fit.nwk"), "--fit")
    assert (tmp_path / "fit.nwk").read_bytes() == (tmp_path / "plain.nwk").read_bytes()
    g, worst5 = parse_fit(r.stderr)
    assert int(g[0]) + int(g[1]) == 40 * 39 // 2 and len(worst5) == 5 and float(g[3]) >= 0


def test_unwritable_taxa_file_ends_the_run_before_the_tree(tmp_path, sources):
    args, _, _ = sources["d"]
    r = run(*args, "-O", str(tmp_path / "t.nwk"), "--fit", "--fit-taxa", str(tmp_path / "no" / "dir" / "t.tsv"), ok=False)
    assert r.returncode != 0 and "--fit-taxa" in r.stderr and "Fit:" not in r.stderr
