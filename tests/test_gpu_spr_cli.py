"""`dipper --spr R`: the tree of dpr_bme_spr_host on the same distances, its stderr line, `--spr 0` against `--nni 0`, the
command without the option, and the usage errors (those need no GPU: they are decided from the arguments alone)."""
import os
import subprocess

import numpy as np
import pytest

from tests import _bme_ref as R, _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
gpu = pytest.mark.gpu


def run(*args):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def spr_line(ref):
    return (f", {ref['moves']} moves ({ref['long_moves']} beyond NNI, longest {ref['max_k']}), {ref['rounds']} rounds, "
            f"{ref['fallbacks']} fallbacks")


@pytest.fixture(scope="module")
def aln(tmp_path_factory):
    import dipper_amd
    from dipper_amd import capi
    seqs = _util.synth_alignment(np.random.default_rng(41), n=120, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    names = [f"S{i+1}" for i in range(len(seqs))]
    fa = tmp_path_factory.mktemp("spr") / "a.fa"
    _util.write_fasta(str(fa), names, seqs)
    d = dipper_amd.Dipper(0)
    try:
        d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
        d.dist_matrix(capi.SRC_MSA, 2)
        return fa, names, d.matrix()
    finally:
        d.close()


@gpu
@pytest.mark.parametrize("variant,rounds", [(0, 0), (0, 20), (1, 20)], ids=["spr0", "spr20", "bionj_spr20"])
def test_cli_alignment_input(tmp_path, aln, variant, rounds):
    from dipper_amd import capi
    fa, names, M = aln
    out = tmp_path / "t.nwk"
    base = ("-i", "m", "-I", str(fa), "-m", "2", "-d", "2", "--seed", "-1", *(["--bionj"] if variant else []))
    r = run(*base, "-O", str(out), "--spr", str(rounds))
    g = capi.nj_variant_host(variant, M)
    ref = capi.bme_spr_host(M, g["merge_x"], g["merge_y"], rounds)
    assert out.read_text() == R.newick(names, ref["kids"], ref["top"], ref["len"])
    line = [ln for ln in r.stderr.split("\n") if ln.startswith("BME SPR: L ")]
    assert len(line) == 1 and " -> " in line[0] and line[0].endswith(spr_line(ref)), r.stderr[-800:]
    assert not [ln for ln in r.stderr.split("\n") if ln.startswith("BME NNI:")]
    if rounds == 0:
        nni, plain = tmp_path / "n.nwk", tmp_path / "p.nwk"
        q = run(*base, "-O", str(nni), "--nni", "0")
        assert nni.read_bytes() == out.read_bytes() and "BME NNI:" in q.stderr and "BME SPR:" not in q.stderr
        p = run(*base, "-O", str(plain))                                  # without the option: the NJ tree, and no line
        assert plain.read_text() == _util.newick_from_merges(names, g["merge_x"], g["merge_y"], g["bl_x"], g["bl_y"], g["last_d"])
        assert "BME" not in p.stderr


@gpu
def test_cli_matrix_input(tmp_path, orc):
    from dipper_amd import capi
    n = 150
    D = R.random_matrix(np.random.default_rng(357), 257)[:n, :n]
    names = [f"X{i}" for i in range(n)]
    phy, out = tmp_path / "d.phy", tmp_path / "b.nwk"
    _util.write_phylip_lower(str(phy), names, D)
    r = run("-i", "d", "-I", str(phy), "-O", str(out), "--spr", "20")
    Dr = np.zeros_like(D)
    for i in range(n):
        for j in range(i):
            Dr[i, j] = Dr[j, i] = orc.phylip_value("%.9g" % D[i, j])
    g = capi.nj_variant_host(0, Dr)
    ref = capi.bme_spr_host(Dr, g["merge_x"], g["merge_y"], 20)
    assert out.read_text() == R.newick(names, ref["kids"], ref["top"], ref["len"])
    assert ref["long_moves"] >= 1 and spr_line(ref) in r.stderr


def test_help_text_names_the_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--spr arg" in r.stderr and "pruning and regrafting" in r.stderr


@pytest.mark.parametrize("extra,word", [
    (("--spr", "-1"), "whole number"), (("--spr", "x"), "whole number"), (("--spr", "3", "-m", "1"), "conventional NJ"),
    (("--spr", "3", "-m", "3"), "conventional NJ"), (("--spr", "3", "--add", "-t", "x.nwk"), "--add"), (("--spr", "3", "-o", "d"), "-o t"),
    (("--spr", "3", "-o", "j", "--add", "-t", "x.nwk"), "--add"), (("--spr", "3", "--bootstrap", "5"), "--bootstrap"),
    (("--spr", "3", "--gpus", "2"), "one GPU"), (("--spr", "3", "--devices", "0,0"), "one GPU"),
    (("--spr", "3", "--rank", "0", "--world", "2", "--rendezvous", "/r"), "one GPU"), (("--spr",), "missing"),
    (("--spr", "3", "--nni", "3"), "--nni"), (("--nni", "3", "--spr", "0"), "--nni"),
])
def test_usage_errors_before_any_gpu_call(tmp_path, extra, word):
    """decided from the arguments alone: the input file does not even exist"""
    r = subprocess.run([BIN, "-i", "m", "-I", str(tmp_path / "none.fa"), "-O", str(tmp_path / "o.nwk"), *extra], capture_output=True, text=True,
                       timeout=60)
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and word in head and "--spr" in head, r.stderr[:400]
    assert not (tmp_path / "o.nwk").exists()
