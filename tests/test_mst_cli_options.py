"""The command line of -o s [--dendrogram FILE] without a GPU: every usage error ends with status 1 and its message before the help
banner, decided before any file is opened or a device touched (the input file does not exist and no output file appears); a valid line
ends with the reader's missing-file error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")

NEEDS = "--dendrogram needs the spanning-tree output (-o s)"
TREE = " needs tree output (-o t)"
ONE_GPU = "-o s runs on one GPU"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


USAGE = [
    ("--dendrogram {tmp}/d.nwk", NEEDS),
    ("-o t --dendrogram {tmp}/d.nwk", NEEDS),
    ("-o d --dendrogram {tmp}/d.nwk", NEEDS),
    ("-o p --within 0.1 --dendrogram {tmp}/d.nwk", NEEDS),
    ("-o n --nearest 5 --dendrogram {tmp}/d.nwk", NEEDS),
    ("-o s --dendrogram=", "--dendrogram: a file name"),
    ("-o s --dendrogram {tmp}/o.tsv", "--dendrogram: the file must differ from the output file (-O)"),
    ("-o s --add -t {tmp}/t.nwk", "-o s is not supported with --add or -t"),
    ("-o s -t {tmp}/t.nwk", "-o s is not supported with --add or -t"),
    ("-o s --bionj", "--bionj" + TREE),
    ("-o s --nni 1", "--nni" + TREE),
    ("-o s --spr 1", "--spr" + TREE),
    ("-o s --upgma", "--upgma" + TREE),
    ("-o s --wpgma", "--wpgma" + TREE),
    ("-o s --fit", "--fit" + TREE),
    ("-o s --bootstrap 3", "--bootstrap" + TREE),
    ("-o s --within 0.1", "--within needs the pair output (-o p)"),
    ("-o s --clusters {tmp}/c.tsv", "--clusters needs the pair output (-o p)"),
    ("-o s --nearest 5", "--nearest needs the neighbour output (-o n)"),
    ("-o s --gpus 2", ONE_GPU),
    ("-o s --devices 0,0", ONE_GPU),
    ("-o s --rank 0 --world 2 --rendezvous x", ONE_GPU),
    ("-o s --dendrogram {tmp}/d.nwk --gpus 2", ONE_GPU),
]


@pytest.mark.parametrize("args,message", USAGE, ids=[a for a, _ in USAGE])
def test_usage_errors_are_decided_before_any_file_or_gpu(tmp_path, args, message):
    (tmp_path / "t.nwk").write_text("((A:0.1,B:0.2):0.05,C:0.3);\n")
    r = run("-i", "m", "-I", str(tmp_path / "missing.fa"), "-O", str(tmp_path / "o.tsv"), *args.replace("{tmp}", str(tmp_path)).split())
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and "DIPPER Command Line Arguments" in r.stderr and message in head, (r.returncode, head)
    assert head.startswith("\033[31m") and head.count("\n") == 1      # one message, in red
    assert sorted(os.listdir(tmp_path)) == ["t.nwk"]


@pytest.mark.parametrize("args", ["-o s", "-o s --dendrogram {tmp}/d.nwk", "-o s -i r -k 12 -s 500", "-o s -i d", "-o s --protein -d 8", "-o s -d 9",
                                  "-o s --site-coverage 0.9", "-o s --complete-deletion", "-o s --devices 0", "-o s -i d --dendrogram {tmp}/d.nwk"])
def test_valid_combinations_reach_the_reader(tmp_path, args):
    r = run("-i", "m", "-I", str(tmp_path / "missing.fa"), "-O", str(tmp_path / "o.tsv"), *args.replace("{tmp}", str(tmp_path)).split())
    assert r.returncode == 1 and "DIPPER Command Line Arguments" not in r.stderr and "missing.fa" in r.stderr, r.stderr
    assert "Invalid input-output combinations" not in r.stdout and os.listdir(tmp_path) == []


def test_help_names_the_options():
    r = run("-h")
    assert r.returncode == 0
    for word in ("s - the minimum spanning tree of the distances", "--dendrogram arg", "ID1<TAB>ID2<TAB>Distance", "line `MST:` on stderr"):
        assert word in r.stderr, word
