"""The command line of -o n --nearest K without a GPU: every usage error ends with status 1 and its message before the help banner,
decided before any file is opened or a device touched (the input file does not exist and no output file appears); a valid line ends
with the reader's missing-file error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")

K_RANGE = "--nearest: the number of neighbours must be a whole number from 1 to 256"
TREE = " needs tree output (-o t)"
ONE_GPU = "-o n runs on one GPU"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


USAGE = [
    ("-o n", "-o n needs the number of neighbours (--nearest K)"),
    ("--nearest 5", "--nearest needs the neighbour output (-o n)"),
    ("-o d --nearest 5", "--nearest needs the neighbour output (-o n)"),
    ("-o p --within 0.1 --nearest 5", "--nearest needs the neighbour output (-o n)"),
    ("-o n --nearest 0", K_RANGE),
    ("-o n --nearest 257", K_RANGE),
    ("-o n --nearest -3", K_RANGE),
    ("-o n --nearest 2.5", K_RANGE),
    ("-o n --nearest ten", K_RANGE),
    ("-o n --nearest 1e1", K_RANGE),
    ("-o n --nearest=", K_RANGE),
    ("-o n --nearest 99999999999", K_RANGE),
    ("-o n --nearest 5 --add -t {tmp}/t.nwk", "-o n is not supported with --add or -t"),
    ("-o n --nearest 5 -t {tmp}/t.nwk", "-o n is not supported with --add or -t"),
    ("-o n --nearest 5 --bionj", "--bionj" + TREE),
    ("-o n --nearest 5 --nni 1", "--nni" + TREE),
    ("-o n --nearest 5 --spr 1", "--spr" + TREE),
    ("-o n --nearest 5 --upgma", "--upgma" + TREE),
    ("-o n --nearest 5 --wpgma", "--wpgma" + TREE),
    ("-o n --nearest 5 --fit", "--fit" + TREE),
    ("-o n --nearest 5 --bootstrap 3", "--bootstrap" + TREE),
    ("-o n --nearest 5 --bootstrap 3 --bootstrap-metric tbe", "--bootstrap" + TREE),
    ("-o n --nearest 5 --within 0.1", "--within needs the pair output (-o p)"),
    ("-o n --nearest 5 --clusters {tmp}/c.tsv", "--clusters needs the pair output (-o p)"),
    ("-o n --nearest 5 --gpus 2", ONE_GPU),
    ("-o n --nearest 5 --devices 0,0", ONE_GPU),
    ("-o n --nearest 5 --rank 0 --world 2 --rendezvous x", ONE_GPU),
]


@pytest.mark.parametrize("args,message", USAGE, ids=[a for a, _ in USAGE])
def test_usage_errors_are_decided_before_any_file_or_gpu(tmp_path, args, message):
    (tmp_path / "t.nwk").write_text("((A:0.1,B:0.2):0.05,C:0.3);\n")
    r = run("-i", "m", "-I", str(tmp_path / "missing.fa"), "-O", str(tmp_path / "o.tsv"), *args.replace("{tmp}", str(tmp_path)).split())
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and "DIPPER Command Line Arguments" in r.stderr and message in head, (r.returncode, head)
    assert head.startswith("\033[31m") and head.count("\n") == 1      # one message, in red
    assert sorted(os.listdir(tmp_path)) == ["t.nwk"]


@pytest.mark.parametrize("args", ["-o n --nearest 5", "-o n --nearest 1", "-o n --nearest 256", "-o n --nearest 5 -i r -k 12 -s 500", "-o n --nearest 5 -i d",
                                  "-o n --nearest 5 --protein -d 8", "-o n --nearest 5 -d 9", "-o n --nearest 5 --site-coverage 0.9",
                                  "-o n --nearest 5 --complete-deletion", "-o n --nearest 5 --devices 0", "-o n --nearest 007"])
def test_valid_combinations_reach_the_reader(tmp_path, args):
    r = run("-i", "m", "-I", str(tmp_path / "missing.fa"), "-O", str(tmp_path / "o.tsv"), *args.split())
    assert r.returncode == 1 and "DIPPER Command Line Arguments" not in r.stderr and "missing.fa" in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_help_names_the_options():
    r = run("-h")
    assert r.returncode == 0
    for word in ("n - the nearest neighbours of every sequence", "--nearest arg", "ID<TAB>Rank<TAB>Neighbour<TAB>Distance"):
        assert word in r.stderr, word
