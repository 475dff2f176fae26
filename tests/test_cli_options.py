"""What a `dipper` command line means, pinned as a recorded table (CPU, no GPU): tests/golden/cli_usage_matrix.tsv holds, for
every single option group below, every unordered pair of them and one case per branch of the value parsers, the exit status
and the text the command writes.  The input file of every case does not exist on purpose: a command line that passes
validation ends with the reader's missing-file error, before the device thread starts or ranks are forked -- so the table
says which rule wins when two are broken, and every message byte for byte, without touching a GPU.

The table is written by `python -m tests.test_cli_options record` from the binary that is built; it was recorded from the
command as it stood before its options moved into options.cpp and is not recorded again when that code changes."""
import itertools
import json
import os
import shlex
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_usage_matrix.tsv")
BANNER = "DIPPER Command Line Arguments"
TMP = "<TMP>"                  # placeholder of the case's directory in the table

# the option groups whose singles and unordered pairs are run (a pair that gives one flag two values: the later one wins)
GROUPS = [
    "--bionj", "--nni 1", "--spr 1", "--upgma", "--wpgma", "--fit",
    f"--fit-taxa {TMP}/fit.tsv", "--protein", "--site-coverage 0.5", "--complete-deletion",
    "-o j", "-o d", f"--add -t {TMP}/t.nwk",
    "--bootstrap 3", "--bootstrap-metric tbe", f"--bootstrap-taxa {TMP}/taxa.tsv",
    "-m 1", "-m 3", "-i r", "-i d", "-d 4",
    "--gpus 2", "--devices 0,0", "--rank 0 --world 2 --rendezvous x",
]
BASE = f"-i m -I {TMP}/missing.fa -O {TMP}/o.nwk"
# one case per branch of the value parsers; `!` in front: the whole command line, without the base
VALUES = [
    "--nni -1", "--nni x", "--nni 1234567890", "--spr -1", "--spr x", "--nni 0",
    "--bootstrap 0", "--bootstrap +3", "--bootstrap -", "--bootstrap 2000000000", "--bootstrap x",
    "--bootstrap 3 --bootstrap-seed -1", "--bootstrap 3 --bootstrap-seed 18446744073709551615", "--bootstrap 3 --bootstrap-seed 18446744073709551616",
    "--bootstrap-seed 1",
    "--bootstrap 3 --bootstrap-metric x", "--bootstrap 3 --bootstrap-metric fbp",
    f"--bootstrap 3 --bootstrap-taxa {TMP}/taxa.tsv --bootstrap-taxa-cutoff 1",
    f"--bootstrap 3 --bootstrap-taxa {TMP}/taxa.tsv --bootstrap-taxa-cutoff .25",
    f"--bootstrap 3 --bootstrap-taxa {TMP}/taxa.tsv --bootstrap-taxa-cutoff 0.1234",
    f"--bootstrap 3 --bootstrap-taxa {TMP}/taxa.tsv --bootstrap-taxa-cutoff .",
    "--bootstrap 3 --bootstrap-taxa-cutoff 0.3", "--bootstrap-taxa-cutoff 0.3",
    "--site-coverage 0", "--site-coverage 1.000", "--site-coverage .5", "--site-coverage 1.5",
    "--transport x", "--transport ipc", "--devices a", "--devices 3", "--gpus 0", "--world 2", "--world 2 --rank 2 --rendezvous x",
    "--world 2 --rank 0", "--rank 0",
    "-d abc", "--protein -d abc", "--protein -d 3", "--protein -d 5", "--protein -d 7", "--protein -d 9",
    f"--fit --fit-taxa {TMP}/o.nwk", "--fit --fit-taxa=", f"--bootstrap 3 --bootstrap-taxa {TMP}/o.nwk", "--bootstrap 3 --bootstrap-taxa=",
    "--add", f"--add -t {TMP}/missing.nwk", f"--add -t {TMP}/t.nwk -o j --bootstrap 3", f"--add -t {TMP}/t.nwk -o j -i r --bootstrap 3",
    "-i x", "-m 2 -p 0", "--seed x",
    # three rules broken: which one is named (the one-GPU rules come after everything the rank options say)
    "--fit --nni 1 --gpus 2", "--fit --upgma --devices 0,0", "--nni 1 --gpus 2 --transport x", "--upgma --gpus 2 --protein -i r",
    "--fit --gpus 2 --world 2", "--bionj --site-coverage 0.5 -i r -o d", "--fit --protein --bootstrap 3", "--wpgma --gpus 0 -m 1",
    f"--fit --fit-taxa {TMP}/o.nwk --bootstrap 3", "--spr 1 --devices 0,a",
    "--bogus", "-z", "stray", "--nni", "-O",
    "!-h", "!--help --bogus", f"!-I {TMP}/missing.fa -O {TMP}/o.nwk", f"!-i m -O {TMP}/o.nwk", f"!-i m -I {TMP}/missing.fa", "!",
]


def cases():
    out = [BASE + " " + g for g in GROUPS]
    out += [BASE + " " + a + " " + b for a, b in itertools.combinations(GROUPS, 2)]
    out += [v[1:] if v.startswith("!") else BASE + " " + v for v in VALUES]
    assert len(out) == len(set(out))
    return out


def run_case(case, binary=BIN, **kw):
    """(exit status, stderr, stdout) of one case in a fresh directory, the directory's path replaced by the placeholder.  stderr
    of a usage error (and of -h): the text in front of the help banner; of everything else: the whole text."""
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "t.nwk"), "w") as f:
            f.write("((A:0.1,B:0.2):0.05,C:0.3);\n")
        env = {k: v for k, v in os.environ.items() if k not in ("DPR_LOG", "DPR_CLI_NORMAL_EXIT")}
        r = subprocess.run([binary, *shlex.split(case.replace(TMP, tmp))], capture_output=True, text=True, cwd=tmp, timeout=120,
                           env=dict(env, **kw.pop("env", {})), **kw)
        left = sorted(os.listdir(tmp))
    err = r.stderr.replace(tmp, TMP)
    if BANNER in err:
        err = err.split(BANNER)[0]
    return r, (r.returncode, err, r.stdout.replace(tmp, TMP)), left


def read_table():
    table = {}
    with open(TABLE) as f:
        for ln in f:
            case, status, err, out = ln.rstrip("\n").split("\t")
            table[case] = (int(status), json.loads(err), json.loads(out))
    return table


def record(binary=BIN):
    with open(TABLE, "w") as f:
        for case in cases():
            _, (status, err, out), _ = run_case(case, binary)
            f.write("\t".join([case, str(status), json.dumps(err), json.dumps(out)]) + "\n")
    print(f"{len(cases())} cases written to {TABLE}")


# how a case may end without a device: a usage error, the help, or one of the messages in front of the first GPU call
ENDS = ("ERROR: cant open file: <TMP>/missing.fa\n", "Cannot open file: <TMP>/missing.fa\n", "ERROR: Unable to open input tree file: <TMP>/missing.nwk\n",
        "Adding new sequnces only supported with input aligned and unaligned sequences\n")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def test_the_table_lists_exactly_the_cases():
    assert list(read_table()) == cases()
    assert len(GROUPS) == 24 and len(cases()) >= 24 + 24 * 23 // 2 + 40


def test_every_case_ends_as_recorded_and_before_a_device():
    table = read_table()
    wrong = []
    for case in cases():
        r, got, left = run_case(case)
        if got != table[case]:
            wrong.append((case, got, table[case]))
        status, err, out = got
        # no case reaches a device, none creates -O or a report file
        assert left == ["t.nwk"], (case, left)
        if BANNER in r.stderr:
            assert out == "" and (status, err) == (0, "") or (status == 1 and err.startswith("\033[31m") and err.endswith("\033[0m\n")), (case, err)
        elif out:
            assert status == 1 and err == "" and out == "Invalid input-output combinations!!!!!\n", (case, out)
        else:
            assert status == 1 and err in ENDS, (case, status, err)
    assert not wrong, f"{len(wrong)} cases differ from the table; the first: {wrong[:3]}"


if __name__ == "__main__":
    if sys.argv[1:2] == ["record"] and len(sys.argv) <= 3:
        record(*sys.argv[2:])
    else:
        sys.exit("usage: python -m tests.test_cli_options record [BINARY]")
