"""`dipper` in the default mode at 30 000 sequences: the input selects placement, which is known only once the input is read.
Every option that builds its tree where conventional NJ does ends the run there with its own line and leaves no tree
(test_gpu_upgma_cli.py pins `--wpgma` loosely; here every such option, its whole line)."""
import os
import subprocess

import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
N = 30000
TAIL = f": {N} sequences select placement in the default mode; use -m 2\n"
LINES = {
    "--bionj": "ERROR: --bionj needs conventional NJ" + TAIL,
    "--nni 1": "ERROR: --nni needs conventional NJ" + TAIL,
    "--spr 1": "ERROR: --spr needs conventional NJ" + TAIL,
    "--upgma": "ERROR: --upgma builds the tree where conventional NJ does" + TAIL,
    "--wpgma": "ERROR: --wpgma builds the tree where conventional NJ does" + TAIL,
    "--fit": "ERROR: --fit needs conventional NJ" + TAIL,
    "--bootstrap 2": "ERROR: --bootstrap needs conventional NJ" + TAIL,
}


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    rng = np.random.default_rng(1)
    seqs = [bytes(row) for row in np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (N, 24))]]
    fa = tmp_path_factory.mktemp("modecheck") / "many.fa"
    _util.write_fasta(str(fa), [f"T{i}" for i in range(N)], seqs)
    return fa


@pytest.mark.parametrize("option", list(LINES))
def test_default_mode_at_30000_sequences_ends_with_the_options_line(tmp_path, many, option):
    out = tmp_path / "o.nwk"
    r = subprocess.run([BIN, "-i", "m", "-I", str(many), "-O", str(out), *option.split()], capture_output=True, text=True, timeout=300)
    print(option, r.returncode, repr(r.stderr[-600:]))
    assert r.returncode != 0 and r.stdout == "", (r.returncode, r.stderr[-600:])
    assert LINES[option] in r.stderr.splitlines(keepends=True), r.stderr[-600:]
    assert "ERROR: " not in r.stderr.replace(LINES[option], "", 1)      # (the one rule, named once)
    assert not out.exists()
