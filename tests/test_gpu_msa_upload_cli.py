"""`dipper -i m -m 2` with the alignment uploaded by the device thread (as soon as the context exists, before the graph warm-up):
the Newick of a 200-tip FASTA is byte for byte what the command wrote before the upload moved there
(tests/golden/msa_upload_cli/: the input and that output)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GOLDEN = os.path.join(ROOT, "tests", "golden", "msa_upload_cli")


def test_newick_unchanged(tmp_path):
    out = tmp_path / "out.nwk"
    r = subprocess.run([BIN, "-i", "m", "-I", os.path.join(GOLDEN, "in200.fa"), "-O", str(out), "-m", "2", "-d", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLDEN, "out200.nwk"), "rb") as f:
        want = f.read()
    assert out.read_bytes() == want
