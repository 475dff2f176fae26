"""CPU tests of the site filter (--site-coverage / --complete-deletion): the NumPy reference the GPU tests compare with
(tests/_sites_ref.py) on hand-computed columns, the `dipper` usage errors that are decided before any input is read or a GPU
touched, and the two jplace metadata fields through the GPU-free writer (--dump-jplace)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _sites_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


# ---- the reference's own properties ---------------------------------------------------------------------------------------------
def test_reference_coverage_on_hand_computed_columns():
    seqs = [
        b"ACGTU-NacgtRY",
        b"ACGTUACGTACGT",
        b"-CGTUACG-ACG.",
        b"NCGTUAC--AC-?",
    ]
    cov = _sites_ref.coverage(seqs, "nt")
    #                              A  C  G  T  U  -  N  a  c  g  t  R  Y
    assert cov.tolist() == [2, 4, 4, 4, 4, 3, 3, 2, 1, 3, 3, 2, 1]
    assert cov.dtype == np.int64
    prot = [b"ARNDx*-v", b"arndX*-V", b"BZJUO.?w"]
    assert _sites_ref.coverage(prot, "aa").tolist() == [2, 2, 2, 2, 0, 0, 0, 3]
    with pytest.raises(ValueError):
        _sites_ref.coverage(seqs, "rna")


def test_reference_tie_is_kept_and_integer_compare():
    # n = 8, 500 per mille: cov 4 is exactly at the threshold (4000 >= 4000), cov 3 below it
    assert _sites_ref.keep([4, 3, 8, 0], 8, 500).tolist() == [True, False, True, False]
    # n = 3: two of three is 666.67 per mille -- 667 drops it (2000 < 2001), 666 keeps it (2000 >= 1998)
    assert _sites_ref.keep([2], 3, 667).tolist() == [False]
    assert _sites_ref.keep([2], 3, 666).tolist() == [True]
    # 1 per mille of up to 1000 sequences drops only the columns nobody holds (of 30 000 it asks for 30); 1000 needs everybody
    assert _sites_ref.keep([0, 1, 999, 1000], 1000, 1).tolist() == [False, True, True, True]
    assert _sites_ref.keep([0, 1, 29, 30, 30000], 30000, 1).tolist() == [False, False, False, True, True]
    assert _sites_ref.keep([0, 1, 29999, 30000], 30000, 1000).tolist() == [False, False, False, True]
    for bad in (0, 1001, -1):
        with pytest.raises(AssertionError):
            _sites_ref.keep([1], 2, bad)


def test_reference_complete_deletion_is_all_over_the_sequences():
    rng = np.random.default_rng(5)
    n, L = 23, 400
    a = rng.choice(np.frombuffer(b"ACGTU", dtype=np.uint8), size=(n, L))
    bad = rng.random((n, L)) < 0.03
    a[bad] = rng.choice(np.frombuffer(b"-Nacgu", dtype=np.uint8), size=int(bad.sum()))
    seqs = [r.tobytes() for r in a]
    h = _sites_ref.holds(seqs, "nt")
    k = _sites_ref.keep(_sites_ref.coverage(seqs, "nt"), n, 1000)
    assert np.array_equal(k, h.all(axis=0)) and 0 < k.sum() < L
    f = _sites_ref.filtered(seqs, k)
    assert len(f) == n and all(len(s) == int(k.sum()) for s in f)
    assert np.array_equal(np.frombuffer(b"".join(f), dtype=np.uint8).reshape(n, -1), a[:, k])
    assert _sites_ref.holds(f, "nt").all()
    # 1 per mille keeps exactly the columns somebody holds
    assert np.array_equal(_sites_ref.keep(_sites_ref.coverage(seqs, "nt"), n, 1), h.any(axis=0))


# ---- the command: usage errors before any input is read or a GPU touched --------------------------------------------------------
@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()
    p = tmp_path_factory.mktemp("sites") / "a.fa"
    p.write_text(">a\nACGTACGT\n>b\nACGTAC-T\n>c\nACGTTCGT\n>d\nAC-TACGA\n")
    return p


def run(*args, exe=BIN, env=None):
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env)


USAGE = [
    (["-i", "r", "--site-coverage", "0.5"], "need aligned sequences (-i m)"),
    (["-i", "d", "--site-coverage", "0.5"], "need aligned sequences (-i m)"),
    (["-i", "r", "--complete-deletion"], "need aligned sequences (-i m)"),
    (["-i", "d", "--complete-deletion"], "need aligned sequences (-i m)"),
    (["-i", "m", "--site-coverage", "1", "--complete-deletion"], "give one of the two"),
    (["-i", "m", "--site-coverage", "0"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "0.000"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "1.001"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "2"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "10"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "0.1234"], "at most three places"),
    (["-i", "m", "--site-coverage", "-0.5"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "0.5x"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "5e-1"], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "."], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", ""], "0 < x <= 1"),
    (["-i", "m", "--site-coverage", "0,5"], "0 < x <= 1"),
]


@pytest.mark.parametrize("args,needle", USAGE)
def test_site_filter_usage_errors(fasta, tmp_path, args, needle):
    out = tmp_path / "o.nwk"
    r = run(*args, "-I", str(fasta), "-O", str(out))
    assert r.returncode == 1 and "\033[31m" in r.stderr and needle in r.stderr, r.stderr[:400]
    assert not out.exists()


def test_usage_errors_come_before_the_input_is_read(tmp_path):
    """the input file does not exist: the usage error wins"""
    out = tmp_path / "o.nwk"
    r = run("-i", "m", "--site-coverage", "1.5", "-I", str(tmp_path / "missing.fa"), "-O", str(out))
    assert r.returncode == 1 and "--site-coverage: a decimal" in r.stderr and "cant open" not in r.stderr
    assert not out.exists()


def test_help_names_the_options():
    r = run("-h")
    assert r.returncode == 0
    for word in ("--site-coverage arg", "--complete-deletion", "backbone and queries together", "a column exactly at the threshold"):
        assert word in r.stderr, word


# ---- the host code under AddressSanitizer + UBSan (the command's own CPU build, as tests/test_cli.py runs it) -------------------
ROWS = "q1 1\n0 0 0.25 0.5\nq2 1\n2 0 0.125 0.0625\n"


def test_option_parsing_and_jplace_metadata_under_sanitizers(fasta, tmp_path):
    host = os.path.join(ROOT, "dipper_amd", "host")
    r = subprocess.run(["make", "-C", host, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asan = os.path.join(ROOT, "dipper_amd", "bin", "dipper_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")

    def arun(*args):
        q = run(*args, exe=asan, env=env)
        assert q.returncode != 66 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (args, q.stderr[-2000:])
        return q

    for args, needle in USAGE:
        q = arun(*args, "-I", str(fasta), "-O", str(tmp_path / "o.nwk"))
        assert q.returncode == 1 and needle in q.stderr, (args, q.stderr[:300])
    # the jplace writer: the two fields appear with the option, in canonical form, and only then
    tree = tmp_path / "b.nwk"
    tree.write_text("((A:0.1,B:0.2):0.05,C:0.3);\n")
    rows = tmp_path / "rows.txt"
    rows.write_text(ROWS)
    plain = arun("--dump-jplace", str(rows), "-t", str(tree))
    assert plain.returncode == 0, plain.stderr
    assert "site_coverage" not in plain.stdout and "sites_kept" not in plain.stdout
    for given, text in (("1", "1"), ("1.000", "1"), ("0.50", "0.5"), (".667", "0.667"), ("0.001", "0.001")):
        q = arun("--dump-jplace", str(rows), "-t", str(tree), "--site-coverage", given)
        assert q.returncode == 0, q.stderr
        doc = json.loads(q.stdout)
        assert doc["metadata"]["site_coverage"] == text and doc["metadata"]["sites_kept"] == 0
        base = json.loads(plain.stdout)
        assert {k: v for k, v in doc["metadata"].items() if k not in ("site_coverage", "sites_kept")} == base["metadata"]
        assert doc["placements"] == base["placements"] and doc["tree"] == base["tree"]
