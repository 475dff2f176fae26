"""CPU: the reference of the pair-table distance types 9-11 (tests/_pairtable_ref.py) on hand-built pairs and on JC-evolved
data, and the command line's treatment of `-d 9|10|11` where no GPU is needed.

LogDet of two identical sequences is -1/4 sum_i ln f_i - ln 4 for base frequencies f_i: 0 for a uniform composition only (a known
property of the uncorrected LogDet), so "identical sequences give 0" is asserted for types 9 and 11 at any composition with all
four bases, and for type 10 at the uniform one; at a skewed composition type 10 is asserted against that closed form."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import _msa_ref, _pairtable_ref as R, _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def _F(a, b):
    return R.table(_msa_ref.codes(a), _msa_ref.codes(b))


def test_table_orientation_and_exact_determinant():
    F = _F(b"AACGTTGA-N", b"ACCGTAGANT")
    assert F[0][0] == 2 and F[0][1] == 1 and F[3][0] == 1 and F[3][3] == 1 and sum(map(sum, F)) == 8     # [row base][column base]
    rng = np.random.default_rng(1)
    for _ in range(50):
        M = rng.integers(0, 2 ** 30, size=(4, 4))
        F = [[int(v) for v in row] for row in M]
        Ft = [[F[j][i] for j in range(4)] for i in range(4)]
        assert R.det4(F) == R.det4(Ft)
        small = rng.integers(0, 50, size=(4, 4))
        assert R.det4([[int(v) for v in row] for row in small]) == round(np.linalg.det(small.astype(np.float64)))


@pytest.mark.parametrize("seq", [b"ACGTACGTACGTACGT", b"AAAAAAAACCGGTTTT", b"ACGTTTTTTTTTTGGG"])
def test_identical_sequences(seq):
    assert len(seq) == 16
    F = _F(seq, seq)
    assert R.distance(F, 9) == (R.REGULAR, 0.0)
    assert R.distance(F, 11) == (R.REGULAR, 0.0)
    f = [F[i][i] / 16 for i in range(4)]
    k, v = R.distance(F, 10)
    assert k == R.REGULAR
    if seq == b"ACGTACGTACGTACGT":
        assert v == 0.0
    else:
        assert v > 0 and abs(v - (-0.25 * sum(math.log(x) for x in f) - math.log(4.0))) < 1e-14


def test_stated_specials():
    # A <-> C only: every site a transversion between the same two bases; G and T absent from the row or column side
    a, b = b"AAAAAAAACCCCCCCC", b"CCCCCCCCAAAAAAAA"
    F = _F(a, b)
    assert R.det4(F) == 0
    k, v = R.distance(F, 9)
    assert k == R.SPECIAL and math.isnan(v)                       # a_A a_G = 0
    assert R.distance(F, 10) == (R.SPECIAL, math.inf)             # det 0, N > 0
    k, v = R.distance(F, 11)
    assert k == R.SPECIAL and math.isnan(v)                       # det 0 and a marginal 0
    # a base missing from one side only: the row has no T, every base has a positive pooled frequency
    a, b = b"ACGAACGAACGAACGA", b"ACGTACGTACGTACGT"
    F = _F(a, b)
    N, r, c = R.margins(F)
    assert N == 16 and r[3] == 0 and c[3] == 4 and R.det4(F) == 0
    k, v = R.distance(F, 9)
    assert k == R.REGULAR and v > 0
    assert R.distance(F, 10) == (R.SPECIAL, math.inf)
    k, v = R.distance(F, 11)
    assert k == R.SPECIAL and math.isnan(v)
    # a negative determinant: the row's A and C swapped in the column
    F = _F(b"AAAACCCCGGGGTTTT", b"CCCCAAAAGGGGTTTT")
    assert R.det4(F) < 0
    assert math.isnan(R.distance(F, 10)[1]) and math.isnan(R.distance(F, 11)[1])
    assert R.distance(F, 9) == (R.SPECIAL, None)                  # a log argument <= 0
    # no common site
    F = _F(b"ACGT----", b"----ACGT")
    assert all(R.distance(F, t)[0] == R.SPECIAL and math.isnan(R.distance(F, t)[1]) for t in R.TYPES)
    # a singular table with all marginals positive: +inf for both determinant types
    F = _F(b"ACGTACGTACGTACGT", b"ACACACACGTGTGTGT")
    assert R.det4(F) == 0 and all(x > 0 for x in R.margins(F)[1] + R.margins(F)[2])
    assert R.distance(F, 10) == (R.SPECIAL, math.inf) and R.distance(F, 11) == (R.SPECIAL, math.inf)


def test_close_to_jc_on_jc_evolved_data():
    rng = np.random.default_rng(3)
    seqs = _util.synth_alignment(rng, 6, 20000, mean_bl=5e-2, lo=1e-2, hi=1e-1)
    cs = [_msa_ref.codes(s) for s in seqs]
    for r in range(1, 6):
        for c in range(r):
            cnt = _msa_ref.Counts(cs[r], cs[c])
            k, jc = _msa_ref.distance(cnt, 2)
            assert k == _msa_ref.REGULAR
            for t in R.TYPES:
                k, v = R.distance(R.table(cs[r], cs[c]), t)
                assert k == R.REGULAR and abs(v - jc) < 1e-3, (r, c, t, v, jc)


def test_value_does_not_depend_on_the_orientation():
    seqs = R.msa_drift(L=600, n=8)
    cs = [_msa_ref.codes(s) for s in seqs]
    F = R.table(cs[7], cs[0])
    Ft = R.table(cs[0], cs[7])
    assert Ft == [[F[j][i] for j in range(4)] for i in range(4)] and F != Ft
    for t in R.TYPES:
        assert R.distance(F, t) == R.distance(Ft, t)


# ---- the command, no GPU needed ---------------------------------------------------------------------------------------------
def _run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("dt", ["9", "10", "11"])
def test_protein_refuses_the_nucleotide_pair_table_types(tmp_path, dt):
    fa = tmp_path / "p.fa"
    fa.write_text(">a\nARND\n>b\nARNE\n>c\nAKND\n")
    r = _run("-i", "m", "--protein", "-I", str(fa), "-O", str(tmp_path / "o.nwk"), "-d", dt)
    assert r.returncode == 1 and "--protein takes -d 1, 2, 7 or 8" in r.stderr


def test_help_lists_the_pair_table_types():
    r = _run("--help")
    text = r.stdout + r.stderr
    assert "9 - TN93" in text and "10 - LogDet" in text and "11 - paralinear" in text
