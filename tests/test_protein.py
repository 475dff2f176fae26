"""CPU tests of protein input: the host encoder dpr_pack_aa, the NumPy reference the GPU tests compare with (tests/_aa_ref.py)
on hand-computed pairs, and the `dipper --protein` usage errors that are decided before any GPU call."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import _aa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def test_pack_aa_table_all_bytes():
    from dipper_amd import capi
    want = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate("ARNDCQEGHILKMFPSTWYV"):
        want[ord(ch)] = i
        want[ord(ch.lower())] = i
    assert np.array_equal(_aa_ref.table(), want)
    got = capi.pack_aa(bytes(range(256)))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for ch in b"-.?*XBZJUOxbzjuo0123456789 \n\0":
        assert got[ch] == 255


@pytest.mark.parametrize("L", [0, 1, 31, 32, 33, 1000])
def test_pack_aa_lengths(L):
    from dipper_amd import capi
    rng = np.random.default_rng(L)
    s = rng.integers(0, 256, size=L, dtype=np.uint8).tobytes()
    got = capi.pack_aa(s)
    assert len(got) == L and np.array_equal(got, _aa_ref.table()[np.frombuffer(s, dtype=np.uint8)])


def test_pack_aa_many_pads_and_cuts():
    from dipper_amd import capi
    got = capi.pack_aa_many([b"ARND", b"ar", b"VVVVVV"])
    assert np.array_equal(got, [[0, 1, 2, 3], [0, 1, 255, 255], [19, 19, 19, 19]])
    assert np.array_equal(got, _aa_ref.encode([b"ARND", b"ar", b"VVVVVV"]))
    assert (capi.DIST_POISSON, capi.DIST_KIMURA) == (7, 8)


def test_reference_on_hand_computed_pairs():
    seqs = [
        b"ARNDCQEGHI",      # 0
        b"ARNDCQEGVV",      # 1: (10, 8) against 0
        b"-----QEGHI",      # 2: (5, 5) against 0: match = useful
        b"RNDCQEGHIL",      # 3: (10, 0) against 0: match = 0
        b"XBZ*-.?JUO",      # 4: no residue at all: useful = 0 against everybody
        b"arndcqeghi",      # 5: lower case = sequence 0
    ]
    useful, match = _aa_ref.counts(_aa_ref.encode(seqs))
    assert np.array_equal(useful, useful.T) and np.array_equal(match, match.T)
    assert (useful[1, 0], match[1, 0]) == (10, 8)
    assert (useful[2, 0], match[2, 0]) == (5, 5)
    assert (useful[3, 0], match[3, 0]) == (10, 0)
    assert np.all(useful[4] == 0) and np.all(match[4] == 0)
    assert (useful[5, 0], match[5, 0]) == (10, 10)
    assert (useful[2, 1], match[2, 1]) == (5, 3)
    d = {t: _aa_ref.dist(useful, match, t) for t in (1, 2, 7, 8)}
    p = 1 - 8.0 / 10
    assert d[1][1, 0] == p
    assert d[2][1, 0] == -0.95 * math.log(1.0 - p / 0.95)
    assert d[7][1, 0] == -math.log(1.0 - p) and abs(d[7][1, 0] + math.log(0.8)) < 1e-15
    assert d[8][1, 0] == -math.log(1.0 - p - 0.2 * p * p)
    for t in (1, 2, 7, 8):
        assert d[t][2, 0] == 0.0 and d[t][5, 0] == 0.0                 # match = useful
        assert np.all(np.isnan(d[t][4])) and np.all(np.isnan(d[t][:, 4]))      # useful = 0
        assert np.all(np.diag(_aa_ref.matrix(useful, match, t)) == 0)
    assert d[1][3, 0] == 1.0 and d[7][3, 0] == np.inf and np.isnan(d[2][3, 0]) and np.isnan(d[8][3, 0])     # match = 0


# ---- the command: usage errors before any GPU call -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()
    p = tmp_path_factory.mktemp("prot") / "p.fa"
    p.write_text(">a\nARNDCQEG\n>b\nARNDCQEV\n>c\nARNDCQVV\n>d\nARNDVVVV\n")
    return p


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True)


@pytest.mark.parametrize("args,needle", [
    (["-i", "r", "--protein"], "--protein needs aligned sequences"),
    (["-i", "d", "--protein"], "--protein needs aligned sequences"),
    (["-i", "m", "--protein", "-d", "3"], "nucleotide models"),
    (["-i", "m", "--protein", "-d", "4"], "nucleotide models"),
    (["-i", "m", "--protein", "-d", "5"], "nucleotide models"),
    (["-i", "m", "--protein", "-d", "6"], "nucleotide models"),
    (["-i", "m", "--protein", "-d", "9"], "-d 1, 2, 7 or 8"),
    (["-i", "m", "--protein", "--bootstrap", "10"], "--bootstrap is not available with --protein"),
    (["-i", "m", "--protein", "-m", "3"], "-m 1 or -m 2"),
])
def test_protein_usage_errors(fasta, tmp_path, args, needle):
    out = tmp_path / "o.nwk"
    r = run(*args, "-I", str(fasta), "-O", str(out))
    assert r.returncode == 1 and "\033[31m" in r.stderr and needle in r.stderr, r.stderr[:400]
    assert not out.exists()


def test_help_names_the_switch_and_the_types():
    r = run("-h")
    assert r.returncode == 0
    for word in ("--protein", "7 - Poisson", "8 - Kimura"):
        assert word in r.stderr
