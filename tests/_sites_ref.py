"""NumPy restatement of the site filter (include/dipper_hip.h, dpr_msa_filter_sites): which sequences hold a symbol at a column,
the coverage of every column, the kept columns for a per mille threshold and the filtered alignment.  Sequences are byte strings
of one length.  Alphabets: "nt" -- A, C, G, T, U as dpr_pack4 codes them (upper case only: a lower-case letter is not a base
there); "aa" -- the 20 letters ARNDCQEGHILKMFPSTWYV in either case, as dpr_pack_aa codes them."""
import numpy as np

NT = b"ACGTU"
AA = b"ARNDCQEGHILKMFPSTWYV"


def _symbol_table(alphabet):
    t = np.zeros(256, dtype=bool)
    if alphabet == "nt":
        t[list(NT)] = True
    elif alphabet == "aa":
        t[list(AA)] = True
        t[list(AA.lower())] = True
    else:
        raise ValueError(alphabet)
    return t


def holds(seqs, alphabet):
    """bool [n][L]: sequence s holds a symbol at column c"""
    L = len(seqs[0])
    assert all(len(s) == L for s in seqs)
    a = np.frombuffer(b"".join(bytes(s) for s in seqs), dtype=np.uint8).reshape(len(seqs), L)
    return _symbol_table(alphabet)[a]


def coverage(seqs, alphabet):
    """int64 [L]: the sequences that hold a symbol at every column"""
    return holds(seqs, alphabet).sum(axis=0, dtype=np.int64)


def keep(cov, n, permille):
    """bool [L]: 1000 cov >= permille n in integers (Python ints below: no overflow, no rounding), so a tie is kept"""
    assert 1 <= permille <= 1000
    return np.array([1000 * int(c) >= permille * int(n) for c in cov], dtype=bool)


def filtered(seqs, keep):
    """the alignment of the kept columns, ascending"""
    k = np.asarray(keep, dtype=bool)
    return [np.frombuffer(bytes(s), dtype=np.uint8)[k].tobytes() for s in seqs]
