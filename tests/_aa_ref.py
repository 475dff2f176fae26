"""NumPy reference of the protein distances (include/dipper_hip.h, dpr_set_msa_aa): the alphabet table, integer useful / match
over all pairs by pairwise deletion, and the four formulas in float64 in the operation order the header states.  Builders of
seeded protein alignments for the tests live here too."""
import numpy as np

LETTERS = b"ARNDCQEGHILKMFPSTWYV"
NOT_A_RESIDUE = 255


def table():
    """byte -> code: the 20 letters in either case 0..19, everything else 255"""
    t = np.full(256, NOT_A_RESIDUE, dtype=np.uint8)
    for i, ch in enumerate(LETTERS):
        t[ch] = i
        t[ch + 32] = i
    return t


def encode(seqs):
    """[n][L] codes, L = len(seqs[0]); shorter sequences end in not-a-residue"""
    t = table()
    L = len(seqs[0])
    out = np.full((len(seqs), L), NOT_A_RESIDUE, dtype=np.uint8)
    for i, s in enumerate(seqs):
        c = t[np.frombuffer(s, dtype=np.uint8)]
        out[i, : min(L, len(c))] = c[:L]
    return out


def counts(codes):
    """(useful, match), int64 [n][n]: sites where both are residues / where the residues are equal"""
    codes = np.asarray(codes, dtype=np.uint8)
    n = codes.shape[0]
    valid = codes < 20
    useful = np.zeros((n, n), dtype=np.int64)
    match = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        both = valid & valid[i]
        useful[i] = both.sum(axis=1)
        match[i] = (both & (codes == codes[i])).sum(axis=1)
    return useful, match


def dist(useful, match, dist_type):
    """float64 distances of integer counts (any shape); 1 p, 2 JC with 20 states, 7 Poisson, 8 Kimura"""
    with np.errstate(all="ignore"):
        p = 1 - np.asarray(match, dtype=np.float64) / np.asarray(useful, dtype=np.float64)
        if dist_type == 1:
            return p
        if dist_type == 2:
            return -0.95 * np.log(1.0 - p / 0.95)
        if dist_type == 7:
            return -np.log(1.0 - p)
        if dist_type == 8:
            return -np.log(1.0 - p - 0.2 * p * p)
    raise ValueError(dist_type)


def matrix(useful, match, dist_type):
    """the n x n matrix: dist() with a zero diagonal"""
    D = dist(useful, match, dist_type)
    np.fill_diagonal(D, 0.0)
    return D


# ---- seeded alignments ------------------------------------------------------------------------------------------------------
RES = np.frombuffer(LETTERS, dtype=np.uint8)


def related(rng, n, L, lo=0.01, hi=0.3, alphabet=20):
    """n x L residue codes: one root, every sequence with its own share (lo..hi) of sites redrawn among `alphabet` codes"""
    root = rng.integers(0, alphabet, size=L, dtype=np.uint8)
    out = np.empty((n, L), dtype=np.uint8)
    for i in range(n):
        s = root.copy()
        hit = rng.random(L) < rng.uniform(lo, hi)
        s[hit] = rng.integers(0, alphabet, size=int(hit.sum()), dtype=np.uint8)
        out[i] = s
    return out


def to_bytes(codes):
    """list of byte strings (upper-case letters) of residue codes 0..19"""
    return [bytearray(RES[c].tobytes()) for c in codes]


def scatter(rng, seqs, rate, chars=b"-", runs=False):
    """non-residue bytes over every sequence at `rate`; runs: as runs of 5..40 sites"""
    chars = np.frombuffer(chars, dtype=np.uint8)
    for s in seqs:
        L = len(s)
        a = np.frombuffer(bytes(s), dtype=np.uint8).copy()
        if runs:
            k = max(1, int(rate * L / 20))
            for p0 in rng.integers(0, L, size=k):
                a[p0:p0 + int(rng.integers(5, 41))] = chars[0]
        else:
            m = rng.random(L) < rate
            a[m] = rng.choice(chars, size=int(m.sum()))
        s[:] = a.tobytes()
    return seqs


def evolve_yule(rng, n, L, mean_bl=0.03, lo=0.003, hi=0.15):
    """residues evolved down a Yule tree (tests/_util.yule_tree), every substitution a uniform draw among the 19 others"""
    from tests import _util
    parent, children, leaves = _util.yule_tree(rng, n)
    seq = {0: rng.integers(0, 20, size=L, dtype=np.uint8)}
    pending = [0]
    while pending:
        node = pending.pop()
        for c in children[node]:
            t = seq[node].copy()
            k = rng.poisson(L * float(np.clip(rng.exponential(mean_bl), lo, hi)))
            if k:
                pos = rng.integers(0, L, size=k)
                t[pos] = (t[pos] + rng.integers(1, 20, size=k, dtype=np.uint8)) % 20
            seq[c] = t
            pending.append(c)
    return [bytes(RES[seq[leaf]].tobytes()) for leaf in leaves]
