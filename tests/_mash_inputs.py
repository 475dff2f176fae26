"""Inputs that sit on the edges of the Mash inverted-index kernel (dipper_amd/csrc/mash_index.hip), and the conditions that say so.

The kernel cuts the column tips into chunks of C tips.  Per chunk every distinct sketch value has a posting list whose length
is the number of copies of the value in the chunk's sketches (further copies inside one sketch are entries too: they carry the
"never" payload).  A list of at least Dm entries is DENSE (positions by tip, packed 16-bit arithmetic, two tips per lane), a
shorter one is SPARSE (64 entries preloaded, then whole groups of 192, then up to three groups of 64, the last one partial).  A row
walks its distinct values 64 sketch positions at a time and applies those present in the chunk two per step; two dense values of
one step are applied in one fused update.

Everything here works on sketches -- the oracle's or the device's -- and takes C and Dm as arguments: the tests read them from
Dipper.mash_index_info(), the CPU test of this module uses the values of the kernel as it stands."""
from concurrent.futures import ThreadPoolExecutor
import os

import numpy as np

from tests import _util

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)      # the value short reads are padded with (orc_sketch)
MARKER, SPACER = 30, 3
CLASSES = ("dense,dense", "dense,sparse", "sparse,dense", "sparse,sparse", "single")


def _threads():
    return max(1, min(16, os.cpu_count() or 1))


def list_length_edges(C, Dm):
    """E: posting-list lengths around every group boundary of the sparse path, the dense threshold and a whole chunk"""
    return sorted(set([1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, Dm - 1, Dm, Dm + 1, 600, C]))


def marker_reads(rng, sizes, k, T):
    """Reads whose k-mers are held by chosen numbers of tips.  `sizes`: tips per chunk; marker j (30 random bases: 31 - k k-mers
    that nothing else holds) is given to exactly min(T[j], tips of the chunk) reads of each chunk.  A read is a random body of
    40-80 bases, then marker + a 3-base random spacer for every marker it holds."""
    assert 2 <= k <= MARKER
    markers = [rng.integers(0, 4, size=MARKER, dtype=np.uint8) for _ in T]
    reads = []
    for tips in sizes:
        holds = np.zeros((tips, len(T)), dtype=bool)
        for j, t in enumerate(T):
            holds[rng.choice(tips, size=min(int(t), tips), replace=False), j] = True
        for r in range(tips):
            parts = [rng.integers(0, 4, size=int(rng.integers(40, 81)), dtype=np.uint8)]
            for j in np.flatnonzero(holds[r]):
                parts += [markers[j], rng.integers(0, 4, size=SPACER, dtype=np.uint8)]
            reads.append(_util.BASES[np.concatenate(parts)].tobytes())
    return reads


def clonal_4096(rng):
    """1 030 tips for sketches of 4 096 (k = 15): 630 clonal reads of ~6 000 bases (full sketches, nearly every value dense in
    chunk 0, position 4 095 in use) and 400 prefixes of read 7 with 1 986 .. 3 183 k-mers (913 .. 2 110 copies of the padding
    value behind values they share with the clone)"""
    reads = _util.synth_reads(rng, 1030, 6000, mean_bl=3e-4, lo=3e-5, hi=3e-3)[:630]
    return reads + [reads[7][:2000 + 3 * i] for i in range(400)]


def oracle_sketches(orc, reads, k, S):
    out = np.zeros((len(reads), S), dtype=np.uint64)

    def some(r0):
        for r in range(r0, min(r0 + 32, len(reads))):
            out[r] = orc.sketch(orc.pack2(reads[r]), len(reads[r]), k=k, S=S)
    with ThreadPoolExecutor(_threads()) as ex:
        list(ex.map(some, range(0, len(reads), 32)))
    return out


def oracle_rows(orc, sk, k, rows):
    """{i: distances of tip i to tips 0 .. i - 1 by the oracle's literal merge} on a pool of at most 16 threads (ctypes releases
    the GIL during the call; every row is the oracle's own loop)"""
    sk = np.ascontiguousarray(sk, dtype=np.uint64)
    rows = [int(i) for i in rows]
    with ThreadPoolExecutor(_threads()) as ex:
        return dict(zip(rows, ex.map(lambda i: orc.mash_dist_row(sk, k, i, i), rows)))


def assert_rows(M, ref):
    """the suite's rule for Mash distances: integer intersection counts, so rtol = 1e-12 tells every count >= 1 apart"""
    for i, want in ref.items():
        ok = np.isclose(M[i, :i], want, rtol=1e-12, atol=0)
        assert ok.all(), (i, np.flatnonzero(~ok)[:5], M[i, :i][~ok][:5], want[~ok][:5])


def chunk_tables(sk, C):
    """per chunk of C tips: (distinct values ascending, entries of each value's posting list)"""
    sk = np.asarray(sk, dtype=np.uint64)
    return [np.unique(sk[c0:c0 + C].ravel(), return_counts=True) for c0 in range(0, sk.shape[0], C)]


def index_counts(tables, Dm):
    """(distinct (chunk, value) pairs, those with at least Dm entries) -- what the index build reports"""
    return sum(len(u) for u, _ in tables), sum(int((cnt >= Dm).sum()) for _, cnt in tables)


def padding_copies(sk):
    return (np.asarray(sk, dtype=np.uint64) == PAD).sum(axis=1)


def marker_conditions(sk, C, Dm):
    """2(a): in every full chunk each list length of E is taken by at least one value, and every tip carries between 1 and
    S - 1 copies of the padding value.  Returns {chunk: {t: values with exactly t entries}} of the full chunks."""
    sk = np.asarray(sk, dtype=np.uint64)
    S = sk.shape[1]
    full = {}
    for c, (uniq, cnt) in enumerate(chunk_tables(sk, C)):
        if (c + 1) * C > sk.shape[0]:
            continue
        real = cnt[uniq != PAD]
        full[c] = {t: int((real == t).sum()) for t in list_length_edges(C, Dm)}
        missing = [t for t, v in full[c].items() if v == 0]
        assert not missing, f"chunk {c}: no value with exactly {missing} entries"
        pad = padding_copies(sk[c * C:(c + 1) * C])
        assert pad.min() >= 1 and pad.max() <= S - 1, (c, int(pad.min()), int(pad.max()))
    assert full, "no full chunk"
    return full


def clonal_conditions(sk, C, Dm):
    """2(b), all in chunk 0: >= 1 000 dense values, a dense value whose first copy sits at the last position of the largest
    sketch some tip can have (S - 1), >= 300 tips with padding and more than 2 000 copies of it in one tip.  Returns the figures."""
    sk = np.asarray(sk, dtype=np.uint64)
    S = sk.shape[1]
    uniq, cnt = chunk_tables(sk[:C], C)[0]
    dense = uniq[cnt >= Dm]
    assert len(dense) >= 1000, len(dense)
    last_first = sk[:C, S - 1][sk[:C, S - 1] != sk[:C, S - 2]]          # values whose FIRST position is S - 1
    at_end = np.intersect1d(last_first[last_first != PAD], dense)
    assert len(at_end) >= 1, "no dense value whose first position is S - 1"
    pad = padding_copies(sk[:C])
    assert (pad > 0).sum() >= 300 and pad.max() > 2000, (int((pad > 0).sum()), int(pad.max()))
    assert PAD in dense
    return dict(dense=len(dense), at_end=len(at_end), padded_tips=int((pad > 0).sum()), most_copies=int(pad.max()))


def pair_classes(sk, tables, C, Dm, rows):
    """2(c): how the two-values-per-step loop pairs the values of the checked rows.  For row i and every column chunk below it
    (chunk c with c C < i): the row's distinct values (first copies), 64 sketch positions at a time, those present in the chunk,
    in order, paired off.  Returns the count of every class of CLASSES over all (row, chunk) tasks."""
    sk = np.asarray(sk, dtype=np.uint64)
    S = sk.shape[1]
    out = dict.fromkeys(CLASSES, 0)
    for i in rows:
        row = sk[i]
        first = np.ones(S, dtype=bool)
        first[1:] = row[1:] != row[:-1]
        for c, (uniq, cnt) in enumerate(tables):
            if c * C >= i:
                break
            at = np.minimum(np.searchsorted(uniq, row), len(uniq) - 1)
            present = first & (uniq[at] == row)
            dense = cnt[at] >= Dm
            for b0 in range(0, S, 64):
                d = dense[b0:b0 + 64][present[b0:b0 + 64]]
                a, b = d[0:len(d) - 1:2], d[1::2]
                out["dense,dense"] += int((a & b).sum())
                out["dense,sparse"] += int((a & ~b).sum())
                out["sparse,dense"] += int((~a & b).sum())
                out["sparse,sparse"] += int((~a & ~b).sum())
                out["single"] += len(d) & 1
    return out


def assert_pair_classes(classes, least=10):
    short = {k: v for k, v in classes.items() if v < least}
    assert not short, f"pair classes met fewer than {least} times: {short} of {classes}"
