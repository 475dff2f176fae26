"""Inputs that sit on the edges of the Mash pair kernels and of the sketch kernel (dipper_amd/csrc/mash.hip), and the conditions
that say so.  Companion of tests/_mash_inputs.py, which does the same for the inverted-index kernel.

Table kernel (mash_dist_lookup_kernel).  The ROW tip (the higher index, list B of the merge) is resident: its sorted sketch, two
pad entries of ~0 behind it, and per bucket of its leading 9 significant bits the number of values below the bucket and eight
15-bit tags.  A wave holds one COLUMN sketch (the lower index, list A) in registers and walks it 64 positions per step.  Restated
here is the bookkeeping -- shift, bucket, tag, occupancy, duplicates, the cut-off position and the step at which the wave leaves --
with exact ranks (searchsorted) in place of the kernel's tag arithmetic.  The branch `bits <= 24` of the shift needs a sketch
whose largest value is below 2^24; no read produces one (64-bit hashes, or the padding value), so it is not reached and not built.

Token kernel (mash_encode_kernel, mash_dist_tokens_kernel).  Every sketch is encoded against the distinct values R of one tip as
RUN(p, len) and LIT(v, rk, EQ) tokens, exactly as the comment above mash_encode_kernel states them; the pair loop is ported step
for step so that a condition can say which rule a pair meets.  In that loop a bulk step is capped at S - uni, so when the `bend`
rule fires (two runs meet and B's run ends in the step) uni + Lp <= S - 1 always: `uni + Lp == S` cannot happen, and the edge next
to it is a B run that ends exactly at the cap (uni + Lp == S - 1).  That is what `bend_at_cap` counts.

The launch arithmetic of the host side (reference tip, sample stride, columns per block) is restated too.  Everything works on
sketches alone -- the oracle's in tests/test_mash_pair_inputs.py, the device's in tests/test_gpu_mash_pair_edges.py."""
import re

import numpy as np

from tests import _mash_inputs as mi
from tests import _util

PAD = mi.PAD

# the constants of mash.hip under their names there (tests/test_mash_pair_inputs.py holds them against the source)
kSortCap = 16384
kLS = 1024
kTB = 512
kLRows = 8
kLColsPerBlock = 512
kTWaves = 4
kTagsPerBucket = 8           # "8 x 15-bit tags per bucket": one uint4 of 16-bit fields
CONSTEXPR = dict(kSortCap=kSortCap, kLS=kLS, kTB=kTB, kLRows=kLRows, kLColsPerBlock=kLColsPerBlock, kTWaves=kTWaves)
PLACE_BATCH = 1024           # rows per placement batch of Mash input


def constants_in_source(text):
    """{name: value} of the `constexpr int NAME = VALUE;` lines of mash.hip for the names of CONSTEXPR, and the number of tag
    fields the bucket-table build fills per bucket (`uint32_t t8[N]`)"""
    found = {}
    for name in CONSTEXPR:
        m = re.findall(r"^constexpr int %s = (\d+);" % name, text, flags=re.M)
        assert len(m) == 1, (name, m)
        found[name] = int(m[0])
    t8 = re.findall(r"uint32_t t8\[(\d+)\];", text)
    assert len(t8) == 1, t8
    return found, int(t8[0])


def mash_distance(inter, uni, k):
    j = max(float(inter), 1.0) / uni
    return min(1.0, abs(np.log(2.0 * j / (1.0 + j)) / k))


def rand_bases(rng, L):
    return rng.integers(0, 4, size=L, dtype=np.uint8)


def to_read(*parts):
    return _util.BASES[np.concatenate(parts)].tobytes()


def mutate(rng, s, m):
    t = s.copy()
    if m:
        pos = rng.integers(0, len(t), size=m)
        t[pos] = (t[pos] + rng.integers(1, 4, size=m, dtype=np.uint8)) & 3
    return t


class Case:
    """reads, k, S, the (row, column) pairs (column < row) that carry the case's conditions, and conditions(sk) -> {name: count},
    which asserts them on sketches"""

    def __init__(self, name, reads, k, S, pairs, conditions):
        self.name, self.reads, self.k, self.S, self.pairs, self.conditions = name, reads, k, S, pairs, conditions
        self.n = len(reads)


def all_pairs(n):
    return [(i, j) for i in range(1, n) for j in range(i)]


# ---- table kernel: bookkeeping of one resident row ---------------------------------------------------------------------------------
def table_of(row):
    """bits, sh, bucket and tag of every value, occupancy of the kTB + 1 buckets, and whether the row holds a value twice"""
    row = np.asarray(row, dtype=np.uint64)
    mx = int(row[-1])
    bits = mx.bit_length() if mx else 1
    sh = bits - 9 if bits > 24 else 15
    bucket = bucket_of(row, sh)
    return dict(bits=bits, sh=sh, bucket=bucket, tag=tag_of(row, sh), occupancy=np.bincount(bucket, minlength=kTB + 1),
                dups=bool((row[1:] == row[:-1]).any()))


def bucket_of(v, sh):
    b = np.asarray(v, dtype=np.uint64) >> np.uint64(sh)
    return np.where(b >= np.uint64(kTB), np.uint64(kTB), b).astype(np.int64)


def tag_of(v, sh):
    return ((np.asarray(v, dtype=np.uint64) >> np.uint64(sh - 15)) & np.uint64(0x7FFF)).astype(np.int64)


def table_pair(A, B, bound=True):
    """The table formulation on column sketch A and row sketch B, in the kernel's order: a first copy in A matches when the row
    entry at its rank equals it -- with bound=True only at a rank below S (the two pad entries behind the row are no values) --
    takes the row's multiplicity, and counts while  position + rank - (multiplicities matched before it) < S;  after each step of
    64 positions the wave leaves when the next step cannot count.  Returns inter, the cut-off position (first position whose union
    rank is >= S; S if none), the steps run, and whether a pad entry matched."""
    A, B = np.asarray(A, dtype=np.uint64), np.asarray(B, dtype=np.uint64)
    S = len(A)
    ext = np.concatenate([B, [PAD, PAD]])
    pos = np.arange(S)
    rank = np.searchsorted(B, A, "left")
    first = np.ones(S, dtype=bool)
    first[1:] = A[1:] != A[:-1]
    match = first & (ext[rank] == A)
    if bound:
        match &= rank < S
    mult = np.where(match, np.maximum(np.searchsorted(B, A, "right") - rank, 1), 0)
    incl = np.cumsum(mult)
    union = pos + rank - (incl - mult)
    ok = match & (union < S)
    over = np.flatnonzero(union >= S)
    inter, steps = 0, 0
    for u in range(-(-S // 64)):
        sl = slice(64 * u, min(64 * u + 64, S))
        inter += int(mult[sl][ok[sl]].sum())
        steps = u + 1
        rb63 = int(rank[64 * u + 63]) if 64 * u + 63 < S else int(np.searchsorted(B, PAD, "left"))
        if 64 * (u + 1) >= S or 64 * (u + 1) + rb63 - int(incl[sl][-1]) >= S:
            break
    return dict(inter=inter, cut=int(over[0]) if len(over) else S, steps=steps, steps_all=-(-S // 64),
                phantom=bool((match & (rank >= S)).any()))


def phantom_condition(A, B):
    """column A padded, row B without padding and with duplicates, and the multiplicities in B of the values matched before A's
    first pad exceed that pad's position: the pad entry behind the row passes the cut-off"""
    A, B = np.asarray(A, dtype=np.uint64), np.asarray(B, dtype=np.uint64)
    if A[-1] != PAD or B[-1] == PAD or not (B[1:] == B[:-1]).any():
        return False
    p = int(np.searchsorted(A, PAD, "left"))
    head = np.unique(A[:p])
    matched = int((np.searchsorted(B, head, "right") - np.searchsorted(B, head, "left")).sum())
    return matched > p


def crowded_condition(A, B, dups):
    """row B (with / without duplicates) has a bucket of more than 8 entries -- distinct values when the row has no duplicates --
    and a value of column A is in the row at the 9th or a later place of such a bucket"""
    t = table_of(B)
    if t["dups"] != dups:
        return False
    crowded = t["occupancy"] > kTagsPerBucket
    lo = np.concatenate([[0], np.cumsum(t["occupancy"])])
    rank = np.searchsorted(B, A, "left")
    hit = (rank < len(B)) & (np.append(B, PAD)[rank] == A)
    kb = bucket_of(A, t["sh"])
    return bool((hit & crowded[kb] & (rank - lo[kb] >= kTagsPerBucket)).any())


def equal_tag_condition(A, B):
    """two different values of row B share bucket and tag, and column A holds the larger: the rank from the tags is that of the
    smaller and the walk has to move on"""
    t = table_of(B)
    key = t["bucket"] * 32768 + t["tag"]
    same = (key[1:] == key[:-1]) & (B[1:] != B[:-1])
    return bool(np.isin(B[1:][same], A).any())


def catch_all_condition(A, B):
    """column A holds real values at or above 2^bits of row B"""
    t = table_of(B)
    return t["bits"] < 64 and bool(((A != PAD) & (bucket_of(A, t["sh"]) == kTB)).any())


def multiplicities(A, B):
    ua, ca = np.unique(A[A != PAD], return_counts=True)
    ub, cb = np.unique(B[B != PAD], return_counts=True)
    both, ia, ib = np.intersect1d(ua, ub, return_indices=True)
    return ca[ia], cb[ib]


def count_pairs(sk, pairs, cond):
    return sum(1 for i, j in pairs if cond(sk[j], sk[i]))


def need(seen, name, least=10):
    assert seen[name] >= least, (name, seen)


# ---- table kernel: builders -----------------------------------------------------------------------------------------------------------
def phantom(seed=0, families=14):
    """The recipe of the padding defect, k = 15, S = 64: X = 54 random bases (40 k-mers, 24 pads), A = X, B = X + X + 0 .. 29 random
    bases (at least 94 k-mers, those of X twice).  Per family four tips A, B, B, A: the pair (B, A) with A as the column is on the
    edge, the pair (A, B) with B as the column is the same two reads in the other roles."""
    rng = np.random.default_rng(9100 + seed)
    reads, edge, swapped = [], [], []
    for _ in range(families):
        X = rand_bases(rng, 54)
        a, b = to_read(X), to_read(X, X, rand_bases(rng, int(rng.integers(0, 30))))
        t = len(reads)
        reads += [a, b, b, a]
        edge.append((t + 1, t))
        swapped.append((t + 3, t + 2))

    def conditions(sk):
        seen = dict(phantom=count_pairs(sk, edge, phantom_condition), swapped=count_pairs(sk, swapped, lambda A, B: phantom_condition(B, A)))
        need(seen, "phantom")
        need(seen, "swapped")
        seen["unbounded_differs"] = sum(1 for i, j in edge if table_pair(sk[j], sk[i], bound=False)["inter"] != table_pair(sk[j], sk[i])["inter"])
        assert not any(table_pair(sk[j], sk[i], bound=False)["phantom"] for i, j in swapped)
        return seen
    return Case("phantom", reads, 15, 64, edge + swapped, conditions)


def _families(rng, bases, clones, L, mutations, doubled=False):
    """per base read: the base and `clones` mutated copies, next to each other"""
    reads, pairs = [], []
    for _ in range(bases):
        b = rand_bases(rng, L)
        t = len(reads)
        for c in range(clones + 1):
            s = mutate(rng, b, mutations if c else 0)
            reads.append(to_read(s, s) if doubled else to_read(s))
        pairs += [(t + i, t + j) for i in range(1, clones + 1) for j in range(i)]
    return reads, pairs


def crowded(dups, seed=0):
    """S = 1 024.  Without duplicates: 24 unrelated reads of 1 500 bases, each with three clones (2 bases changed).  With: 12 reads of
    900 bases written twice in a row (every k-mer twice: a row of duplicates), each with three clones.  Pairs inside a family.  (A row
    of 1 024 values spread over 256 to 512 buckets has a bucket of more than 8 more often than not.)"""
    rng = np.random.default_rng(9200 + seed + (50 if dups else 0))
    reads, pairs = _families(rng, 12 if dups else 24, 3, 900 if dups else 1500, 2, doubled=dups)
    name = "crowded_dups" if dups else "crowded"

    def conditions(sk):
        seen = {name: count_pairs(sk, pairs, lambda A, B: crowded_condition(A, B, dups))}
        need(seen, name)
        return seen
    return Case(name, reads, 15, 1024, pairs, conditions)


def equal_tags(seed=0, tries=400):
    """S = 1 024: base reads of 1 300 bases are searched (at most `tries`) for sketches in which two different values share bucket
    and tag; of each of the first three hits a family of the read and four clones (1 base changed) is kept."""
    rng = np.random.default_rng(9300 + seed)
    reads, pairs = [], []
    from tests import _orc
    orc = _orc.load()
    for _ in range(tries):
        b = rand_bases(rng, 1300)
        r = to_read(b)
        sk = orc.sketch(orc.pack2(r), len(r), k=15, S=1024)
        if not equal_tag_condition(sk, sk):
            continue
        t = len(reads)
        reads += [r] + [to_read(mutate(rng, b, 1)) for _ in range(4)]
        pairs += [(t + i, t + j) for i in range(1, 5) for j in range(i)]
        if len(reads) == 15:
            break
    assert len(reads) == 15, "no sketch with equal tags found"

    def conditions(sk):
        seen = dict(equal_tags=count_pairs(sk, pairs, equal_tag_condition))
        need(seen, "equal_tags")
        return seen
    return Case("equal_tags", reads, 15, 1024, pairs, conditions)


def catch_all(seed=0):
    """S = 1 024: four reads of 20 000 bases as rows (sketch maximum near 2^64 / 20), their first 1 100 bases as columns (values up
    to the top of the range, far above 2^bits of a row): the catch-all bucket, and the wave leaves after its first step."""
    rng = np.random.default_rng(9400 + seed)
    long_ = [rand_bases(rng, 20000) for _ in range(4)]
    reads = [to_read(x[:1100]) for x in long_] + [to_read(x) for x in long_]
    pairs = [(4 + i, j) for i in range(4) for j in range(4)]

    def conditions(sk):
        seen = dict(catch_all=count_pairs(sk, pairs, catch_all_condition),
                    leaves_at_first_step=sum(1 for i, j in pairs if table_pair(sk[j], sk[i])["steps"] == 1))
        need(seen, "catch_all")
        need(seen, "leaves_at_first_step", 1)
        assert seen["leaves_at_first_step"] and table_pair(sk[0], sk[4])["steps_all"] == 16
        return seen
    return Case("catch_all", reads, 15, 1024, pairs, conditions)


def multiplicity(seed=0, families=8):
    """S = 256: per family Y (300 bases) written twice, three times, once, four times and twice with a tail, in that tip order"""
    rng = np.random.default_rng(9500 + seed)
    reads, pairs = [], []
    for _ in range(families):
        Y = rand_bases(rng, 300)
        t = len(reads)
        reads += [to_read(Y, Y), to_read(Y, Y, Y), to_read(Y), to_read(Y, Y, Y, Y), to_read(Y, Y, rand_bases(rng, 200))]
        pairs += [(t + i, t + j) for i in range(1, 5) for j in range(i)]

    def conditions(sk):
        def unequal(A, B):
            ma, mb = multiplicities(A, B)
            return bool(((ma >= 2) & (mb >= 2) & (ma != mb)).any())

        def two_one(A, B):
            ma, mb = multiplicities(A, B)
            return bool(((ma == 2) & (mb == 1)).any())
        seen = dict(unequal_multiplicities=count_pairs(sk, pairs, unequal), twice_in_A_once_in_B=count_pairs(sk, pairs, two_one))
        need(seen, "unequal_multiplicities")
        need(seen, "twice_in_A_once_in_B")
        return seen
    return Case("multiplicity", reads, 15, 256, pairs, conditions)


def cut_off(seed=0):
    """S = 1 024: 48 reads of a divergent family (1 500 bases, with indels): pairs whose cut-off position falls inside a step of 64
    and pairs where it is the first position of a step"""
    rng = np.random.default_rng(9600 + seed)
    reads = _util.synth_reads(rng, 48, 1500, mean_bl=2e-2, lo=2e-3, hi=8e-2)
    pairs = all_pairs(len(reads))

    def conditions(sk):
        cuts = np.array([table_pair(sk[j], sk[i])["cut"] for i, j in pairs])
        cut = cuts[(cuts > 0) & (cuts < sk.shape[1])]
        seen = dict(cut_inside_a_step=int((cut % 64 != 0).sum()), cut_at_a_step_boundary=int((cut % 64 == 0).sum()))
        need(seen, "cut_inside_a_step")
        need(seen, "cut_at_a_step_boundary", 1)
        return seen
    return Case("cut_off", reads, 15, 1024, pairs, conditions)


SKETCH_SIZES = (1, 63, 64, 65, 1023, 1024)


def sizes(S, seed=0):
    """a family for every sketch size of SKETCH_SIZES: 24 clonal reads of 2 500 bases, a read with every k-mer twice, its first half,
    short reads (padding) and unrelated reads"""
    rng = np.random.default_rng(9700 + seed)
    clonal = _util.synth_reads(rng, 24, 2500, mean_bl=3e-4, lo=3e-5, hi=3e-3)
    rep = (b"ACGTTGCA" * 40 + clonal[3][:1200]) * 2
    reads = clonal + [rep, rep[:len(rep) // 2], clonal[5], b"ACGT" * 30, b"A" * 40, b"AC", clonal[5][:300]]
    reads += [to_read(rand_bases(rng, int(L))) for L in (300, 1040, 2500)]

    def conditions(sk):
        assert sk.shape[1] == S
        return dict(steps=-(-S // 64), partial_last_step=int(S % 64 != 0))
    return Case(f"S={S}", reads, 15, S, all_pairs(len(reads)), conditions)


def shapes(seed=0, n=1100):
    """1 100 tips at S = 1 024 (reads of 1 300 bases, a divergent family): a second placement batch (rows from 2 + 1 024 on), a last
    row group of 4 rows, three column blocks of 512, and row groups whose rows all lie below a column block (the early return)"""
    rng = np.random.default_rng(9800 + seed)
    reads = _util.synth_reads(rng, n, 1300, mean_bl=5e-3, lo=5e-4, hi=5e-2)
    rows = sorted(set([1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 519, 520, 1023, 1024, 1025, 1026, 1027, n - 5, n - 4, n - 1]
                      + [int(i) for i in rng.integers(1, n, size=12)]))

    def conditions(sk):
        assert sk.shape == (n, 1024)
        seen = dict(rows_in_second_batch=n - (2 + PLACE_BATCH), last_row_group=n % kLRows, column_blocks=-(-n // kLColsPerBlock),
                    row_groups_below_a_column_block=sum(1 for t0 in range(0, n, kLRows) for c in range(0, n, kLColsPerBlock)
                                                        if c >= min(t0 + kLRows, n) - 1))
        assert n >= 1100 and seen["rows_in_second_batch"] > 0 and seen["last_row_group"] != 0
        assert (n - 2 - PLACE_BATCH) % kLRows != 0 and seen["column_blocks"] == 3 and seen["row_groups_below_a_column_block"] > 0
        return seen
    c = Case("shapes", reads, 15, 1024, [(i, j) for i in rows for j in range(0, i, 37)], conditions)
    c.rows = rows
    return c


# ---- token kernel: encoding and the pair loop -------------------------------------------------------------------------------------------
RUN, LIT = 0, 1


def _token_starts(X, R):
    """per element: rk = #{r in R : r < x}, inR, run element (first copy of a reference value), and whether a token starts there"""
    X, R = np.asarray(X, dtype=np.uint64), np.asarray(R, dtype=np.uint64)
    rk = np.searchsorted(R, X, "left")
    inR = (rk < len(R)) & (np.append(R, PAD)[rk] == X)
    first = np.ones(len(X), dtype=bool)
    first[1:] = X[1:] != X[:-1]
    runel = inR & first
    start = np.ones(len(X), dtype=bool)
    start[1:] = ~(runel[1:] & runel[:-1] & (rk[1:] == rk[:-1] + 1))
    return rk, inR, runel, start


def token_count(X, R):
    return int(_token_starts(X, R)[3].sum())


def encode(X, R):
    """tokens of sketch X against the reference list R: (RUN, p, len) or (LIT, v, rk, eq)"""
    rk, inR, runel, start = _token_starts(X, R)
    at = np.flatnonzero(start)
    end = np.append(at[1:], len(X))
    return [(RUN, int(rk[i]), int(e - i)) if runel[i] else (LIT, int(X[i]), int(rk[i]), bool(inR[i])) for i, e in zip(at, end)]


def decode(tokens, R):
    out = []
    for t in tokens:
        out += [int(R[t[1] + q]) for q in range(t[2])] if t[0] == RUN else [t[1]]
    return np.array(out, dtype=np.uint64)


class _Cursor:
    def __init__(self, tokens):
        self.t, self.i = tokens, 0
        self.advance()

    def advance(self):
        self.done = self.i >= len(self.t)
        if self.done:
            self.run, self.key, self.rem, self.val = False, 1, 1, 0
            return
        t = self.t[self.i]
        self.i += 1
        self.run = t[0] == RUN
        if self.run:
            self.key, self.rem, self.val = 2 * t[1] + 1, t[2], t[1]
        else:
            self.key, self.rem, self.val = 2 * t[2] + (1 if t[3] else 0), 1, t[1]

    def consume(self, L):
        self.rem -= L
        if self.run:
            self.key += 2 * L
        if L > 0 and self.rem == 0:
            self.advance()


def token_pair(tA, tB, S):
    """the loop of mash_dist_tokens_kernel on the tokens of column A and row B: (inter, uni, events).  Events: bend (B's run ends in
    a step of two runs), bend_at_cap (and that step is cut by S - uni), even_lt / even_gt / even_eq (two literals of one even key, B's
    value below / above / equal to A's)."""
    A, B = _Cursor(tA), _Cursor(tB)
    uni = inter = 0
    ev = dict(bend=0, bend_at_cap=0, even_lt=0, even_gt=0, even_eq=0)
    while uni < S and not A.done:
        cap = S - uni
        kA, kB, bdone = A.key, B.key, B.done
        eqk = (not bdone) and kB == kA
        odd = (kA & 1) != 0
        vlt, veq = B.val < A.val, B.val == A.val
        b_less = ((not bdone) and kB < kA) or (eqk and not odd and vlt)
        equal = eqk and (odd or veq)
        a_less = not (b_less or equal)
        pairs = equal and A.run and B.run
        Lb = (kA - kB + 1) >> 1 if B.run else 1
        La = A.rem if bdone else ((kB - kA + 1) >> 1 if A.run else 1)
        L = min(A.rem, B.rem) if pairs else min(Lb, B.rem) if b_less else min(La, A.rem) if a_less else 1
        L = min(L, cap)
        bend = pairs and L == B.rem
        Lp = L - (1 if bend else 0)
        if eqk and not odd:
            ev["even_eq" if veq else "even_lt" if vlt else "even_gt"] += 1
        if bend:
            assert uni + Lp < S
            ev["bend"] += 1
            ev["bend_at_cap"] += int(L == cap)
        cA = cB = du = di = 0
        if pairs:
            di = du = cA = cB = Lp
            if bend and uni + Lp < S:
                di += 1
                cB += 1
        elif b_less:
            du = cB = L
        elif a_less:
            du = cA = L
        else:
            di = cB = 1
        uni += du
        inter += di
        A.consume(cA)
        B.consume(cB)
    return inter, uni, ev


def reference_choice(sk):
    """(best tip, {candidate tip: tokens of the evaluated sample}) as mash_encode picks it: up to 16 evenly spaced candidates, tip 0
    first, on a sample of up to 256 evenly spaced sketches; the first of the cheapest wins"""
    n = len(sk)
    neval, ncand = min(n, 256), min(n, 16)
    estride = n // neval
    cost = {}
    for c in range(ncand):
        tip = c * (n // ncand) + ((n // ncand) // 2 if c else 0)
        R = np.unique(sk[tip])
        cost[tip] = sum(token_count(sk[q * estride], R) for q in range(neval))
    return min(cost, key=lambda t: (cost[t], t)), cost


def sample_step(n):
    """stride of the token-count sample: above 1 the strided copy is taken"""
    return n // min(n, 4096)


def cols_per_block(nr, ncols):
    tiles = -(-nr // 64)
    return max(8, min(128, ncols * tiles // 4096))


def token_events(sk, pairs, S):
    """events of the token loop summed over the pairs, under the reference the library picks, and the encodings"""
    best, _ = reference_choice(sk)
    R = np.unique(sk[best])
    toks = {}
    tot = dict(bend=0, bend_at_cap=0, even_lt=0, even_gt=0, even_eq=0)
    for i, j in pairs:
        for q in (i, j):
            if q not in toks:
                toks[q] = encode(sk[q], R)
        for name, v in token_pair(toks[j], toks[i], S)[2].items():
            tot[name] += v
    return tot, toks, R, best


def tokens_family(seed=0):
    """k = 15, S = 64, 30 tips.  Y: 200 random bases.  Tips: Y four times (one run each under the reference Y), eight clones of Y
    (runs and a few literals), ten reads Y + a stretch of Y (duplicates: runs that end where an extra copy of their last value
    follows, literals with EQ set), six clones of an unrelated Z and Z twice (all literals, pairs of literals between the same two
    reference values: in both orders, and equal)."""
    rng = np.random.default_rng(9900 + seed)
    Y, Z = rand_bases(rng, 200), rand_bases(rng, 200)
    reads = [to_read(Y)] * 2 + [to_read(mutate(rng, Y, 1)) for _ in range(8)]
    for _ in range(10):
        p0, ln = int(rng.integers(0, 120)), int(rng.integers(20, 80))
        reads.append(to_read(mutate(rng, Y, int(rng.integers(0, 2))), Y[p0:p0 + ln]))
    reads += [to_read(Y)] * 2 + [to_read(mutate(rng, Z, 1)) for _ in range(6)] + [to_read(Z)] * 2
    pairs = all_pairs(len(reads))

    def conditions(sk):
        S = sk.shape[1]
        tot, toks, R, best = token_events(sk, pairs, S)
        seen = dict(tot, one_run=sum(1 for t in toks.values() if len(t) == 1 and t[0][0] == RUN),
                    all_literals=sum(1 for t in toks.values() if len(t) == S and all(x[0] == LIT for x in t)),
                    eq_literals=sum(1 for t in toks.values() for x in t if x[0] == LIT and x[3]))
        for name in ("bend", "even_lt", "even_gt", "even_eq", "eq_literals"):
            need(seen, name)
        need(seen, "bend_at_cap", 1)
        need(seen, "one_run", 2)
        need(seen, "all_literals", 2)
        return seen
    return Case("tokens_family", reads, 15, 64, pairs, conditions)


def padded_reference(seed=0, n=20):
    """k = 15, S = 64: every tip is W + W with W of 35 bases (21 k-mers twice + 14 across the seam: 56 values, 8 pads) or a clone
    of it, so whichever tip becomes the reference holds duplicates and padding"""
    rng = np.random.default_rng(10000 + seed)
    W = rand_bases(rng, 35)
    reads = []
    for t in range(n):
        w = mutate(rng, W, 1 if t % 3 == 2 else 0)
        reads.append(to_read(w, w) if t % 4 else to_read(w, w, rand_bases(rng, 12)))
    pairs = all_pairs(n)

    def conditions(sk):
        best, _ = reference_choice(sk)
        ref = sk[best]
        seen = dict(reference_pads=int((ref == PAD).sum()), reference_duplicates=int((ref[1:] == ref[:-1]).sum() - max(int((ref == PAD).sum()) - 1, 0)))
        need(seen, "reference_pads", 2)
        need(seen, "reference_duplicates", 5)
        return seen
    return Case("padded_reference", reads, 15, 64, pairs, conditions)


def candidates(n, outlier, seed=0):
    """n = 15, 16, 17 tips, S = 64: fewer candidates than 16, exactly 16 (every tip), 16 of 17.  outlier: tip 0 is an unrelated
    read, so that it costs more tokens than another candidate and the reference is not tip 0."""
    rng = np.random.default_rng(10100 + seed + n)
    Y = rand_bases(rng, 400)
    reads = [to_read(mutate(rng, Y, int(rng.integers(0, 4)))) for _ in range(n)]
    if outlier:
        reads[0] = to_read(rand_bases(rng, 400))

    def conditions(sk):
        best, cost = reference_choice(sk)
        seen = dict(candidates=len(cost), best_tip=best, tip0_tokens=cost[0], best_tokens=cost[best])
        assert len(cost) == min(n, 16)
        if outlier:
            assert best != 0 and cost[0] > cost[best], seen
        return seen
    return Case(f"candidates n={n}{' outlier' if outlier else ''}", reads, 15, 64, all_pairs(n), conditions)


def strided_sample(seed=0, n=8200):
    """8 200 clonal reads of 60 bases at S = 8: the token-count sample takes every second tip (step = n / 4096 = 2) through the strided
    copy, the evaluation sample every 32nd, and a whole-matrix launch of the token kernel walks 128 columns per block"""
    rng = np.random.default_rng(10200 + seed)
    Y = rand_bases(rng, 60)
    s = np.tile(Y, (n, 1))
    hit = rng.random(n) < 0.7
    pos = rng.integers(0, 60, size=n)
    s[hit, pos[hit]] = (s[hit, pos[hit]] + rng.integers(1, 4, size=int(hit.sum()), dtype=np.uint8)) & 3
    reads = [r.tobytes() for r in _util.BASES[s]]
    rows = sorted(set([1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, n - 1] + [int(i) for i in rng.integers(1, n, size=17)]))

    def conditions(sk):
        seen = dict(sample_step=sample_step(len(sk)), cols_per_block=cols_per_block(len(sk), len(sk)), rows_checked=len(rows))
        assert seen["sample_step"] == 2 and seen["cols_per_block"] == 128 and n // 256 == 32
        return seen
    c = Case("strided_sample", reads, 15, 8, [(i, j) for i in rows[:8] for j in range(0, i, 97)], conditions)
    c.rows = rows
    return c


# ---- sketch kernel --------------------------------------------------------------------------------------------------------------------
def sketch_lengths(S, k=15):
    """read lengths on the sketch kernel's edges for sketch size S: the chunk of cap = kSortCap - S hashes (one short of it, exactly,
    one over, two chunks, two and one hash), the sort sizes (S + nk = 1 024, 1 025, 2 048, 2 049, kSortCap), reads around k, and
    lengths around a multiple of 32 bases (the last packed word)"""
    cap = kSortCap - S
    nks = [cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1] + [t - S for t in (1024, 1025, 2048, 2049, kSortCap) if t - S >= 1]
    return sorted(set([nk + k - 1 for nk in nks] + [k - 1, k, k + 1, 63, 64, 65, 4095, 4096, 4097]))


def sketch_reads(S, k=15, seed=0):
    rng = np.random.default_rng(10300 + seed + S)
    return [to_read(rand_bases(rng, L)) for L in sketch_lengths(S, k)]


def many_sequences(seed=0, n=1030):
    """more sequences than the sketch grid of 1 024 blocks: blocks 0 .. 5 take a second sequence, the last one a long read"""
    rng = np.random.default_rng(10400 + seed)
    return [to_read(rand_bases(rng, int(L))) for L in rng.integers(10, 90, size=n - 1)] + [to_read(rand_bases(rng, 40000))]


# ---- divide and conquer -----------------------------------------------------------------------------------------------------------------
def dc_family(seed=0, B=24, families=6):
    """k = 15, S = 64, backbone of B unrelated reads of 110 bases; backbone read 3 f + 1 of family f is X + X + tail (X = 54 bases).
    Queries of family f, in this order: X (padded), X + X + tail' (duplicates, no padding: the pair of the padding defect, with the
    padded tip as the earlier member), X + X, and a clone of the backbone read."""
    rng = np.random.default_rng(10500 + seed)
    back = [to_read(rand_bases(rng, 110)) for _ in range(B)]
    queries, edge = [], []
    for f in range(families):
        X = rand_bases(rng, 54)
        tail = rand_bases(rng, 20)
        back[3 * f + 1] = to_read(X, X, tail)
        t = B + len(queries)
        queries += [to_read(X), to_read(X, X, rand_bases(rng, int(rng.integers(0, 30)))), to_read(X, X), to_read(X, mutate(rng, X, 1), tail)]
        edge.append((t + 1, t))
    reads = back + queries

    def conditions(sk):
        seen = dict(phantom=count_pairs(sk, edge, phantom_condition))
        need(seen, "phantom", 4)
        return seen
    c = Case("dc_family", reads, 15, 64, all_pairs(len(reads)), conditions)
    c.B, c.edge = B, edge
    return c


TABLE_BUILDERS = dict(phantom=phantom, crowded=lambda: crowded(False), crowded_dups=lambda: crowded(True), equal_tags=equal_tags,
                      catch_all=catch_all, multiplicity=multiplicity, cut_off=cut_off)
TOKEN_BUILDERS = dict(tokens_family=tokens_family, padded_reference=padded_reference)
_CASES = {}


def case(name, build):
    """builders are deterministic: one instance per name and process"""
    if name not in _CASES:
        _CASES[name] = build()
    return _CASES[name]
