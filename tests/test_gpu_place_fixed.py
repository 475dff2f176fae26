"""GPU parity of the independent placement on a fixed backbone (dpr_place_fixed_set / dpr_place_fixed_run) through the C ABI.

Per query the oracle is run once on a fresh copy of the backbone state -- the helper's adjacency arrays, place_init_lists,
place_run(first = m) with the query's GPU distance row as row m -- and trace[m] = (slot, frac, add) must equal the GPU's
triple bit for bit.  The oracle places every tip from `first` on, so its state is sized for m + 1 tips: the query is the only one
placed.  Node ids do not enter the arithmetic and the order of a slot's two ends (belong >= e) is the same for any number of tips
(leaf < first internal id <= every internal id, internal ids ascend in pre-order); test_oracle_state_size_does_not_matter pins
that against the literal n-tip state.  All aligned inputs have 200 sites and distances <= 0.5, so add <= 1 and the oracle's
default tuple (slot 0, add 2) never wins; every test asserts add < 2 for every query."""
import numpy as np
import pytest

from tests import _jplace, _util
from tests.conftest import dirty_device_memory
from tests.test_gpu_mash_place import _reads

pytestmark = pytest.mark.gpu

SITES = 200
QMAX = 200
SHAPES = [(3, "caterpillar"), (4, "balanced"), (6, "random"), (40, "random"), (300, "random")]
COUNTS = [1, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_INPUT = {}


def backbone(m):
    kind = dict(SHAPES)[m]
    return _jplace.random_backbone(np.random.default_rng(100 + m), m, kind)


def alignment(m):
    """m + QMAX sequences of 200 sites, all p-distances <= 0.36 (JC <= 0.5); query 5 is a copy of backbone tip 2 (its distance
    row is that tip's: a tie with it on every edge)"""
    if ("aln", m) not in _INPUT:
        rng = np.random.default_rng(200 + m)
        seqs = _util.synth_alignment(rng, m + QMAX, SITES, mean_bl=6e-3, lo=1e-3, hi=2e-2)
        seqs[m + 5] = seqs[2]
        a = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), SITES)
        p = (a[:, None, :] != a[None, :, :]).mean(axis=2)
        assert p.max() <= 0.36, p.max()
        _INPUT[("aln", m)] = seqs
    return _INPUT[("aln", m)]


def reads(m):
    if ("reads", m) not in _INPUT:
        _INPUT[("reads", m)] = _reads(np.random.default_rng(300 + m), m + QMAX, 1500, 2500)
    return _INPUT[("reads", m)]


_ORACLE = {}


def oracle(orc, m, rows, n_state=None):
    """(slot, frac, add) of every row of `rows` (distances of a query to the m backbone tips) from one oracle run each"""
    N = n_state or m + 1
    key = (m, N)
    if key not in _ORACLE:
        st, _ = _jplace.backbone_arrays(orc, backbone(m), N)
        orc.place_init_lists(N, m, st)
        _ORACLE[key] = (st, {})
    st0, done = _ORACLE[key]
    out = np.zeros((len(rows), 3))
    for i, row in enumerate(rows):
        k = row.tobytes()
        if k not in done:
            st = {name: v.copy() for name, v in st0.items()}
            D = np.zeros((N, N))
            D[m, :m] = row
            done[k] = orc.place_run(D, first=m, state=st)["trace"][m].copy()
        out[i] = done[k]
    return out[:, 0].astype(np.int32), out[:, 1].copy(), out[:, 2].copy()


def same(got, ref):
    slot, frac, add = got
    rs, rf, ra = ref
    assert np.all(add < 2.0)
    assert np.array_equal(slot, rs), np.flatnonzero(slot != rs)[:8]
    assert np.array_equal(_bits(add), _bits(ra)), np.flatnonzero(_bits(add) != _bits(ra))[:8]
    assert np.array_equal(_bits(frac), _bits(rf)), np.flatnonzero(_bits(frac) != _bits(rf))[:8]


def set_backbone(gpu, orc, m, n):
    st, _ = _jplace.backbone_arrays(orc, backbone(m), n)
    gpu.place_fixed_set(m, n, st)
    return st


def load_msa(gpu, orc, m, c, batch=64):
    from dipper_amd import capi
    gpu.set_msa(capi.pack4_many(alignment(m)[:m + c]), SITES)
    gpu.set_place_fixed_batch(batch)
    return set_backbone(gpu, orc, m, m + c)


@pytest.mark.parametrize("dist_type", [1, 2])
@pytest.mark.parametrize("c", COUNTS)
@pytest.mark.parametrize("m", [s[0] for s in SHAPES])
def test_msa_matches_oracle(gpu, orc, m, c, dist_type):
    from dipper_amd import capi
    st = load_msa(gpu, orc, m, c)
    got = gpu.place_fixed_run(capi.SRC_MSA, dist_type)
    rows, _ = gpu.msa_dist_block(m, c, m, dist_type)
    assert rows.max() <= 0.5
    same(got, oracle(orc, m, rows))
    lim = 4 * m - 4
    assert np.all(got[0] >= 0) and np.all(got[0] < lim) and np.all(st["belong"][got[0]] >= st["e"][got[0]])     # eligible slots only


@pytest.mark.parametrize("c", COUNTS)
@pytest.mark.parametrize("m", [s[0] for s in SHAPES])
def test_mash_matches_oracle(gpu, orc, m, c):
    from dipper_amd import capi
    gpu.set_reads(reads(m)[:m + c])
    gpu.sketch(k=15, S=1000, fetch=False)
    gpu.set_place_fixed_batch(64)
    set_backbone(gpu, orc, m, m + c)
    got = gpu.place_fixed_run(capi.SRC_MASH, 0, k=15)
    gpu.dist_matrix(capi.SRC_MASH, 0, 15)
    rows = np.ascontiguousarray(gpu.matrix()[m:, :m])
    same(got, oracle(orc, m, rows))
    again = gpu.place_fixed_run(capi.SRC_MASH, 0, k=15)                          # (the distance matrix left the table alone)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def test_oracle_state_size_does_not_matter(gpu, orc):
    """the oracle on the literal state (sized for all n tips, internal ids from n) gives the triples of the m + 1 state"""
    from dipper_amd import capi
    m, c = 6, 65
    load_msa(gpu, orc, m, c)
    rows, _ = gpu.msa_dist_block(m, c, m, 2)
    a, b = oracle(orc, m, rows), oracle(orc, m, rows, n_state=m + c)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    same(gpu.place_fixed_run(capi.SRC_MSA, 2), b)


@pytest.mark.parametrize("batch", [0, 1, 64, 100])
def test_batch_size_and_scan_form_do_not_matter(gpu, orc, monkeypatch, batch):
    """0 = the rule of dpr_dc_run (one batch here), 1 and 100 are no multiples of the 64 queries of a workgroup; the scan that
    carries the position through its loop (DPR_PFIX_CARRY=1) gives the bits of the one whose reduce step evaluates the winner again"""
    from dipper_amd import capi
    m, c = 40, 130
    load_msa(gpu, orc, m, c, batch=batch)
    rows, _ = gpu.msa_dist_block(m, c, m, 2)
    ref = oracle(orc, m, rows)
    same(gpu.place_fixed_run(capi.SRC_MSA, 2), ref)
    monkeypatch.setenv("DPR_PFIX_CARRY", "1")
    same(gpu.place_fixed_run(capi.SRC_MSA, 2), ref)


@pytest.mark.parametrize("m", [4, 40, 300])
def test_identical_sequences_go_to_the_lowest_eligible_slot(gpu, orc, m):
    from dipper_amd import capi
    c = 70
    gpu.set_msa(capi.pack4_many([alignment(m)[0]] * (m + c)), SITES)
    gpu.set_place_fixed_batch(64)
    st = set_backbone(gpu, orc, m, m + c)
    slot, frac, add = gpu.place_fixed_run(capi.SRC_MSA, 1)
    lowest = int(np.flatnonzero(st["belong"][:4 * m - 4] >= st["e"][:4 * m - 4])[0])
    assert np.all(add == 0.0) and np.all(slot == lowest)
    same((slot, frac, add), oracle(orc, m, np.zeros((c, m))))


def test_state_across_runs_resampling_and_other_placement_runs(gpu, orc):
    import dipper_amd
    from dipper_amd import capi
    m, c = 40, 90
    load_msa(gpu, orc, m, c)
    first = gpu.place_fixed_run(capi.SRC_MSA, 2)
    second = gpu.place_fixed_run(capi.SRC_MSA, 2)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    # replicates: the context's current planes are scored, the backbone and its lists stay
    main_rows, _ = gpu.msa_dist_block(m, c, m, 2)
    for r in (0, 3):
        gpu.msa_resample(11, r)
        rows, _ = gpu.msa_dist_block(m, c, m, 2)
        assert not np.array_equal(rows, main_rows)
        same(gpu.place_fixed_run(capi.SRC_MSA, 2), oracle(orc, m, rows))
    gpu.msa_resample(11, -1)
    for a, b in zip(first, gpu.place_fixed_run(capi.SRC_MSA, 2)):
        assert np.array_equal(a, b)
    # a placement run rebuilds the placement state: it equals a fresh context's, and the fixed backbone is gone
    n = m + c
    st_a, _ = _jplace.backbone_arrays(orc, backbone(m), n)
    st_b = {k: v.copy() for k, v in st_a.items()}
    got = gpu.place_run(capi.SRC_MSA, n, first=m, dist_type=2, state=st_a)
    fresh = dipper_amd.Dipper(0)
    try:
        fresh.set_msa(capi.pack4_many(alignment(m)[:n]), SITES)
        ref = fresh.place_run(capi.SRC_MSA, n, first=m, dist_type=2, state=st_b)
    finally:
        fresh.close()
    live = 4 * n - 4                                                             # (the arrays hold 8n slots; the lists of the unused ones are never written)
    for key in ("head", "e", "nxt", "belong", "len", "cid", "cdis", "trace"):
        k = {"head": 2 * n, "trace": n, "cid": 5 * live, "cdis": 5 * live}.get(key, live)
        assert np.array_equal(got[key][:k], ref[key][:k]), key
    with pytest.raises(capi.DipperError, match="dpr_place_fixed_set first") as ei:
        gpu.place_fixed_run(capi.SRC_MSA, 2)
    assert ei.value.code == -3
    set_backbone(gpu, orc, m, n)
    for a, b in zip(first, gpu.place_fixed_run(capi.SRC_MSA, 2)):
        assert np.array_equal(a, b)


def test_errors_are_clean(orc):
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        with pytest.raises(capi.DipperError, match="dpr_place_fixed_set first"):
            d.place_fixed_run(capi.SRC_MSA, 2)
        m, n = 6, 10
        st, _ = _jplace.backbone_arrays(orc, backbone(m), n)
        bad = {k: v.copy() for k, v in st.items()}
        bad["e"][4 * m - 5] = -1                                                 # a polytomy leaves a slot unused: what --add rejects
        with pytest.raises(capi.DipperError, match="not a rooted binary tree"):
            d.place_fixed_set(m, n, bad)
        with pytest.raises(capi.DipperError, match="bad argument"):
            d.place_fixed_set(n, n, st)
        d.place_fixed_set(m, n, st)
        with pytest.raises(capi.DipperError, match="dpr_set_msa"):               # no input yet
            d.place_fixed_run(capi.SRC_MSA, 2)
        with pytest.raises(capi.DipperError, match="sequences"):
            d.place_fixed_run(capi.SRC_MATRIX, 2)
    finally:
        d.close()


def test_dirty_device_memory_changes_nothing(orc):
    """device memory full of 0xFF (NaN as fp64) before the context's allocations: nothing is read before it is written"""
    import dipper_amd
    from dipper_amd import capi
    m, c = 40, 65
    out = []
    for dirty in (False, True):
        if dirty:
            capi.load_library()
            dirty_device_memory(2 << 30, 0xFF)
        d = dipper_amd.Dipper(0)
        try:
            out.append(load_and_run(d, orc, m, c))
        finally:
            d.close()
    for a, b in zip(*out):
        assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)


def load_and_run(d, orc, m, c):
    from dipper_amd import capi
    load_msa(d, orc, m, c)
    return d.place_fixed_run(capi.SRC_MSA, 2)
