"""The pruned NJ scan with TWO blocks per listed unit (rows 0-7 and 8-15, njp_scan_kernel<.., 2>): two records per list entry,
two words per sub-unit bound.  Every case compares the pruned loop's whole merge log (merge_x, merge_y, bl_x, bl_y, last_d) bit
for bit with the streaming loop (set_nj_mode(0)) on the same matrix and, where the oracle is quick (N <= 1 500), with the
oracle as tests/test_gpu_nj.py does.  Shapes: the smallest at which the split can go wrong -- a tied clique across the row 7 | 8
seam, position counts that leave the last unit's second half empty / partial / full, blocks that walk several entries, epoch
rebuilds and resumed runs, unit-sharded and row-sharded virtual ranks, non-finite input, the large launch shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu

LOG = ("merge_x", "merge_y", "bl_x", "bl_y")
_stream = {}      # reference runs of the streaming loop, one per matrix
_oracle = {}      # ... and of the oracle


def _run(D, mode, chunks=(10 ** 9,), make=None):
    """the NJ loop on D in pieces of `chunks` iterations: (log arrays, iterations done, code, last_d)"""
    import dipper_amd
    from dipper_amd import capi
    d = make() if make else dipper_amd.Dipper(0)
    try:
        d.set_nj_mode(mode)
        if make is None:
            d.set_nj_adaptive(0)          # the pruned plan from the first to the last iteration
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        got = {k: [] for k in LOG}
        done, code, last = 0, 0, None
        for c in chunks:
            res = d.nj_run_partial(max_iters=c)
            for k in LOG:
                got[k].append(res[k])
            done += res["iters"]
            code, last = res["code"], res["last_d"]
            if code != 0 or done >= D.shape[0] - 2:
                break
        return {k: np.concatenate(got[k]) for k in LOG}, done, code, last
    finally:
        d.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_log(got, ref, what):
    g, gdone, gcode, glast = got
    r, rdone, rcode, rlast = ref
    assert (gdone, gcode) == (rdone, rcode), what
    for k in LOG:
        if not np.array_equal(_bits(g[k]), _bits(r[k][:gdone])):
            bad = int(np.flatnonzero(_bits(g[k]) != _bits(r[k][:gdone]))[0])
            raise AssertionError(f"{what}: {k} differs first at iteration {bad} of {gdone}: {g[k][bad]} vs {r[k][bad]}")
    if gcode == 0:
        assert np.float64(glast).view(np.uint64) == np.float64(rlast).view(np.uint64), what


def _stream_ref(name, D):
    if name not in _stream:
        _stream[name] = _run(D, 0)
    return _stream[name]


def _check(name, D, orc=None, **kw):
    ref = _stream_ref(name, D)
    got = _run(D, 1, **kw)
    _same_log(got, ref, name + ": pruned vs streaming")
    if orc is not None and D.shape[0] <= 1500:
        if name not in _oracle:
            _oracle[name] = orc.nj_run(np.tril(D, -1))
        ref = _oracle[name]
        assert ref["iters"] == got[1] == D.shape[0] - 2
        _same_log(got, ({k: ref[k] for k in LOG}, got[1], 0, ref["last_d"]), name + ": pruned vs oracle")
    return got


def _additive(n, seed, ties=True):
    rng = np.random.default_rng(seed)
    D = _util.random_additive_matrix(rng, n, zero_frac=0.4 if ties else 0.0)
    return np.round(D, 1) if ties else D


def _n1500():
    D = _additive(1500, 77)
    _stream_ref("n1500", D)          # (before a test changes the plan or the environment)
    return D


def clonal_matrix(min_groups=42):
    """Near-clonal p-distances over 256 sites (multiples of 1 / 256: every row sum is exact in any order, so the order by row
    sum is the same here and on the GPU): groups of 12 - 20 identical sequences, i.e. exact Q ties inside and between the
    groups.  The seed is searched for until one group of 12 sits on positions 16 k + 2 ... 16 k + 13 of the (stable) order
    by row sum: rows 2 - 7 of a unit in the first half-block, rows 8 - 13 in the second.  Returns (D, first position)."""
    for seed in range(400):
        rng = np.random.default_rng(seed)
        sizes = np.where(rng.random(min_groups) < 0.5, 12, rng.integers(13, 21, min_groups))
        G = len(sizes)
        k = rng.integers(1, 9, size=(G, G))
        Dg = (np.tril(k, -1) + np.tril(k, -1).T) / 256.0
        group = np.repeat(np.arange(G), sizes)
        perm = rng.permutation(len(group))          # tips of a group are scattered over the input order
        group = group[perm]
        D = Dg[np.ix_(group, group)]
        order = np.argsort(D.sum(axis=1), kind="stable")
        gs = group[order]
        for g in np.flatnonzero(sizes == 12):
            pos = np.flatnonzero(gs == g)
            if pos[0] % 16 == 2 and pos[-1] - pos[0] == 11:
                return D, int(pos[0])
    raise AssertionError("no seed places a group of 12 on positions 16 k + 2 ... 16 k + 13")


def test_tied_clique_across_the_half_seam(orc):
    D, p0 = clonal_matrix()
    n = D.shape[0]
    assert 500 <= n <= 800 and p0 % 16 == 2
    got = _check("clonal", D, orc)
    # the premise: identical sequences are joined at distance 0 throughout (the ties are real)
    assert np.count_nonzero((got[0]["bl_x"] == 0.0) & (got[0]["bl_y"] == 0.0)) >= n // 2


@pytest.mark.parametrize("n", [513, 519, 520, 521, 527])
def test_ragged_position_counts(orc, n):
    """P % 16 in {1, 7, 8, 9, 15}: the last unit's second half holds no row (its first half one row, seven rows, all eight),
    one row, seven rows; N <= 1 024 has only diagonal units plus one strip below them"""
    _check(f"ragged{n}", _additive(n, 4000 + n), orc)


@pytest.mark.parametrize("grid", [3, 37])
def test_blocks_walk_several_entries(orc, monkeypatch, grid):
    """cnt > ugrid: the two halves of one entry sit in different passes of different blocks, and the seed records are the
    first 2 x grid ones"""
    D = _n1500()
    monkeypatch.setenv("DPR_NJP_GRID", str(grid))
    _check("n1500", D, orc)


def test_epochs_and_resumed_runs(orc, monkeypatch):
    """several rebuilds (the first full scan of each epoch on the new grid), the run interrupted between iterations"""
    D = _n1500()
    monkeypatch.setenv("DPR_NJ_EPOCH_MIN", "256")
    _check("n1500", D, orc, chunks=(1500 // 2 + 7, 1, 1500 // 4, 5, 10 ** 9))


@pytest.mark.parametrize("world", [2, 3])
def test_unit_sharded_virtual_ranks(orc, monkeypatch, world):
    """record offsets (2 x ugrid per rank) and the size of the gathered array"""
    from dipper_amd import capi
    D = _n1500()
    monkeypatch.setenv("DPR_NJ_EPOCH_MIN", "256")
    capi.set_nj_virtual_shards(world)
    try:
        _check("n1500", D, orc, chunks=(500, 7, 10 ** 9))
    finally:
        capi.set_nj_virtual_shards(1)


def test_row_sharded_virtual_ranks(orc, monkeypatch):
    """the one-block instantiation on the eight-word layout of the bounds (second word +inf)"""
    import dipper_amd
    D = _n1500()
    monkeypatch.setenv("DPR_NJ_EPOCH_MIN", "256")

    def make():
        d = dipper_amd.Dipper(0, virtual_world=2)
        d.set_nj_multi_plan(3)              # rows sharded, pruned
        d.set_nj_exchange(1)                # collective
        return d
    _check("n1500", D, orc, make=make, chunks=(500, 7, 10 ** 9))


@pytest.mark.parametrize("case", [0, 3], ids=["nan_pair", "inf_row"])
def test_nonfinite_input(orc, case):
    """one NaN pair / one +inf tip: the same end state as the streaming loop, DPR_ERR_NOCAND progress included"""
    from tests import _nonfinite
    name, D = _nonfinite.matrices(600, 53)[case]
    got = _check("nonfinite_" + name, D)
    ref = orc.nj_run(np.tril(D, -1))
    assert got[1] == ref["done"] and (got[2] == -4) == (ref["iters"] == -1)
    assert got[1] >= 590


def _large_shape_worker():
    D = _additive(3000, 91)
    _same_log(_run(D, 1, chunks=(1000, 7, 10 ** 9)), _run(D, 0), "large shape: pruned vs streaming")
    print("RESULT " + json.dumps({"ok": True}))


@pytest.mark.parametrize("post2", ["1", "0"])
def test_large_launch_shape(post2):
    """DPR_NJ_BIG_P lowered (read once per process: a process of its own): njp_post2_kernel<4> with its coarse cells, and the
    fused njp_post_kernel<256, 4>, on the two-word bounds at N = 3 000"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DPR_NJ_BIG_P="1", DPR_NJP_POST2=post2, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_njp_half_units"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and line, (r.stdout[-2000:], r.stderr[-3000:])
    assert json.loads(line[0][7:])["ok"]


if __name__ == "__main__":
    _large_shape_worker()
