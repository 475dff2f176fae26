"""GPU tests of BIONJ (dpr_ctx_set_nj_variant(ctx, 1)): the device loop -- scan, lambda kernel, weighted update -- against the host
restatement dpr_nj_variant_host bit for bit (tests/test_bionj.py pins that restatement against a textbook BIONJ), partial runs,
context reuse across the variants, plan selection, and `dipper --bionj`."""
import os
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _bionj_ref, _nonfinite, _util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
KEYS = ("merge_x", "merge_y", "bl_x", "bl_y")


@pytest.fixture()
def dev():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    d.set_nj_variant(1)
    yield d
    d.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def run_device(d, chunks=(-1,)):
    """the context's loop on the matrix it holds, in pieces; (log with lam, iterations, code)"""
    got = {k: [] for k in KEYS}
    done, code, last = 0, 0, None
    n = d.n_total()
    for c in chunks:
        res = d.nj_run_partial(max_iters=c)
        for k in KEYS:
            got[k].append(res[k])
        done += res["iters"]
        code, last = res["code"], res["last_d"]
        if code != 0 or done >= n - 2:
            break
    log = {k: np.concatenate(got[k]) for k in KEYS}
    log["last_d"] = last
    log["lam"] = d.nj_lambda()
    return log, done, code


def assert_equals_host(log, done, code, M, variant=1):
    """M: the matrix the device loop started from"""
    from dipper_amd import capi
    n = M.shape[0]
    ref = capi.nj_variant_host(variant, M)
    assert done == ref["iters"], (done, ref["iters"], code)
    assert (code == -4) == (ref["iters"] < n - 2)
    for k in KEYS + (("lam",) if variant == 1 else ()):
        if not same_bits(log[k][:done], ref[k]):
            bad = int(np.flatnonzero(~((log[k][:done] == ref[k]) | ((log[k][:done] != log[k][:done]) & (ref[k] != ref[k]))))[0])
            raise AssertionError(f"{k} differs first at iteration {bad} of {done}: {log[k][bad]!r} vs {ref[k][bad]!r}")
    if code == 0:
        assert same_bits(log["last_d"], ref["last_d"]), (log["last_d"], ref["last_d"])
    return ref


def from_matrix(d, D, chunks=(-1,)):
    from dipper_amd import capi
    d.set_matrix_full(D)
    d.dist_matrix(capi.SRC_MATRIX)
    return run_device(d, chunks)


# ---- device against the host restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "additive_ties"])
@pytest.mark.parametrize("n", [3, 4, 5, 255, 256, 257, 513, 1000])
def test_device_equals_host_bit_for_bit(dev, n, kind):
    rng = np.random.default_rng(7 * n + (kind == "random"))
    D = _bionj_ref.random_matrix(rng, n) if kind == "random" else _util.random_additive_matrix(rng, n, zero_frac=0.4)
    log, done, code = from_matrix(dev, D)
    assert done == n - 2 and code == 0 and len(log["lam"]) == n - 2
    assert_equals_host(log, done, code, D)
    assert np.all((log["lam"] >= 0.0) & (log["lam"] <= 1.0))


def test_msa_source(dev):
    from dipper_amd import capi
    seqs = _util.synth_alignment(np.random.default_rng(3), n=130, L=700, mean_bl=2e-2, lo=2e-3, hi=2e-1)
    dev.set_msa(capi.pack4_many(seqs), 700)
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    M = dev.matrix()
    log, done, code = run_device(dev)
    assert done == 128 and code == 0
    assert_equals_host(log, done, code, M)


def test_protein_source(dev):
    from dipper_amd import capi
    seqs = _aa_ref.evolve_yule(np.random.default_rng(9), 90, 300)
    dev.set_msa_aa(capi.pack_aa_many(seqs))
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)
    M = dev.matrix()
    log, done, code = run_device(dev)
    assert done == 88 and code == 0
    assert_equals_host(log, done, code, M)


@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_nonfinite_distances_equal_host(dev, case):
    """the inputs of test_nj_nonfinite_distances_equal_oracle: the same log to the same end (all iterations, or the same
    iteration without a candidate), no NaN lambda"""
    name, D = _nonfinite.matrices(700, 31)[case]
    log, done, code = from_matrix(dev, D)
    assert_equals_host(log, done, code, D)
    assert done >= 1 and not np.any(np.isnan(log["lam"])), name


def test_partial_run_and_resume(dev):
    D = _bionj_ref.random_matrix(np.random.default_rng(12), 300)
    full, done, code = from_matrix(dev, D)
    parts, pdone, pcode = from_matrix(dev, D, chunks=(7, -1))
    assert (done, code) == (pdone, pcode) == (298, 0)
    for k in KEYS + ("lam", "last_d"):
        assert same_bits(full[k], parts[k]), k
    # after 7 iterations the getter holds 7 weights
    dev.dist_matrix(3)         # capi.SRC_MATRIX: the same matrix again
    dev.nj_run(max_iters=7)
    assert same_bits(dev.nj_lambda(), full["lam"][:7])


# ---- one context, both variants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0], ids=["pruned", "stream"])
def test_context_bionj_then_nj_then_bionj(orc, mode):
    import dipper_amd
    from dipper_amd import capi
    n = 400
    D = _util.random_additive_matrix(np.random.default_rng(21), n, zero_frac=0.3)
    E = np.tril(np.random.default_rng(22).normal(size=(n, n)), -1)
    D = np.round(D * np.exp(0.05 * (E + E.T)), 3)
    ref_nj = orc.nj_run(np.tril(D, -1))
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_mode(mode)
        d.set_nj_variant(1)
        log, done, code = from_matrix(d, D)
        ref_bj = assert_equals_host(log, done, code, D)
        assert not same_bits(ref_bj["merge_x"], ref_nj["merge_x"])          # the two logs differ on this input
        d.set_nj_variant(0)
        d.dist_matrix(capi.SRC_MATRIX)
        res = d.nj_run()
        for k in KEYS:
            assert same_bits(res[k], ref_nj[k]), k
        assert res["last_d"] == ref_nj["last_d"]
        with pytest.raises(capi.DipperError) as ei:
            d.nj_lambda()
        assert ei.value.code == -3
        d.set_nj_variant(1)
        log, done, code = from_matrix(d, D)
        assert_equals_host(log, done, code, D)
    finally:
        d.close()


def test_pruned_mode_request_is_ignored(dev):
    from dipper_amd import capi
    dev.set_nj_mode(1)
    dev.set_nj_adaptive(0)
    D = _bionj_ref.random_matrix(np.random.default_rng(5), 300)
    log, done, code = from_matrix(dev, D)
    assert_equals_host(log, done, code, D)
    with pytest.raises(capi.DipperError) as ei:
        dev.prune_stats()                           # no pruned state was built
    assert ei.value.code == -3
    assert dev.nj_multi_info() == "single rank"


def test_virtual_ranks_are_refused(orc):
    import dipper_amd
    from dipper_amd import capi
    D = _bionj_ref.random_matrix(np.random.default_rng(6), 200)
    ref = orc.nj_run(np.tril(D, -1))
    d = dipper_amd.Dipper(0, virtual_world=2)
    try:
        d.set_nj_variant(1)
        d.set_matrix_full(D)
        with pytest.raises(capi.DipperError) as ei:
            d.dist_matrix(capi.SRC_MATRIX)
        assert ei.value.code == -1 and "BIONJ" in str(ei.value)
        d.set_nj_variant(0)
        d.dist_matrix(capi.SRC_MATRIX)
        res = d.nj_run()
        for k in KEYS:
            assert same_bits(res[k], ref[k]), k
    finally:
        d.close()
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_variant(1)
        d.set_nj_virtual_shards(2)
        d.set_matrix_full(D)
        with pytest.raises(capi.DipperError) as ei:
            d.dist_matrix(capi.SRC_MATRIX)
        assert ei.value.code == -1
        d.set_nj_virtual_shards(-1)
        log, done, code = from_matrix(d, D)
        assert_equals_host(log, done, code, D)
    finally:
        d.close()


# ---- the command ------------------------------------------------------------------------------------------------------------
def run(*args):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def host_newick(names, M):
    from dipper_amd import capi
    g = capi.nj_variant_host(1, M)
    assert g["iters"] == len(names) - 2
    return _util.newick_from_merges(names, g["merge_x"], g["merge_y"], g["bl_x"], g["bl_y"], g["last_d"]), g


def device_matrix(seqs, dist_type, protein=False):
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        if protein:
            d.set_msa_aa(capi.pack_aa_many(seqs))
        else:
            d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
        d.dist_matrix(capi.SRC_MSA, dist_type)
        return d.matrix()
    finally:
        d.close()


@pytest.fixture(scope="module")
def aln(tmp_path_factory):
    seqs = _util.synth_alignment(np.random.default_rng(41), n=120, L=600, mean_bl=3e-2, lo=3e-3, hi=3e-1)
    names = [f"S{i+1}" for i in range(len(seqs))]
    fa = tmp_path_factory.mktemp("bionj") / "a.fa"
    _util.write_fasta(str(fa), names, seqs)
    return fa, names, seqs


def test_cli_matrix_input(tmp_path, orc):
    n = 150
    rng = np.random.default_rng(8)
    D = _util.random_additive_matrix(rng, n)
    E = np.tril(rng.normal(size=(n, n)), -1)
    D = D * np.exp(0.1 * (E + E.T))
    names = [f"X{i}" for i in range(n)]
    phy, out, out_nj = tmp_path / "d.phy", tmp_path / "b.nwk", tmp_path / "n.nwk"
    _util.write_phylip_lower(str(phy), names, D)
    r = run("-i", "d", "-I", str(phy), "-O", str(out), "--bionj")
    assert "Using conventional NJ (BIONJ)" in r.stderr
    Dr = np.zeros_like(D)
    for i in range(n):
        for j in range(i):
            Dr[i, j] = Dr[j, i] = orc.phylip_value("%.9g" % D[i, j])
    expect, _ = host_newick(names, Dr)
    assert out.read_text() == expect
    run("-i", "d", "-I", str(phy), "-O", str(out_nj))           # without the option nothing changes: NJ's tree, another one
    ref = orc.nj_run(np.tril(Dr, -1))
    assert out_nj.read_text() == _util.newick_from_merges(names, ref["merge_x"], ref["merge_y"], ref["bl_x"], ref["bl_y"], ref["last_d"])
    assert out_nj.read_text() != expect


def test_cli_alignment_input(tmp_path, aln):
    fa, names, seqs = aln
    out = tmp_path / "m.nwk"
    run("-i", "m", "-I", str(fa), "-O", str(out), "-m", "2", "-d", "2", "--seed", "-1", "--bionj")
    expect, _ = host_newick(names, device_matrix(seqs, 2))
    assert out.read_text() == expect


def test_cli_protein_input(tmp_path):
    seqs = _aa_ref.evolve_yule(np.random.default_rng(31), 100, 400)
    names = [f"P{i+1}" for i in range(len(seqs))]
    fa, out = tmp_path / "p.fa", tmp_path / "p.nwk"
    _util.write_fasta(str(fa), names, seqs, width=60)
    run("-i", "m", "--protein", "-I", str(fa), "-O", str(out), "-d", "8", "--seed", "-1", "--bionj")
    expect, _ = host_newick(names, device_matrix(seqs, 8, protein=True))
    assert out.read_text() == expect


def test_cli_bootstrap_one_and_two_ranks(tmp_path, aln):
    """the main tree and the three replicate trees are BIONJ trees: the file is the host-built main tree with the labels
    recomputed from three host-built replicate logs; two ranks on one GPU write the same bytes"""
    from tests.test_gpu_bootstrap import check_labels, replicate_seqs, strip_labels
    fa, names, seqs = aln
    o1, o2 = tmp_path / "one.nwk", tmp_path / "two.nwk"
    args = ["-i", "m", "-I", str(fa), "-m", "2", "-d", "2", "--seed", "-1", "--bionj", "--bootstrap", "3", "--bootstrap-seed", "5"]
    run(*args, "-O", str(o1))
    r2 = run(*args, "-O", str(o2), "--devices", "0,0")
    assert "Starting 2 ranks" in r2.stderr and "BIONJ, streaming, every rank its own copy" in r2.stderr, r2.stderr[-1500:]
    assert o1.read_bytes() == o2.read_bytes()
    text = o1.read_text()
    expect, _ = host_newick(names, device_matrix(seqs, 2))
    assert strip_labels(text) == expect
    rep_splits = []
    for r in range(3):
        nwk, _ = host_newick(names, device_matrix(replicate_seqs(seqs, 5, r), 2))
        rep_splits.append(_util.splits(nwk, names))
    check_labels(text, names, rep_splits)
