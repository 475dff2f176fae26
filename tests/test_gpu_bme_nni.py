"""GPU tests of the balanced minimum evolution NNI search (dpr_bme_nni): the device -- table kernels, lengths and gains -- against
the host restatement dpr_bme_nni_host bit for bit (tests/test_bme_nni.py pins that restatement against a textbook reference), over
the sizes where the launches change shape, every kind of start tree, every distance source and both matrix layouts; the state and
argument errors; and `dipper --nni`."""
import os
import subprocess

import numpy as np
import pytest

from tests import _aa_ref, _bme_ref as R, _util
from tests.test_bme_nni import FALLBACK_SEED, fallback_input, start_log

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
SIZES = [3, 4, 5, 6, 7, 63, 64, 65, 257, 600]
ROUNDS = 12


@pytest.fixture(scope="module")
def dev():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_same(got, ref):
    for k in ("rounds", "moves", "fallbacks", "candidates0", "top"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("kids", "L_rounds", "len"):
        assert same_bits(got[k], ref[k]), (k, got[k][:8], ref[k][:8])


def device_search(d, D, mx, my, rounds=ROUNDS):
    from dipper_amd import capi
    d.set_matrix_full(D)
    d.dist_matrix(capi.SRC_MATRIX)
    return d.bme_nni(mx, my, rounds)


_inputs = {}


def noisy(n):
    if n not in _inputs:
        _inputs[n] = R.random_matrix(np.random.default_rng(100 + n), n)
    return _inputs[n]


# ---- device against the host restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["nj", "bionj", "caterpillar", "balanced"])
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_bit_for_bit(dev, n, start):
    from dipper_amd import capi
    D = noisy(n)
    mx, my = start_log(start, n, D)
    got = device_search(dev, D, mx, my)
    assert_same(got, capi.bme_nni_host(D, mx, my, ROUNDS))
    if n >= 63 and start in ("caterpillar", "balanced"):
        assert got["rounds"] >= 2 and got["moves"] > got["rounds"]


@pytest.mark.parametrize("mode", [1, 0], ids=["pruned", "stream"])
@pytest.mark.parametrize("n", [5, 65, 600])
def test_both_matrix_layouts(n, mode):
    """the pruned plan keeps the fresh matrix in position space, the streaming plan in slot space: the same table either way"""
    import dipper_amd
    from dipper_amd import capi
    D = noisy(n)
    mx, my = start_log("balanced", n, D)
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_mode(mode)
        got = device_search(d, D, mx, my)
        assert_same(got, capi.bme_nni_host(D, mx, my, ROUNDS))
    finally:
        d.close()


def test_bionj_context(dev):
    from dipper_amd import capi
    n = 130
    D = noisy(n)
    dev.set_nj_variant(1)
    try:
        mx, my = start_log("bionj", n, D)
        assert_same(device_search(dev, D, mx, my), capi.bme_nni_host(D, mx, my, ROUNDS))
    finally:
        dev.set_nj_variant(0)


def test_alignment_source(dev):
    from dipper_amd import capi
    seqs = _util.synth_alignment(np.random.default_rng(3), n=130, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    dev.set_msa(capi.pack4_many(seqs), 300)
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    M = dev.matrix()
    mx, my = start_log("nj", 130, M)
    got = dev.bme_nni(mx, my, ROUNDS)
    assert_same(got, capi.bme_nni_host(M, mx, my, ROUNDS))


def test_protein_source(dev):
    from dipper_amd import capi
    seqs = _aa_ref.evolve_yule(np.random.default_rng(9), 90, 200)
    dev.set_msa_aa(capi.pack_aa_many(seqs))
    dev.dist_matrix(capi.SRC_MSA, capi.DIST_KIMURA)
    M = dev.matrix()
    mx, my = start_log("nj", 90, M)
    assert_same(dev.bme_nni(mx, my, ROUNDS), capi.bme_nni_host(M, mx, my, ROUNDS))


def test_recorded_fallback_input(dev):
    from dipper_amd import capi
    D, mx, my = fallback_input(FALLBACK_SEED)
    ref = capi.bme_nni_host(D, mx, my, 100)
    assert ref["fallbacks"] >= 1
    assert_same(device_search(dev, D, mx, my, 100), ref)


@pytest.mark.parametrize("bad", ["nan", "inf", "both", "inf_row"])
def test_nonfinite_distances(dev, bad):
    from dipper_amd import capi
    n = 100
    D = noisy(257)[:n, :n].copy()
    if bad in ("nan", "both"):
        D[7, 3] = D[3, 7] = np.nan
    if bad in ("inf", "both"):
        D[60, 2] = D[2, 60] = np.inf
    if bad == "inf_row":
        D[20, :] = D[:, 20] = np.inf
        D[20, 20] = 0.0
    mx, my = R.balanced_log(n)
    got = device_search(dev, D, mx, my)
    assert_same(got, capi.bme_nni_host(D, mx, my, ROUNDS))
    assert got["moves"] == 0


# ---- state, arguments, allocations ------------------------------------------------------------------------------------------
def test_state_error_after_an_nj_iteration(dev):
    from dipper_amd import capi
    n = 64
    D = noisy(n)
    mx, my = start_log("nj", n, D)
    dev.set_matrix_full(D)
    dev.dist_matrix(capi.SRC_MATRIX)
    dev.nj_run(max_iters=1)
    with pytest.raises(capi.DipperError) as ei:
        dev.bme_nni(mx, my, 3)
    assert ei.value.code == -3
    dev.dist_matrix(capi.SRC_MATRIX)                 # a fresh matrix again
    assert_same(dev.bme_nni(mx, my, 3), capi.bme_nni_host(D, mx, my, 3))
    with pytest.raises(capi.DipperError) as ei:      # a log that is none, and one of another size
        dev.bme_nni(my, mx, 3)
    assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        dev.bme_nni(mx[:10], my[:10], 3)
    assert ei.value.code == -1


def test_virtual_ranks_and_shards_are_refused():
    import dipper_amd
    from dipper_amd import capi
    n = 200
    D = noisy(257)[:n, :n]
    mx, my = start_log("nj", n, D)
    d = dipper_amd.Dipper(0, virtual_world=2)
    try:
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        with pytest.raises(capi.DipperError) as ei:
            d.bme_nni(mx, my, 3)
        assert ei.value.code == -1
        res = d.nj_run()                             # the context is as usable as before
        assert np.array_equal(res["merge_x"], mx) and np.array_equal(res["merge_y"], my)
    finally:
        d.close()
    d = dipper_amd.Dipper(0)
    try:
        d.set_nj_virtual_shards(2)
        d.set_matrix_full(D)
        d.dist_matrix(capi.SRC_MATRIX)
        with pytest.raises(capi.DipperError) as ei:
            d.bme_nni(mx, my, 3)
        assert ei.value.code == -1
        d.set_nj_virtual_shards(-1)
        assert_same(device_search(d, D, mx, my, 3), capi.bme_nni_host(D, mx, my, 3))
    finally:
        d.close()


def test_second_call_reuses_its_allocations():
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        n = 257
        D = noisy(n)
        mx, my = start_log("balanced", n, D)
        first = device_search(d, D, mx, my)
        s1 = d.bme_stats()
        assert s1["allocations"] == 4 and s1["table_bytes"] >= (2 * n - 2) ** 2 * 8 and s1["evaluations"] >= first["rounds"] + 1
        again = device_search(d, D, mx, my)
        s2 = d.bme_stats()
        assert_same(again, first)
        assert s2["allocations"] == 4 and s2["launches"] == s1["launches"]
        small = noisy(65)                            # fewer tips: the same buffers
        sx, sy = start_log("nj", 65, small)
        assert_same(device_search(d, small, sx, sy), capi.bme_nni_host(small, sx, sy, ROUNDS))
        assert d.bme_stats()["allocations"] == 4
        table_ms, select_ms = d.bme_timing()
        assert table_ms > 0 and select_ms > 0
    finally:
        d.close()


# ---- the command ------------------------------------------------------------------------------------------------------------
def run(*args):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def device_matrix(seqs, dist_type):
    import dipper_amd
    from dipper_amd import capi
    d = dipper_amd.Dipper(0)
    try:
        d.set_msa(capi.pack4_many(seqs), len(seqs[0]))
        d.dist_matrix(capi.SRC_MSA, dist_type)
        return d.matrix()
    finally:
        d.close()


@pytest.fixture(scope="module")
def aln(tmp_path_factory):
    seqs = _util.synth_alignment(np.random.default_rng(41), n=120, L=300, mean_bl=5e-2, lo=5e-3, hi=3e-1)
    names = [f"S{i+1}" for i in range(len(seqs))]
    fa = tmp_path_factory.mktemp("nni") / "a.fa"
    _util.write_fasta(str(fa), names, seqs)
    return fa, names, device_matrix(seqs, 2)


@pytest.mark.parametrize("variant,rounds", [(0, 0), (0, 20), (1, 20)], ids=["nni0", "nni20", "bionj_nni20"])
def test_cli_alignment_input(tmp_path, aln, variant, rounds):
    from dipper_amd import capi
    fa, names, M = aln
    out = tmp_path / "t.nwk"
    r = run("-i", "m", "-I", str(fa), "-O", str(out), "-m", "2", "-d", "2", "--seed", "-1", "--nni", str(rounds), *(["--bionj"] if variant else []))
    g = capi.nj_variant_host(variant, M)
    ref = capi.bme_nni_host(M, g["merge_x"], g["merge_y"], rounds)
    assert out.read_text() == R.newick(names, ref["kids"], ref["top"], ref["len"])
    line = [ln for ln in r.stderr.split("\n") if ln.startswith("BME NNI:")]
    assert len(line) == 1 and f", {ref['moves']} moves, {ref['rounds']} rounds, {ref['fallbacks']} fallbacks" in line[0], r.stderr[-800:]
    if rounds == 0:
        # the NJ topology with balanced lengths: the splits of the plain command's tree
        plain = tmp_path / "p.nwk"
        run("-i", "m", "-I", str(fa), "-O", str(plain), "-m", "2", "-d", "2", "--seed", "-1")
        assert _util.splits(out.read_text(), names) == _util.splits(plain.read_text(), names)
        assert plain.read_text() == _util.newick_from_merges(names, g["merge_x"], g["merge_y"], g["bl_x"], g["bl_y"], g["last_d"])


def test_cli_matrix_input(tmp_path, orc):
    from dipper_amd import capi
    n = 150
    D = noisy(257)[:n, :n]
    names = [f"X{i}" for i in range(n)]
    phy, out = tmp_path / "d.phy", tmp_path / "b.nwk"
    _util.write_phylip_lower(str(phy), names, D)
    run("-i", "d", "-I", str(phy), "-O", str(out), "--nni", "20")
    Dr = np.zeros_like(D)
    for i in range(n):
        for j in range(i):
            Dr[i, j] = Dr[j, i] = orc.phylip_value("%.9g" % D[i, j])
    g = capi.nj_variant_host(0, Dr)
    ref = capi.bme_nni_host(Dr, g["merge_x"], g["merge_y"], 20)
    assert out.read_text() == R.newick(names, ref["kids"], ref["top"], ref["len"])
