"""GPU parity: the upload of a packed alignment (dpr_set_msa) gives the same bit planes -- hence the same integer counts --
however the caller's array lies in memory, at every edge of a packed word and of a plane word.  (The upload has one route, a
plain copy: the two routes measured against it were not kept, so there is no switch to vary here -- DESIGN 6.)"""
import mmap

import numpy as np
import pytest

from tests import _util

pytestmark = pytest.mark.gpu

NS = (2, 3, 65)
LS = (1, 15, 16, 17, 31, 32, 33, 1025)      # the edges of a packed word (16 sites) and of a plane word (32)
PAGE = mmap.PAGESIZE


@pytest.fixture(scope="module")
def gpu():
    import dipper_amd
    d = dipper_amd.Dipper(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases(orc):
    """(n, L, packed, useful, match) of every shape, gaps and N present; computed once, never written to"""
    from dipper_amd import capi
    out = []
    for n in NS:
        for L in LS:
            rng = np.random.default_rng(1000 * n + L)
            seqs = _util.synth_alignment(rng, n, L, mean_bl=5e-2, lo=1e-3, hi=2e-1, invalid_frac=0.25)
            seqs[0] = b"N" + seqs[0][1:]
            seqs[-1] = seqs[-1][:-1] + b"-"
            packed = capi.pack4_many(seqs)
            u, m = orc.msa_counts(packed, L)
            packed.setflags(write=False)
            out.append((n, L, packed, u, m))
    return out


def _at_offset(packed, off):
    """a writable copy of packed whose first byte lies `off` bytes past a page boundary"""
    raw = np.empty(packed.nbytes + 2 * PAGE, dtype=np.uint8)
    start = (-raw.ctypes.data) % PAGE + off
    view = raw[start:start + packed.nbytes].view(np.uint64).reshape(packed.shape)
    view[...] = packed
    assert view.ctypes.data % PAGE == off
    return view


def _check_counts(gpu, n, u_ref, m_ref, what):
    for row in range(1, n):
        u, m = gpu.msa_counts(row)
        assert np.array_equal(u, u_ref[row, :row]), what + f" useful, row {row}"
        assert np.array_equal(m, m_ref[row, :row]), what + f" match, row {row}"


@pytest.mark.parametrize("layout", ["page_aligned", "page_plus_8", "readonly_memmap", "overwritten_after"])
def test_counts_every_layout(gpu, cases, tmp_path, layout):
    for n, L, packed, u_ref, m_ref in cases:
        what = f"n={n} L={L} {layout}"
        if layout == "page_aligned":
            arr = _at_offset(packed, 0)
        elif layout == "page_plus_8":
            arr = _at_offset(packed, 8)
        elif layout == "readonly_memmap":
            path = tmp_path / f"p4_{n}_{L}.bin"
            packed.tofile(path)
            arr = np.memmap(path, dtype=np.uint64, mode="r", shape=packed.shape)
        else:
            arr = _at_offset(packed, 16)
        gpu.set_msa(arr, L)
        if layout == "overwritten_after":
            arr[...] = np.uint64(0x0123456789ABCDEF)      # nothing may still be reading the host array
        _check_counts(gpu, n, u_ref, m_ref, what)
        del arr


def test_nj_300_tips(gpu, orc):
    from dipper_amd import capi
    rng = np.random.default_rng(300)
    seqs = _util.synth_alignment(rng, 300, 2000, invalid_frac=0.02)
    packed = capi.pack4_many(seqs)
    gpu.set_msa(packed, len(seqs[0]))
    gpu.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    D_gpu = gpu.matrix()
    res = gpu.nj_run()
    ref = orc.nj_run(np.tril(D_gpu, -1))
    D_orc = orc.msa_dist_lower(packed, len(seqs[0]), capi.DIST_JC)
    lo = np.tril_indices(300, -1)
    _util.assert_msa_dist(D_gpu[lo], D_orc[lo], capi.DIST_JC, "300 tips")
    assert res["iters"] == ref["iters"] == 298
    for k in ("merge_x", "merge_y", "bl_x", "bl_y"):
        assert np.array_equal(res[k], ref[k]), k
    assert res["last_d"] == ref["last_d"]
