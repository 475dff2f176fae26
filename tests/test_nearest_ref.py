"""Each sequence's K nearest neighbours without a GPU: the host restatement dpr_nearest_host (the reference of
tests/test_gpu_nearest.py) against an independent NumPy statement (np.lexsort on (column, distance) per row, tests/_nearest_ref.py),
as bits; refused arguments; the restatement under host sanitizers.

Nothing here has a tolerance: j and cnt are integers, d is the entry itself and is compared as uint64."""
import os
import subprocess

import numpy as np
import pytest

from tests import _nearest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [2, 3, 17, 130]


def ks_of(n):
    return sorted({k for k in (1, 3, n - 2, n - 1, n, 256) if 1 <= k <= 256})


def host(D, K):
    from dipper_amd import capi
    return capi.nearest_host(D, K)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(R.MATRICES))
def test_host_restatement_equals_the_numpy_statement(name, n):
    for K in ks_of(n):
        D = R.matrix(name, n, K)
        got, ref = host(D, K), R.nearest(D, K)
        R.same(got, ref)
        finite = np.isfinite(D) & ~np.eye(n, dtype=bool)
        assert np.array_equal(got["cnt"], np.minimum(finite.sum(axis=1), K))
        real = got["j"] >= 0
        assert np.array_equal(real, np.arange(K)[None, :] < got["cnt"][:, None])      # padding only behind the real places
        assert (got["d"].view(np.uint64)[~real] == R.PAD_BITS).all() and np.isfinite(got["d"][real]).all()
        assert not (got["j"] == np.arange(n)[:, None]).any()                           # never the row itself


def test_constant_matrix_names_the_smallest_columns():
    n, K = 130, 10
    got = host(R.constant(n), K)
    for i in (0, 1, 5, 9, 10, 11, 129):
        assert got["j"][i].tolist() == [c for c in range(n) if c != i][:K]


def test_signed_zeros_tie_by_column_and_keep_their_sign():
    n = 17
    D = R.signed_zero(n)
    got = host(D, n - 1)
    R.same(got, R.nearest(D, n - 1))
    row = got["d"][0][: got["cnt"][0]]
    cols = got["j"][0][: got["cnt"][0]]
    neg = int((D[0] < 0).sum())
    assert (row[:neg] < 0).all() and (np.diff(row) >= 0).all()                         # negative entries first
    zeros = cols[row == 0]
    assert {1, 2, n - 1} <= set(zeros.tolist()) and (np.diff(zeros) > 0).all()           # either zero: by column
    sign = {int(c): bool(np.signbit(v)) for c, v in zip(cols, row)}
    assert sign[1] is False and sign[2] is True and sign[n - 1] is True


def test_rows_without_and_with_few_finite_entries():
    n, K = 17, 3
    got = host(R.nonfinite(n, K), K)
    assert got["cnt"][1] == 0 and (got["j"][1] == -1).all()
    assert got["cnt"][2] == K - 1 and got["j"][2][K - 1] == -1 and got["cnt"][3] == K


def test_two_tips():
    for v, cnt in ((0.3, 1), (-0.0, 1), (np.nan, 0), (np.inf, 0), (-np.inf, 0)):
        D = np.array([[0.0, v], [v, 0.0]])
        got = host(D, 2)
        R.same(got, R.nearest(D, 2))
        assert got["cnt"].tolist() == [cnt, cnt] and got["j"][:, 0].tolist() == ([1, 0] if cnt else [-1, -1])


def test_bad_arguments_are_refused():
    from dipper_amd import capi
    D = R.noisy(10)
    for K in (0, 257, -1):
        with pytest.raises(capi.DipperError) as ei:
            host(D, K)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError) as ei:
        host(np.zeros((1, 1)), 1)      # n = 1
    assert ei.value.code == -1
    lib = capi.load_library()
    n, rows = capi._lower_rows(D)
    j, d, cnt = np.full(n, -5, dtype=np.int32), np.full(n, -5.0), np.full(n, -5, dtype=np.int32)
    pj, pd, pc, pr = (a.ctypes.data_as(t) for a, t in ((j, capi.c_i32p), (d, capi.c_f64p), (cnt, capi.c_i32p), (rows, capi.c_f64p)))
    for args in ((None, n, 1, pj, pd, pc), (pr, n, 1, None, pd, pc), (pr, n, 1, pj, None, pc), (pr, n, 1, pj, pd, None), (pr, 1, 1, pj, pd, pc)):
        assert lib.dpr_nearest_host(*args) == -1
    assert (j == -5).all() and (d == -5.0).all() and (cnt == -5).all()                    # nothing was written
    assert lib.dpr_nearest_host(pr, n, 1, pj, pd, pc) == 0 and (cnt == 1).all()


def test_host_side_under_address_and_ub_sanitizers():
    """the restatement is plain C++ in a header of its own: a driver with its own main, built with -fsanitize=address,undefined
    (`make -C dipper_amd/csrc nearest_asan`), runs ties, non-finite entries, signed zeros, K up to 256 and the refused arguments
    without a report"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "nearest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "dipper_amd", "bin", "nearest_check_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 48 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
