"""The pairs within a distance threshold without a GPU: the host restatement dpr_pairs_within_host (the reference of
tests/test_gpu_pairs.py) against NumPy and a dict union-find (tests/_pairs_ref.py), as bits; the command's usage errors and help text;
the restatement under host sanitizers.

Nothing here has a tolerance: a pair is kept or not by one fp64 comparison, d is the entry itself, the labels are integers."""
import os
import subprocess

import numpy as np
import pytest

from tests import _pairs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


def host(D, T):
    from dipper_amd import capi
    return capi.pairs_within_host(D, T)


@pytest.mark.parametrize("n", [2, 3, 64, 65, 300])
def test_noisy_matrices_with_nonfinite_entries(n):
    D = R.nonfinite(n)
    vals = D[np.tril_indices(n, -1)]
    finite = np.sort(vals[np.isfinite(vals)])
    for T in {0.0, float(finite[0]) if len(finite) else 0.5, float(finite[len(finite) // 10]) if len(finite) else 0.5, 0.5, 1.0, R.DBL_MAX}:
        ref = R.within(D, T)
        R.same(host(D, T), ref)
        assert not np.isnan(ref["d"]).any() and not (ref["d"] == np.inf).any()


@pytest.mark.parametrize("name", ["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_the_nonfinite_matrices_of_the_nj_tests(name):
    D = dict(R.nonfinite_named(90))[name]
    for T in (0.3, R.DBL_MAX):
        R.same(host(D, T), R.within(D, T))
    ref = R.within(D, R.DBL_MAX)
    assert ref["stats"]["pairs"] == int(np.isfinite(D[np.tril_indices(90, -1)]).sum())      # every finite pair, no other


def test_threshold_equal_to_an_entry_keeps_it():
    """`<=`, not `<`: with T exactly an entry that entry is within; just below T it is not"""
    D = R.noisy(120)
    T = float(D[77, 5])
    at, below = host(D, T), host(D, np.nextafter(T, 0.0))
    R.same(at, R.within(D, T))
    R.same(below, R.within(D, np.nextafter(T, 0.0)))
    ties = int((D[np.tril_indices(120, -1)] == T).sum())
    assert ties >= 1 and at["stats"]["pairs"] - below["stats"]["pairs"] == ties
    assert (77, 5) in set(zip(at["i"].tolist(), at["j"].tolist())) and (77, 5) not in set(zip(below["i"].tolist(), below["j"].tolist()))


def test_zero_threshold_names_identical_rows():
    D = R.noisy(50).copy()
    D[31, :] = D[8, :]
    D[:, 31] = D[:, 8]
    D[31, 8] = D[8, 31] = 0.0
    D[31, 31] = 0.0
    got = host(D, 0.0)
    R.same(got, R.within(D, 0.0))
    assert list(zip(got["i"].tolist(), got["j"].tolist())) == [(31, 8)] and got["label"][31] == 8 and got["stats"]["components"] == 49


def test_threshold_below_every_entry():
    D = R.noisy(40)
    got = host(D, 0.01)
    R.same(got, R.within(D, 0.01))
    assert got["stats"] == dict(pairs=0, components=40, largest=1, singletons=40) and np.array_equal(got["label"], np.arange(40))


def test_dbl_max_keeps_every_finite_pair():
    D = R.noisy(70)
    got = host(D, R.DBL_MAX)
    R.same(got, R.within(D, R.DBL_MAX))
    assert got["stats"]["pairs"] == 70 * 69 // 2 and got["stats"]["components"] == 1 and (got["label"] == 0).all()


def test_two_tips():
    for v, T, k in ((0.3, 0.3, 1), (0.3, 0.29, 0), (np.nan, R.DBL_MAX, 0), (np.inf, R.DBL_MAX, 0), (-np.inf, 0.0, 1)):
        D = np.array([[0.0, v], [v, 0.0]])
        got = host(D, T)
        R.same(got, R.within(D, T))
        assert got["stats"]["pairs"] == k and got["label"].tolist() == ([0, 0] if k else [0, 1])


@pytest.mark.parametrize("n", [6, 65, 200])
def test_component_shapes(n):
    from dipper_amd import capi
    for name, (D, T) in R.shapes(n).items():
        got = host(D, T)
        ref = R.within(D, T)
        R.same(got, ref)
        want = dict(path=1, star=1, cliques=1, singletons=n)[name]
        assert got["stats"]["components"] == want, name
        assert np.array_equal(capi.pairs_summary_host(got["label"])["rank"], R.ranks(ref["label"]))


def test_bad_arguments_are_refused():
    from dipper_amd import capi
    D = R.noisy(10)
    for T in (np.nan, np.inf, -np.inf, -1e-300):
        with pytest.raises(capi.DipperError) as ei:
            host(D, T)
        assert ei.value.code == -1
    with pytest.raises(capi.DipperError):
        capi.pairs_summary_host(np.array([1, 1], dtype=np.int32))      # a label above its tip


# ---- the command line ---------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


USAGE = [
    ("-o p", "-o p needs a distance threshold (--within T)"),
    ("--within 0.1", "--within needs the pair output (-o p)"),
    ("--clusters {tmp}/c.tsv", "--clusters needs the pair output (-o p)"),
    ("-o d --within 0.1", "--within needs the pair output (-o p)"),
    ("-o p --within x", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within -0.5", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within inf", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within nan", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within 1e999", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within 0.1x", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within=", "--within: the threshold must be a finite decimal >= 0 (0.015)"),
    ("-o p --within 0.1 --clusters=", "--clusters: a file name"),
    ("-o p --within 0.1 --clusters {tmp}/o.tsv", "--clusters: the file must differ from the output file (-O)"),
    ("-o p --within 0.1 --add -t {tmp}/t.nwk", "-o p is not supported with --add or -t"),
    ("-o p --within 0.1 -t {tmp}/t.nwk", "-o p is not supported with --add or -t"),
    ("-o p --within 0.1 --bootstrap 3", "--bootstrap needs tree output (-o t)"),
    ("-o p --within 0.1 --bionj", "--bionj needs tree output (-o t)"),
    ("-o p --within 0.1 --nni 1", "--nni needs tree output (-o t)"),
    ("-o p --within 0.1 --spr 1", "--spr needs tree output (-o t)"),
    ("-o p --within 0.1 --upgma", "--upgma needs tree output (-o t)"),
    ("-o p --within 0.1 --wpgma", "--wpgma needs tree output (-o t)"),
    ("-o p --within 0.1 --fit", "--fit needs tree output (-o t)"),
    ("-o p --within 0.1 --gpus 2", "-o p runs on one GPU"),
    ("-o p --within 0.1 --devices 0,0", "-o p runs on one GPU"),
    ("-o p --within 0.1 --rank 0 --world 2 --rendezvous x", "-o p runs on one GPU"),
]


@pytest.mark.parametrize("args,message", USAGE, ids=[a for a, _ in USAGE])
def test_usage_errors_are_decided_before_any_file_or_gpu(tmp_path, args, message):
    (tmp_path / "t.nwk").write_text("((A:0.1,B:0.2):0.05,C:0.3);\n")
    r = run("-i", "m", "-I", str(tmp_path / "missing.fa"), "-O", str(tmp_path / "o.tsv"), *args.replace("{tmp}", str(tmp_path)).split())
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and "DIPPER Command Line Arguments" in r.stderr and message in head, (r.returncode, head)
    assert sorted(os.listdir(tmp_path)) == ["t.nwk"]


@pytest.mark.parametrize("args", ["-o p --within 0", "-o p --within 0.015 --clusters {tmp}/c.tsv", "-o p --within 1e-3 -i r -k 12", "-o p --within .5 -i d",
                                  "-o p --within 2 --protein -d 8", "-o p --within 0.1 --site-coverage 0.9", "-o p --within 0.1 --devices 0"])
def test_valid_combinations_reach_the_reader(tmp_path, args):
    r = run("-i", "m", "-I", str(tmp_path / "missing.fa"), "-O", str(tmp_path / "o.tsv"), *args.replace("{tmp}", str(tmp_path)).split())
    assert r.returncode == 1 and "DIPPER Command Line Arguments" not in r.stderr and "missing.fa" in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_help_names_the_options():
    r = run("-h")
    assert r.returncode == 0
    for word in ("p - the pairs of sequences within a distance threshold", "--within arg", "--clusters arg"):
        assert word in r.stderr, word


def test_host_side_under_address_and_ub_sanitizers():
    """the restatement is plain C++ in a header of its own: a driver with its own main, built with -fsanitize=address,undefined
    (`make -C dipper_amd/csrc pairs_asan`), runs non-finite entries, every capacity and the refused arguments without a report"""
    exe = os.path.join(ROOT, "dipper_amd", "bin", "pairs_check_asan")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "pairs_asan"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 28 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
