"""The tree fit without a GPU: the host restatement dpr_tree_fit_host (the reference of tests/test_gpu_fit.py) against the NumPy /
math.fsum reference of tests/_fit_ref.py; the three converters against the Newick text the command's own writers produce
(`dipper --dump-newick`, a GPU-free developer aid); the command's usage errors; the restatement under host sanitizers.

Bounds.  A sum of k terms added in ANY order lies within k * 2^-52 * sum|terms| of the exact sum (the first-order bound
(k - 1) u sum|terms| with u = 2^-53, doubled for the higher-order terms): derived, not tuned.  The reference's terms are the
library's bit for bit (the same IEEE operations in the same order), so nothing else enters."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import _fit_ref as R, _nonfinite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
SUMS = ("sum_d", "sum_p", "sum_dd", "sum_pp", "sum_dp", "ss", "wss")


@functools.lru_cache(maxsize=None)
def trees(n, seed=0):
    """name -> (parent, length) of the shapes every size is tested on (computed once per size, shared, never changed)"""
    from dipper_amd import capi
    rng = np.random.default_rng(1000 * n + seed)
    out = {}
    D = R.noisy_matrix(rng, n)
    nj = capi.nj_variant_host(0, D)
    out["nj"] = capi.tree_from_nj(nj["merge_x"], nj["merge_y"], nj["bl_x"], nj["bl_y"], nj["last_d"], n=n)
    out["caterpillar"] = R.caterpillar(n, rng)
    out["balanced"] = R.balanced(n, rng)
    up = capi.upgma_host(D, 0)
    out["upgma"] = capi.tree_from_upgma(up["merge_x"], up["merge_y"], up["height"])
    if n >= 3:
        out["multifurcating"] = R.multifurcating(n, rng)
    p, _ = R.balanced(n, rng)
    out["zero_negative"] = (p, R.lengths(rng, len(p), "zero_negative"))
    return out


def check_against_reference(D, parent, length, got):
    n = D.shape[0]
    ref = R.fit(D, R.Tree(n, parent, length))
    assert got["n"] == ref["n"] and got["skipped"] == ref["skipped"] and got["n_w"] == ref["n_w"]
    assert got["n"] + got["skipped"] == n * (n - 1) // 2
    for k in SUMS:
        bound = ref["terms_" + k] * 2.0 ** -52 * ref["abs_" + k]
        assert abs(got[k] - ref[k]) <= bound, (k, got[k], ref[k], bound)
    assert got["max_e"] == ref["max_e"] and tuple(got["worst"]) == ref["worst"]
    assert np.array_equal(got["taxon_pairs"], ref["taxon_pairs"])
    bound = ref["taxon_terms"] * 2.0 ** -52 * ref["taxon_ss"]
    assert (np.abs(got["taxon_ss"] - ref["taxon_ss"]) <= bound).all()
    # the derived figures from the library's own sums, recomputed here
    rms, rel, ev, cc = R.derived(got)
    for k, v in (("rms", rms), ("rms_rel", rel), ("explained", ev), ("cophenetic", cc)):
        assert (got[k] != got[k] and v != v) or abs(got[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, got[k], v)
    return ref


@pytest.mark.parametrize("n", [2, 3, 4, 5, 17, 65, 257])
def test_host_sums_against_fsum(n):
    from dipper_amd import capi
    D = R.noisy_matrix(np.random.default_rng(n), n)
    for name, (parent, length) in trees(n).items():
        got = capi.tree_fit_host(D, parent, length)
        ref = check_against_reference(D, parent, length, got)
        assert ref["skipped"] == 0, name


def test_depth_formula_against_path_sums():
    """the contract's P against the edges of each path added one at a time: within 4 (h + 2) 2^-53 (sum |len| on the two root paths),
    the bound of the recursive sums involved (a depth is a sum of at most h terms, the path sums likewise, P adds three more roundings)"""
    for n in (5, 65, 200):
        for name, (parent, length) in trees(n).items():
            t = R.Tree(n, parent, length)
            Pd = t.patristic_depth()
            Pp, absroot = t.patristic_paths()
            bound = 4 * (t.height + 2) * 2.0 ** -53 * (absroot[:, None] + absroot[None, :])
            assert (np.abs(Pd - Pp) <= bound).all(), (n, name)


def ultrametric(n, rng):
    """small integers times 2^-10 on a random rooted binary tree: D_ij = 2 * height of lca, heights rising towards the root"""
    parent, _ = R.balanced(n, rng)
    m = len(parent)
    h = np.zeros(m)
    for v in range(n, m):      # children are numbered before their parents
        kids = np.flatnonzero(parent == v)
        h[v] = h[kids].max() + int(rng.integers(1, 6)) * 2.0 ** -10
    t = R.Tree(n, parent, np.zeros(m))
    D = 2.0 * h[t.lca]
    D[np.arange(n), np.arange(n)] = 0.0
    return D


def test_exact_case_on_the_host():
    """WPGMA of an ultrametric matrix of small dyadic numbers averages equal values: every height, depth and path length is exact"""
    from dipper_amd import capi
    n = 40
    D = ultrametric(n, np.random.default_rng(4))
    up = capi.upgma_host(D, 1)
    parent, length = capi.tree_from_upgma(up["merge_x"], up["merge_y"], up["height"])
    assert np.array_equal(R.Tree(n, parent, length).patristic_depth(), D)      # the construction is exact
    got = capi.tree_fit_host(D, parent, length)
    assert got["n"] == n * (n - 1) // 2 and got["ss"] == 0.0 and got["max_e"] == 0.0 and got["explained"] == 1.0
    assert (got["taxon_ss"] == 0.0).all() and abs(got["cophenetic"] - 1.0) <= 2.0 ** -50
    assert got["rms"] == 0.0 and got["rms_rel"] == 0.0


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["nan_pair", "inf_few", "nan_and_inf", "inf_row"])
def test_skipped_pairs_on_the_host(which):
    from dipper_amd import capi
    n = 100
    name, D = _nonfinite.matrices(n, 11)[which]
    parent, length = R.balanced(n, np.random.default_rng(5))
    length = length.copy()
    length[7] = np.inf                         # tip 7 hangs on an infinite edge: its n - 1 pairs are skipped
    got = capi.tree_fit_host(D, parent, length)
    ref = check_against_reference(D, parent, length, got)
    bad = ~np.isfinite(D)
    bad[7, :] = bad[:, 7] = True
    assert ref["skipped"] == int(np.tril(bad, -1).sum()) and got["taxon_pairs"][7] == 0 and got["taxon_ss"][7] == 0.0


def test_all_skipped_and_zero_distances():
    from dipper_amd import capi
    n = 9
    parent, length = R.caterpillar(n, np.random.default_rng(6))
    got = capi.tree_fit_host(np.full((n, n), np.nan), parent, length)
    assert got["n"] == 0 and got["skipped"] == n * (n - 1) // 2 and tuple(got["worst"]) == (-1, -1) and got["max_e"] == 0.0
    assert all(math.isnan(got[k]) for k in ("rms", "rms_rel", "explained", "cophenetic")) and got["ss"] == 0.0
    # D = 0 pairs are counted everywhere but in WSS
    D = R.noisy_matrix(np.random.default_rng(7), n)
    D[3, 1] = D[1, 3] = 0.0
    D[8, 0] = D[0, 8] = -0.0
    got = capi.tree_fit_host(D, parent, length)
    assert got["n"] == n * (n - 1) // 2 and got["n_w"] == got["n"] - 2
    check_against_reference(D, parent, length, got)


def test_malformed_trees_are_refused():
    from dipper_amd import capi
    n = 6
    D = R.noisy_matrix(np.random.default_rng(8), n)
    parent, length = R.balanced(n, np.random.default_rng(8))
    cases = {}
    p = parent.copy(); p[-1] = n; cases["no root (a cycle through it)"] = p
    p = parent.copy(); p[n] = -1; cases["two roots"] = p
    p = parent.copy(); p[0] = 1; cases["a tip with a child"] = p
    p = parent.copy(); p[0] = len(parent); cases["a parent out of range"] = p
    p = parent.copy(); a, b = n, int(parent[n]); p[a], p[b] = b, a; cases["a cycle off the tree"] = p
    p = parent.copy(); p[0] = p[1] = int(parent[n]); cases["an internal node without children"] = p
    for name, p in cases.items():
        with pytest.raises(capi.DipperError) as ei:
            capi.tree_fit_host(D, p, length)
        assert ei.value.code == -1 and "not a tree" in str(ei.value), name
    star = np.array([n] * n + [-1], dtype=np.int32)              # m = n + 1, the smallest
    assert capi.tree_fit_host(D, star, np.ones(n + 1))["n"] == n * (n - 1) // 2
    with pytest.raises(capi.DipperError):                        # m = 2n: one node too many
        capi.tree_fit_host(D, np.append(parent, 0).astype(np.int32), np.append(length, 1.0))
    assert capi.tree_fit_host(D, parent, length)["n"] == n * (n - 1) // 2


# ---- converters against the command's Newick writers -----------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def half_last_digit(v):
    """half a unit of the sixth significant digit of every entry (the writers print %g with precision 6)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    out = np.zeros_like(v)
    nz = v > 0
    out[nz] = 0.5 * 10.0 ** (np.floor(np.log10(v[nz])) - 5)
    return out


def check_converter(tmp_path, n, text, parent, length):
    log = tmp_path / "log.txt"
    log.write_text(text)
    r = run("--dump-newick", str(log))
    assert r.returncode == 0, r.stderr
    names, P, _ = R.newick_patristic(r.stdout)
    assert sorted(names) == sorted(f"t{i}" for i in range(n)) and len(parent) == len(length) == 2 * n - 1
    at = [names.index(f"t{i}") for i in range(n)]
    P = P[np.ix_(at, at)]
    mine, absroot = R.Tree(n, parent, length).patristic_paths()
    tol, _ = R.Tree(n, parent, half_last_digit(length)).patristic_paths()      # half a printed digit per edge on the path
    slack = 2.0 ** -40 * (absroot[:, None] + absroot[None, :])                  # the two summations themselves
    assert (np.abs(P - mine) <= tol + slack).all(), np.abs(P - mine).max()


def hx(v):
    return float(v).hex()


@pytest.mark.parametrize("n", [2, 3, 9, 40])
def test_converters_against_the_commands_newick(tmp_path, n):
    from dipper_amd import capi
    D = R.noisy_matrix(np.random.default_rng(60 + n), n)
    # NJ log
    if n >= 3:
        nj = capi.nj_variant_host(0, D)
    else:
        nj = dict(merge_x=[], merge_y=[], bl_x=[], bl_y=[], last_d=0.37)
    text = f"nj {n} {hx(nj['last_d'])}\n" + "".join(
        f"{x} {y} {hx(a)} {hx(b)}\n" for x, y, a, b in zip(nj["merge_x"], nj["merge_y"], nj["bl_x"], nj["bl_y"]))
    check_converter(tmp_path, n, text, *capi.tree_from_nj(nj["merge_x"], nj["merge_y"], nj["bl_x"], nj["bl_y"], nj["last_d"], n=n))
    # UPGMA log
    up = capi.upgma_host(D, 0)
    text = f"upgma {n}\n" + "".join(f"{x} {y} {hx(h)}\n" for x, y, h in zip(up["merge_x"], up["merge_y"], up["height"]))
    check_converter(tmp_path, n, text, *capi.tree_from_upgma(up["merge_x"], up["merge_y"], up["height"]))
    # BME outputs
    if n >= 3:
        b = capi.bme_nni_host(D, nj["merge_x"], nj["merge_y"], 2)
        kids, top, ln = b["kids"], int(b["top"]), b["len"]
    else:
        kids, top, ln = np.zeros(0, dtype=np.int32), 0, np.array([0.4, 0.0])
    text = f"kids {n} {top}\n" + " ".join(str(int(k)) for k in np.asarray(kids).reshape(-1)) + "\n" + " ".join(hx(v) for v in ln) + "\n"
    check_converter(tmp_path, n, text, *capi.tree_from_kids(kids, top, ln))


def test_converters_refuse_what_is_no_log():
    from dipper_amd import capi
    with pytest.raises(capi.DipperError):
        capi.tree_from_nj([0, 5], [1, 6], [0.1, 0.1], [0.1, 0.1], 0.2)         # slot 5 of 3 live ones
    with pytest.raises(capi.DipperError):
        capi.tree_from_upgma([0, 0, 0], [1, 1, 3], [0.1, 0.2, 0.3])
    with pytest.raises(capi.DipperError):
        capi.tree_from_kids([0, 0, 4, 2], 5, np.ones(6))                        # tip 0 twice


# ---- the command's usage errors --------------------------------------------------------------------------------------------------
def test_help_text_names_the_options():
    r = run("--help")
    assert r.returncode == 0 and "--fit " in r.stderr and "--fit-taxa arg" in r.stderr and "explained" in r.stderr and "cophenetic" in r.stderr


@pytest.mark.parametrize("extra,word", [
    (("-m", "1"), "-m 2"), (("-m", "3"), "-m 2"), (("--add", "-t", "x.nwk"), "--add"), (("-o", "d"), "-o t"), (("-o", "j"), "-o t"),
    (("--bootstrap", "3"), "--bootstrap"), (("--gpus", "2"), "one GPU"), (("--devices", "0,0"), "one GPU"),
    (("--rank", "0", "--world", "2", "--rendezvous", "/r"), "one GPU"),
])
def test_usage_errors_before_any_gpu_call(tmp_path, extra, word):
    """decided from the arguments alone: the input file does not even exist"""
    r = run("-i", "m", "-I", str(tmp_path / "none.fa"), "-O", str(tmp_path / "o.nwk"), "--fit", "--fit-taxa", str(tmp_path / "t.tsv"), *extra)
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and word in head and "--fit" in head, r.stderr[:400]
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "t.tsv").exists()


def test_fit_taxa_needs_fit(tmp_path):
    r = run("-i", "m", "-I", str(tmp_path / "none.fa"), "-O", str(tmp_path / "o.nwk"), "--fit-taxa", str(tmp_path / "t.tsv"))
    head = r.stderr.split("DIPPER Command Line Arguments")[0]
    assert r.returncode == 1 and "--fit-taxa needs --fit" in head
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "t.tsv").exists()


def test_host_side_under_address_and_ub_sanitizers():
    """the restatement and the converters are plain C++ in a header of their own: a driver with its own main, built with
    -fsanitize=address,undefined (`make -C dipper_amd/csrc fit_asan`), runs every tree shape, non-finite and zero entries and refused
    inputs without a report"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dipper_amd", "csrc"), "fit_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")
    q = subprocess.run([os.path.join(ROOT, "dipper_amd", "bin", "fit_check_asan")], capture_output=True, text=True, env=env, timeout=120)
    assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (q.returncode, q.stderr[-2000:])
    lines = q.stdout.strip().split("\n")
    assert len(lines) == 36 and all(ln.endswith(" ok") for ln in lines), q.stdout[-1500:]
