"""CPU tests of the jplace output (`dipper --add -t ... -o j`): the help text, the usage errors that the arguments alone decide
(no input read, no GPU touched, no output file), the refusals that keep their wording, and the test helpers of tests/_jplace.py
(backbone generator, importer arrays, edge numbering of a jplace tree string, the bootstrap tally)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _jplace, _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
HOST = os.path.join(ROOT, "dipper_amd", "host")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:exitcode=66:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=66")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        import __graft_entry__ as g
        g.build()


@pytest.fixture(scope="module")
def asan_bin():
    """the command built with AddressSanitizer + UBSan (`make -C dipper_amd/host asan`; host code only)"""
    r = subprocess.run(["make", "-C", HOST, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(ROOT, "dipper_amd", "bin", "dipper_asan")


def run(binary, *args):
    r = subprocess.run([binary, *args], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=120)
    assert r.returncode != 66 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r


def test_help_lists_jplace():
    r = run(BIN, "-h")
    assert r.returncode == 0
    assert "j - placements in jplace format" in r.stderr


USAGE = [
    (["-i", "m", "-o", "j"], "-o j needs --add"),
    (["-i", "d", "-o", "j", "--add", "-t", "x.nwk"], "-o j needs aligned or unaligned sequences"),
    (["-i", "r", "-o", "j", "--add", "-t", "x.nwk", "--bootstrap", "5"], "--bootstrap with -o j needs aligned sequences"),
    (["-i", "m", "-o", "j", "--add", "-t", "x.nwk", "--bootstrap", "5", "--bootstrap-metric", "tbe"], "--bootstrap-metric does not apply to -o j"),
    (["-i", "m", "-o", "j", "--add", "-t", "x.nwk", "--bootstrap", "5", "--bootstrap-taxa", "f"], "--bootstrap-taxa does not apply to -o j"),
    (["-i", "m", "-o", "j", "--add", "-t", "x.nwk", "--bootstrap", "0"], "whole number >= 1"),
    (["-i", "m", "-o", "j", "--add", "-t", "x.nwk", "--bootstrap-seed", "3"], "--bootstrap-seed needs --bootstrap"),
    # the refusals that were there before keep their wording
    (["-i", "m", "--bootstrap", "5", "--add", "-t", "x.nwk"], "--bootstrap is not supported with --add"),
    (["-i", "m", "--bootstrap", "5", "-o", "d"], "--bootstrap needs tree output (-o t)"),
    (["-i", "m", "--add"], "Backbone tree (--input-tree/-t) is required with --add option"),
]


@pytest.mark.parametrize("sanitized", [False, True])
@pytest.mark.parametrize("extra,msg", USAGE)
def test_usage_errors_need_no_device(tmp_path, asan_bin, sanitized, extra, msg):
    p = tmp_path / "a.fa"
    p.write_text(">a\nACGT\n>b\nACGA\n>c\nACCA\n>d\nTCGA\n")
    r = run(asan_bin if sanitized else BIN, "-I", str(p), "-O", str(tmp_path / "o.jplace"), *extra)
    assert r.returncode == 1, r.stderr
    first = r.stderr.splitlines()[0]
    assert first.startswith("\033[31m") and msg in first, r.stderr[:400]      # (the help that follows is not the message)
    assert "Gpu_ERROR" not in r.stderr and not (tmp_path / "o.jplace").exists()


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["caterpillar", "balanced", "random"])
@pytest.mark.parametrize("m", [2, 3, 4, 6, 40, 300])
def test_backbone_arrays_are_the_importers(orc, kind, m):
    """edge k = the k-th non-root node in post-order owns slot 2k (child to parent) and 2k + 1; internal ids start at n, the
    root is n; exactly one slot of every edge is eligible (belong >= e)"""
    rng = np.random.default_rng(m)
    nwk = _jplace.random_backbone(rng, m, kind)
    n = m + 5
    st, names = _jplace.backbone_arrays(orc, nwk, n)
    assert names == ["B%d" % i for i in range(m)]
    lim = 4 * m - 4
    e, belong, ln = st["e"], st["belong"], st["len"]
    assert np.all(e[:lim] >= 0) and np.all(belong[:lim] >= 0) and np.all(e[lim:] == -1)
    assert np.array_equal(e[0:lim:2], belong[1:lim:2]) and np.array_equal(e[1:lim:2], belong[0:lim:2])
    assert np.array_equal(ln[0:lim:2], ln[1:lim:2])
    assert np.all((belong[0:lim:2] >= e[0:lim:2]) != (belong[1:lim:2] >= e[1:lim:2]))
    assert set(belong[:lim]) == set(range(m)) | set(range(n, n + m - 1))
    assert n not in set(belong[0:lim:2])                                         # the root is nobody's child
    if m >= 40:
        assert np.count_nonzero(ln[0:lim:2] == 0.0) >= 2                         # some zero-length edges
    # the tree the arrays describe is the text's: same leaf sets below the edges, in post-order
    kids, length, name, root = _util.parse_newick(nwk)
    _, below, labels, _ = _jplace.jplace_edges(_with_labels(nwk))
    assert labels == list(range(2 * m - 2))
    for k in range(2 * m - 2):
        assert _jplace.leaves_below_slot(st, 2 * k, names) == below[k]
        assert _jplace.leaves_below_slot(st, 2 * k + 1, names) == below[k]


def _with_labels(nwk):
    """`{k}` behind every branch length, k counting from 0 in the order of the text"""
    out, k, i = [], 0, 0
    while i < len(nwk):
        out.append(nwk[i])
        if nwk[i] == ":":
            j = i + 1
            while nwk[j] not in ",();":
                j += 1
            out.append(nwk[i + 1:j] + "{%d}" % k)
            k += 1
            i = j
            continue
        i += 1
    return "".join(out)


def test_jplace_edges_reads_a_tree_string():
    plain, below, labels, texts = _jplace.jplace_edges("((a:0.1{0},b:0{1}):0.25{2},(c:1e-05{3},(d:2{4},e:3{5}):4{6}):5{7});")
    assert plain == "((a:0.1,b:0):0.25,(c:1e-05,(d:2,e:3):4):5);"
    assert labels == list(range(8))
    assert below[2] == {"a", "b"} and below[6] == {"d", "e"} and below[7] == {"c", "d", "e"} and below[3] == {"c"}
    assert texts[3] == "1e-05" and texts[7] == "5"


def test_tally_orders_rows():
    main = (4, 0.5, 0.25)
    reps = [(7, 0.1, 0.2), (4, 9.0, 9.0), (7, 0.3, 0.4), (2, 0.0, 0.0), (9, 1.0, 1.0)]
    assert _jplace.tally(main, reps) == [(7, 2, 0.1, 0.2), (4, 1, 0.5, 0.25), (2, 1, 0.0, 0.0), (9, 1, 1.0, 1.0)]
    # the main edge is listed even when no replicate chose it, after the edges with a count
    assert _jplace.tally(main, [(7, 0.1, 0.2)]) == [(7, 1, 0.1, 0.2), (4, 0, 0.5, 0.25)]
    assert _jplace.tally(main, []) == [(4, 0, 0.5, 0.25)]


def test_tally_leaves_out_placements_that_are_not_finite():
    inf, nan = float("inf"), float("nan")
    main = (4, 0.5, 0.25)
    assert _jplace.tally((4, nan, inf), [(7, 0.1, 0.2)]) == []                 # no main placement: no record, whatever the replicates say
    assert _jplace.tally(main, [(7, 0.1, 0.2), (0, nan, inf), (7, 0.3, 0.4)]) == [(7, 2, 0.1, 0.2), (4, 0, 0.5, 0.25)]
    assert _jplace.tally(main, [(0, nan, inf)] * 3) == [(4, 0, 0.5, 0.25)]
    assert _jplace.tally((0, 0.01, 0.0), []) == [(0, 0, 0.01, 0.0)]             # add = 0 on the lowest slot (NaN to everything) is finite


# ---- the writer (no GPU: --dump-jplace hands rows from a text file to writeJplace) -------------------------------------------------
TREE = "((a:0.1,b:0):0.25,(c:1e-05,(d:2,e:3):4):5);"


def _no_constant(name):
    raise AssertionError("not JSON: the bare token %s" % name)


def _write(tmp_path, binary, rows_text, *extra):
    (tmp_path / "t.nwk").write_text(TREE + "\n")
    (tmp_path / "rows.txt").write_text(rows_text)
    return run(binary, "-t", str(tmp_path / "t.nwk"), "--dump-jplace", str(tmp_path / "rows.txt"), *extra)


@pytest.mark.parametrize("sanitized", [False, True])
def test_writer_writes_finite_rows_and_skips_queries_without_rows(tmp_path, asan_bin, sanitized):
    r = _write(tmp_path, asan_bin if sanitized else BIN, "q0 1\n3 1 0.25 1e-300\nq1 0\nq2 2\n0 2 0 0.5\n7 1 1.7976931348623157e308 4.9406564584124654e-324\n",
               "--bootstrap", "3")
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout, parse_constant=_no_constant)
    assert [p["n"] for p in doc["placements"]] == [["q0"], ["q2"]]              # q1 has no rows: no record, and no stray comma
    assert doc["placements"][0]["p"] == [[3, 0, 1 / 3, 0.25, 1e-300]]
    assert doc["placements"][1]["p"] == [[0, 0, 2 / 3, 0.0, 0.5], [7, 0, 1 / 3, 1.7976931348623157e308, 5e-324]]
    only_empty = _write(tmp_path, BIN, "q0 0\nq1 0\n")
    assert only_empty.returncode == 0 and json.loads(only_empty.stdout, parse_constant=_no_constant)["placements"] == []


@pytest.mark.parametrize("sanitized", [False, True])
@pytest.mark.parametrize("distal,pendant", [("nan", "inf"), ("0.1", "inf"), ("nan", "0.1"), ("0.1", "-inf"), ("inf", "0.1"), ("0.1", "nan")])
def test_writer_refuses_nan_and_inf(tmp_path, asan_bin, sanitized, distal, pendant):
    """the writer is handed finite rows only (placeFixed); given anything else it writes nothing and fails, it never emits the
    tokens nan / inf"""
    r = _write(tmp_path, asan_bin if sanitized else BIN, "q0 1\n3 1 0.25 0.5\nq1 1\n2 1 %s %s\n" % (distal, pendant))
    assert r.returncode == 1 and "not finite" in r.stderr, r.stderr
    assert r.stdout == ""
