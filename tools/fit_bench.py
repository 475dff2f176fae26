"""Time of the tree fit (dpr_tree_fit) on one GPU, beside the NJ row-sum kernel over the same fresh matrix in the same process.
One JSON line per input on stdout (and appended to --out).

    python tools/fit_bench.py --out profiles/fit/fit_bench.jsonl

Two inputs, both from tools/bin/gen_synth (seeded; nothing is read from outside the repository):
  30 000 x 10 000   the bench's alignment (gtr+g+i, mean branch 2e-5, inherited deletions as gaps), JC distances, its NJ tree;
  100 000 x 400     a matrix of 100 000 tips (80 GB, streaming NJ plan: one copy), a random-join tree -- an NJ run of that size is
                    not part of a measurement of the fit.
The row-sum kernel reads every row of the square matrix once (8 n^2 bytes); the fit reads the lower triangle in a row pass and again
in a column pass (8 n^2 bytes together) plus its lookups, so the ratio of the two times says whether the lookups are hidden.
No torch.  Every GPU step runs under a time limit of its own; a step that overruns ends the process, nothing is started after it."""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _util  # noqa: E402


class step:
    """a GPU step under its own time limit: overrun = one line on stderr and the end of the process (status 124)"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def late(signum, frame):
            sys.stderr.write(f"[fit_bench] step '{self.what}' passed its limit of {self.seconds} s: stopping\n")
            sys.stderr.flush()
            os._exit(124)
        signal.signal(signal.SIGALRM, late)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)
        sys.stderr.write(f"[fit_bench] {self.what}: {time.perf_counter() - self.t0:.2f} s\n")
        return False


def random_join_tree(n, seed):
    """(parent, length) of a random merge log: two live slots joined per step, the NJ log's bookkeeping"""
    rng = np.random.default_rng(seed)
    mx, my = np.zeros(n - 2, dtype=np.int32), np.zeros(n - 2, dtype=np.int32)
    u, w = rng.random(n - 2), rng.random(n - 2)
    for it in range(n - 2):
        live = n - it
        x, y = int(u[it] * live), int(w[it] * (live - 1))
        y += y >= x
        mx[it], my[it] = min(x, y), max(x, y)
    return capi.tree_from_nj(mx, my, 1e-3 * (0.1 + rng.random(n - 2)), 1e-3 * (0.1 + rng.random(n - 2)), 1e-3, n=n)


def measure(d, tree, reps):
    d.set_fit_compare(True)
    with step("fit, warm-up call (allocation, first launches)", 120):
        t0 = time.perf_counter()
        res = d.tree_fit(*tree)
        first_wall = 1e3 * (time.perf_counter() - t0)
    fit_ms, row_ms, wall_ms, passes = [], [], [], []
    for _ in range(reps):
        with step("fit, timed call", 120):
            t0 = time.perf_counter()
            d.tree_fit(*tree)
            wall_ms.append(1e3 * (time.perf_counter() - t0))
        a, b = d.fit_timing()
        fit_ms.append(a)
        row_ms.append(b)
        passes.append(d.fit_pass_timing())
    st = d.fit_stats()
    n = len(res["taxon_ss"])
    best_fit, best_row = min(fit_ms), min(row_ms)
    return dict(fit_kernels_ms=fit_ms, row_pass_ms=[p[0] for p in passes], column_pass_ms=[p[1] for p in passes], nj_row_sums_ms=row_ms, ratio_best=best_fit / best_row, call_wall_ms=wall_ms, first_call_wall_ms=first_wall,
                matrix_bytes=8 * n * n, fit_gb_per_s=8e-6 * n * n / best_fit, row_sums_gb_per_s=8e-6 * n * n / best_row,
                table_levels=st["levels"], bytes_held=st["bytes"], pairs=res["n"], skipped=res["skipped"], rms=res["rms"],
                explained_variance=res["explained"], cophenetic=res["cophenetic"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--big-tips", type=int, default=100000, help="0: skip the second input")
    ap.add_argument("--big-sites", type=int, default=400)
    a = ap.parse_args()
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        d = dipper_amd.Dipper(0)
        try:
            mean = 2e-5
            inp = _util.gen_synth(tmp, "a", a.tips, a.sites, 1, mean, mean / 10, mean * 10, extra=("--model", "gtr+g+i", "--indel-gaps"))
            rec = {"input": "bench alignment, JC, NJ tree", "tips": a.tips, "sites": a.sites, "device": d.device_name()}
            with step("upload and distances", 120):
                d.set_msa(inp["packed4"], a.sites)
                d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            with step("NJ tree", 300):
                nj = d.nj_run()
            tree = capi.tree_from_nj(nj["merge_x"], nj["merge_y"], nj["bl_x"], nj["bl_y"], nj["last_d"], n=a.tips)
            for mode, layout in ((0, "slot space (streaming NJ plan)"), (1, "position space (pruned NJ plan)")):
                d.set_nj_mode(mode)
                with step("distances again", 120):
                    d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                rec2 = dict(rec, matrix_layout=layout)
                rec2.update(measure(d, tree, a.reps))
                recs.append(rec2)
                print(json.dumps(rec2), flush=True)
        finally:
            d.close()
        if a.big_tips:
            d = dipper_amd.Dipper(0)
            try:
                mean = 2e-4
                inp = _util.gen_synth(tmp, "b", a.big_tips, a.big_sites, 2, mean, mean / 10, mean * 10, extra=("--model", "gtr+g+i"))
                rec = {"input": "synthetic alignment, JC, random-join tree", "tips": a.big_tips, "sites": a.big_sites, "device": d.device_name(),
                       "matrix_layout": "slot space (streaming NJ plan)"}
                d.set_nj_mode(0)      # the streaming plan keeps one copy of the matrix
                with step("upload and distances", 300):
                    d.set_msa(inp["packed4"], a.big_sites)
                    d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                tree = random_join_tree(a.big_tips, 3)
                rec.update(measure(d, tree, a.reps))
            except capi.DipperError as e:      # (a device without room for the matrix: the record says so)
                rec["error"] = str(e)
            recs.append(rec)
            try:
                print(json.dumps(rec), flush=True)
            finally:
                d.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
