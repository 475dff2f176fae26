"""UPGMA / WPGMA (dpr_upgma_run) on one GPU.  One JSON line per call on stdout.

    python profiles/upgma/upgma_bench.py --tips 20000 --sites 1000               # the loop: us / iteration, rows rescanned / iteration,
                                                                                 # beside the NJ loop of the same matrix and the cost of
                                                                                 # a naive full scan at the probed bandwidth
    python profiles/upgma/upgma_bench.py --tips 30000 --sites 10000 --flagship --command    # the bench's alignment; + `dipper --upgma` from FASTA

Inputs come from tools/bin/gen_synth (--model gtr+g+i), seeded; nothing is read from outside the repository."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _util  # noqa: E402

BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def loop(d, dist_type, linkage):
    d.dist_matrix(capi.SRC_MSA, dist_type)
    t0 = time.perf_counter()
    res = d.upgma(linkage)
    wall = 1e3 * (time.perf_counter() - t0)
    st, ms = d.upgma_stats(), d.upgma_timing()
    it = len(res["merge_x"])
    return dict(loop_ms=ms, call_wall_ms=wall, us_per_iteration=1e3 * ms / it, rows_rescanned=st["rescanned"],
                rows_rescanned_per_iteration=st["rescanned"] / it, launches=st["launches"], bytes_held=st["bytes"], root_height=float(res["height"][-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=20000)
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--mean-bl", type=float, default=2e-4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dist", type=int, default=capi.DIST_JC)
    ap.add_argument("--flagship", action="store_true", help="the bench's alignment: mean branch 2e-5, inherited deletions as gaps")
    ap.add_argument("--command", action="store_true")
    a = ap.parse_args()
    mean = 2e-5 if a.flagship else a.mean_bl
    extra = ("--model", "gtr+g+i", "--indel-gaps") if a.flagship else ("--model", "gtr+g+i")
    with tempfile.TemporaryDirectory() as tmp:
        inp = _util.gen_synth(tmp, "in", a.tips, a.sites, a.seed, mean, mean / 10, mean * 10, fasta=a.command, extra=extra)
        d = dipper_amd.Dipper(0)
        try:
            d.set_msa(inp["packed4"], a.sites)
            rec = {"tips": a.tips, "sites": a.sites, "mean_bl": mean, "dist_type": a.dist, "device": d.device_name()}
            d.dist_matrix(capi.SRC_MSA, a.dist)
            d.nj_run()                                                           # warm-up of the NJ loop (graphs), then the timed one
            d.dist_matrix(capi.SRC_MSA, a.dist)
            res = d.nj_run()
            rec["nj_ms"] = d.timing()[1]
            rec["nj_us_per_iteration"] = 1e3 * rec["nj_ms"] / res["iters"]
            loop(d, a.dist, 0)                                                   # warm-up: allocation, first launches
            rec["upgma"] = loop(d, a.dist, 0)
            rec["wpgma"] = loop(d, a.dist, 1)
            ms = C.c_float()
            nbytes = 8 * a.tips * a.tips
            assert d.L.dpr_bw_probe(d.h, nbytes, 0, 2048, 10, C.byref(ms)) == 0
            rec["bw_probe_gbs"] = nbytes / ms.value / 1e6
            # a naive iteration scans the m x m matrix of the moment: sum over m of 8 m^2 bytes = 8 n^3 / 3
            rec["naive_full_scan_s"] = 8.0 * a.tips ** 3 / 3.0 / (rec["bw_probe_gbs"] * 1e9)
            rec["naive_first_iteration_us"] = ms.value * 1e3
        finally:
            d.close()
        if a.command:
            for name, extra_args in (("plain", ()), ("upgma", ("--upgma",))):
                walls = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    r = subprocess.run([BIN, "-i", "m", "-I", inp["fasta"], "-O", os.path.join(tmp, "o.nwk"), "-m", "2", "-d", str(a.dist), *extra_args],
                                       capture_output=True, text=True, timeout=600)
                    assert r.returncode == 0, r.stderr[-2000:]
                    walls.append(time.perf_counter() - t0)
                rec["command_" + name + "_s"] = walls
                rec["command_" + name + "_tree_created_ms"] = [ln for ln in r.stderr.split("\n") if ln.startswith("Tree Created in:")][0]
                if extra_args:
                    rec["command_line"] = [ln for ln in r.stderr.split("\n") if ln.startswith("UPGMA:")][0]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
