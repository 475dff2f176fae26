"""Measurements of the placement on a fixed backbone (`dipper --add -t BACKBONE -o j`), BASELINE configs[4]
shape: `queries` onto a backbone of `backbone` tips.

  python3 profiles/jplace_bench.py cli     [backbone 500000] [queries 50000] [sites 1000] [reps 3] [bootstrap 20]
      whole commands, arms alternated: --add (tree output) and -o j on the same input, `reps` times each, then one
      -o j --bootstrap N; wall time per run and the commands' own stderr lines (distances / scan split)
  python3 profiles/jplace_bench.py kernels [backbone 500000] [queries 50000] [sites 1000]
      prints the three commands to run under `rocprofv3 --kernel-trace --stats` one by one (program after `--`): the
      divide-and-conquer command that builds the backbone (dc_assign_scan_kernel), -o j with the scan whose reduce step
      evaluates the winner again (default) and with the scan that carries the position (DPR_PFIX_CARRY=1); with `--run DIR`
      it runs them itself, one profiler process after the other, and prints the rows of the scan / reduce kernels

The input is made once under /dev/shm (tools/bin/gen_synth, seeded) and removed at the end."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tests import _util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def make_input(tmp, m, nq, sites):
    inp = _util.gen_synth(tmp, "a", m + nq, sites, 10, 1e-3, 1e-4, 1e-2, fasta=True, shuffle=7)
    buf = np.memmap(inp["fasta"], dtype=np.uint8, mode="r")
    cut = int(np.flatnonzero(buf == ord(">"))[m])
    bb = os.path.join(tmp, "bb.fa")
    with open(bb, "wb") as f:
        f.write(buf[:cut].tobytes())
    del buf
    return inp["fasta"], bb


def lines(stderr, keys):
    return {k: l.strip() for l in stderr.splitlines() for k in keys if k in l}


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "cli"
    rest = [a for a in sys.argv[2:] if not a.startswith("--")]
    run_dir = sys.argv[sys.argv.index("--run") + 1] if "--run" in sys.argv else None
    if run_dir:
        rest = [a for a in rest if a != run_dir]
    m = int(rest[0]) if len(rest) > 0 else 500000
    nq = int(rest[1]) if len(rest) > 1 else 50000
    sites = int(rest[2]) if len(rest) > 2 else 1000
    reps = int(rest[3]) if len(rest) > 3 else 3
    boot = int(rest[4]) if len(rest) > 4 else 20
    env = dict(os.environ, DPR_HOST_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="jplace_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        fasta, bb = make_input(tmp, m, nq, sites)
        tree, out = os.path.join(tmp, "bb.nwk"), os.path.join(tmp, "out")
        fmt = ["-i", "m", "-d", "2"]
        dc = [EXE] + fmt + ["-m", "3", "-I", bb, "-O", tree]
        add = [EXE] + fmt + ["-a", "-t", tree, "-I", fasta, "-O", out + ".nwk"]
        jpl = [EXE] + fmt + ["-a", "-t", tree, "-I", fasta, "-o", "j", "-O", out + ".jplace"]
        if mode == "kernels":
            arms = [("dc_backbone", dc, {}), ("jplace_reevaluate", jpl, {}), ("jplace_carry", jpl, {"DPR_PFIX_CARRY": "1"})]
            if not run_dir:
                r = subprocess.run(dc, capture_output=True, text=True, env=env)
                assert r.returncode == 0, r.stderr[-400:]
                for tag, cmd, extra in arms:
                    print(tag, " ".join("%s=%s" % kv for kv in extra.items()), "rocprofv3 --kernel-trace --stats -d DIR --", " ".join(cmd))
                return
            for tag, cmd, extra in arms:      # (the first arm writes the backbone tree the other two read)
                d = os.path.join(run_dir, tag)
                r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd, capture_output=True,
                                   text=True, env=dict(env, DPR_CLI_NORMAL_EXIT="1", **extra))
                assert r.returncode == 0, r.stderr[-800:]
                for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        if any(k in row["Name"] for k in ("pfix_", "dc_assign_")):
                            print(json.dumps(dict(row, arm=tag, Name=row["Name"][:70])))      # Calls, TotalDurationNs, AverageNs, MinNs, MaxNs, ..
                for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    os.remove(path)      # (hundreds of thousands of placement launches in the backbone arm: the statistics are the record)
            print(json.dumps(dict(backbone=m, queries=nq, sites=sites, dc_query_x_edge=(m - m // 20) * (2 * (m // 20) - 2), jplace_query_x_edge=nq * (2 * m - 2))))
            return
        r = subprocess.run(dc, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-400:]
        keys = ("Distance Operation Time", "Tree Operation Time", "Placement Scan Time", "Bootstrap placements")
        for rep in range(reps):
            for tag, cmd in (("add", add), ("jplace", jpl)):
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, text=True, env=env)
                wall = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-400:]
                print(json.dumps(dict(arm=tag, rep=rep, backbone=m, queries=nq, sites=sites, wall_s=round(wall, 3), lines=lines(r.stderr, keys))))
        if boot > 0:
            t0 = time.perf_counter()
            r = subprocess.run(jpl + ["--bootstrap", str(boot)], capture_output=True, text=True, env=env)
            wall = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-400:]
            print(json.dumps(dict(arm="jplace_bootstrap", replicates=boot, backbone=m, queries=nq, sites=sites, wall_s=round(wall, 3),
                                  bytes=os.path.getsize(out + ".jplace"), lines=lines(r.stderr, keys))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
