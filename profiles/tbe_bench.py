"""Transfer bootstrap expectation timing: python profiles/tbe_bench.py [--tips 30000] [--sites 10000] [--replicates 20]
[--pairs 2] [--rocprof 30000,100000] [--out DIR (default profiles/tbe)]

The input is bench.py's aligned input (tools/gen_synth --model gtr+g+i --indel-gaps, branch lengths 2e-5 in [2e-6, 2e-4]),
written as FASTA, as in profiles/bootstrap_bench.py.  Records, one JSON line each, into DIR/tbe.jsonl:
  - `--bootstrap R` with `--bootstrap-metric fbp` and `tbe`, alternated (--pairs pairs, one rank): wall time and the command's
    own Bootstrap line; the first tbe run under DPR_LOG=cli, its per-replicate breakdown (resample, distances, NJ, transfer
    support) in DIR/breakdown.txt;
  - for every size of --rocprof: `rocprofv3 --kernel-trace --stats` of a process of its own (this script with --child) that
    calls dpr_transfer_support through the C ABI; the lines of tbe_kernel from its kernel statistics.  At the bench's size the
    trees are NJ trees of the input and of 3 replicates (dpr_set_msa, dpr_dist_matrix, dpr_nj_run, dpr_msa_resample); at
    other sizes they are random merge logs (the kernel's work, (n - 2)^2 node pairs, does not depend on the shape).  The
    command itself is not profiled: see profiles/bootstrap_bench.py.
Every command runs under its own time limit; the first failure ends the script."""
import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GEN = os.path.join(ROOT, "tools", "bin", "gen_synth")
LINE = re.compile(r"Bootstrap: (\d+) replicates \(seed (\d+)\) in (\d+) ms, ([0-9.]+) ms per replicate, (\d+) ranks")


def run(cmd, env=None, limit=600):
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, env=e)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"failed ({r.returncode}): {' '.join(cmd)}")
    return r, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--replicates", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--rocprof", default="30000,100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tbe"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--packed4", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="tbe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rec = open(os.path.join(a.out, "tbe.jsonl"), "a")

    def put(d):
        d.update(tips=a.tips, sites=a.sites)
        rec.write(json.dumps(d) + "\n")
        rec.flush()
        print(json.dumps(d), flush=True)

    try:
        fa = os.path.join(tmp, "aln.fa")
        p4 = os.path.join(tmp, "aln.p4")
        run([GEN, "--tips", str(a.tips), "--sites", str(a.sites), "--seed", "1", "--mean-bl", "2e-05", "--lo", "2e-06", "--hi", "0.0002",
             "--model", "gtr+g+i", "--indel-gaps", "--threads", "16", "--fasta", fa, "--packed4", p4], limit=300)
        base = ["-i", "m", "-I", fa, "-m", "2", "-d", "2", "--bootstrap", str(a.replicates)]
        texts = {}
        for i in range(a.pairs):
            for metric in ("fbp", "tbe"):
                out = os.path.join(tmp, f"{metric}.nwk")
                env = {"DPR_LOG": "cli"} if (metric == "tbe" and i == 0) else None
                r, wall = run([BIN, *base, "-O", out, "--bootstrap-metric", metric], env=env, limit=900)
                m = LINE.search(r.stderr)
                text = open(out).read()
                texts.setdefault(metric, text)
                put(dict(run=metric, pair=i, replicates=a.replicates, wall_s=round(wall, 3), bootstrap_ms=int(m.group(3)),
                         ms_per_replicate=float(m.group(4)), same_file_as_first=text == texts[metric],
                         same_tree_as_fbp=re.sub(r"\)\d+", ")", text) == re.sub(r"\)\d+", ")", texts["fbp"])))
                if env:
                    with open(os.path.join(a.out, "breakdown.txt"), "w") as f:
                        f.write("\n".join(l for l in r.stderr.splitlines() if l.startswith("  replicate") or l.startswith("  main tree")
                                          or l.startswith("Bootstrap:") or l.startswith("Tree Created")) + "\n")
        for n in [int(x) for x in a.rocprof.split(",") if x]:
            pdir = os.path.join(a.out, f"rocprof_{n}")
            shutil.rmtree(pdir, ignore_errors=True)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "3", "--tips", str(n), "--sites", str(a.sites)]
            if n == a.tips:
                cmd += ["--packed4", p4]
            r, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "tbe", "--", *cmd], limit=900)
            lines = []
            for p in glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True):
                rows = open(p).read().splitlines()
                lines += rows[:1] + [l for l in rows[1:] if "tbe_kernel" in l]
            put(dict(run="rocprof", kernel_tips=n, trees="nj" if n == a.tips else "random merge logs", kernel_stats=lines,
                     child=[l for l in r.stdout.splitlines() if l.startswith("replicate")]))
            for p in glob.glob(os.path.join(pdir, "**", "*"), recursive=True):
                if os.path.isfile(p) and not p.endswith("_stats.csv"):
                    os.remove(p)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def child(a):
    import torch  # noqa: F401  (the wheel's HIP runtime first: see profiles/bootstrap_bench.py)
    import numpy as np
    sys.path.insert(0, ROOT)
    import dipper_amd
    from dipper_amd import capi
    from tests import _tbe
    n = a.tips
    d = dipper_amd.Dipper(0)
    if a.packed4:
        W = (a.sites + 15) // 16
        d.set_msa(np.fromfile(a.packed4, dtype=np.uint64).reshape(n, W), a.sites)
        d.dist_matrix(capi.SRC_MSA, 2)
        main = d.nj_run()
        mx, my = main["merge_x"], main["merge_y"]
    else:
        rng = np.random.default_rng(1)
        mx, my = _tbe.random_log(rng, n)
    phi = np.zeros(n - 2, dtype=np.int64)
    for r in range(a.child):
        if a.packed4:
            d.msa_resample(1, r)
            d.dist_matrix(capi.SRC_MSA, 2)
            rep = d.nj_run()
            rx, ry = rep["merge_x"], rep["merge_y"]
        else:
            rx, ry = _tbe.shared_prefix(rng, n, mx, my)
        t0 = time.perf_counter()
        d.transfer_support(n, mx, my, rx, ry, phi)
        t1 = time.perf_counter()
        print(f"replicate {r}: transfer support {1e3 * (t1 - t0):.2f} ms (host + device)", flush=True)
    d.close()


if __name__ == "__main__":
    main()
