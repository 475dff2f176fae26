"""Bootstrap support timing on the bench's flagship input: python profiles/bootstrap_bench.py [--tips 30000] [--sites 10000]
[--replicates 20] [--ranks 1,2,4] [--rocprof 3] [--out DIR (default profiles/bootstrap)]

The input is bench.py's aligned input (tools/gen_synth --model gtr+g+i --indel-gaps, branch lengths 2e-5 in [2e-6, 2e-4]),
written as FASTA.  Records, one JSON line each, into DIR/bootstrap.jsonl:
  - the plain command (-m 2);
  - `--bootstrap R` with 1, 2, 4 ranks on ONE GPU (--devices 0,0,..): wall time, the command's own Bootstrap line (time of the
    replicate phase incl. the sum over the ranks, mean time of a replicate on rank 0), replicates per second;
  - the one-rank run under DPR_LOG=cli: its per-replicate breakdown (resample, distances, NJ, split count) in
    DIR/breakdown.txt;
  - with --rocprof K: `rocprofv3 --kernel-trace --stats` of the same flow with K replicates, one rank, in a run of its own
    (DIR/rocprof/), and the lines of the new kernels from its kernel statistics.  The profiled process is this script
    (--child): torch imported first, then the command's calls through the C ABI (dpr_set_msa, dpr_dist_matrix, dpr_nj_run, then
    per replicate dpr_msa_resample, dpr_dist_matrix, dpr_nj_run, dpr_split_support) -- rocprofv3 --kernel-trace segfaults
    inside the first hipGraphLaunch of the pruned NJ loop of a process on the system HIP runtime (NOTES.md), the command is one.
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
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--rocprof", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--packed4", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="boot_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rec = open(os.path.join(a.out, "bootstrap.jsonl"), "a")

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
        base = ["-i", "m", "-I", fa, "-m", "2", "-d", "2"]
        out_plain = os.path.join(tmp, "plain.nwk")
        r, wall = run([BIN, *base, "-O", out_plain])
        put(dict(run="plain", wall_s=round(wall, 3), tree_ms=int(re.search(r"Tree Created in: (\d+)", r.stderr).group(1))))
        plain = open(out_plain).read()
        first = None
        for G in [int(x) for x in a.ranks.split(",") if x]:      # (--ranks "": the rocprof leg alone)
            out = os.path.join(tmp, f"boot_{G}.nwk")
            cmd = [BIN, *base, "-O", out, "--bootstrap", str(a.replicates)]
            if G > 1:
                cmd += ["--devices", ",".join(["0"] * G)]
            env = {"DPR_LOG": "cli"} if G == 1 else None
            r, wall = run(cmd, env=env, limit=900)
            m = re.search(r"Bootstrap: (\d+) replicates \(seed (\d+)\) in (\d+) ms, ([0-9.]+) ms per replicate, (\d+) ranks", r.stderr)
            text = open(out).read()
            if first is None:
                first = text
            put(dict(run="bootstrap", ranks=G, replicates=a.replicates, wall_s=round(wall, 3), bootstrap_ms=int(m.group(3)),
                     rank0_ms_per_replicate=float(m.group(4)), replicates_per_s=round(a.replicates / (int(m.group(3)) / 1000.0), 3),
                     tree_equals_plain_without_labels=re.sub(r"\)\d+", ")", text) == plain, same_file_as_one_rank=text == first))
            if G == 1:
                with open(os.path.join(a.out, "breakdown.txt"), "w") as f:
                    f.write("\n".join(l for l in r.stderr.splitlines() if l.startswith("  replicate") or l.startswith("  main tree")
                                      or l.startswith("Bootstrap:") or l.startswith("Tree Created")) + "\n")
        if a.rocprof:
            pdir = os.path.join(a.out, "rocprof")
            shutil.rmtree(pdir, ignore_errors=True)
            r, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "boot", "--", sys.executable, os.path.abspath(__file__),
                        "--child", str(a.rocprof), "--packed4", p4, "--tips", str(a.tips), "--sites", str(a.sites)], limit=900)
            stats = glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True)
            lines = []
            for p in stats:
                rows = open(p).read().splitlines()
                lines += rows[:1] + [l for l in rows[1:] if re.search(r"boot_|msa_xstage|mi_scan|msa_dist_kernel", l)]
            put(dict(run="rocprof", replicates=a.rocprof, kernel_stats=lines,
                     child=[l for l in r.stdout.splitlines() if l.startswith("replicate")]))
            # keep the statistics, not the trace databases
            for p in glob.glob(os.path.join(pdir, "**", "*"), recursive=True):
                if os.path.isfile(p) and not p.endswith("_stats.csv"):
                    os.remove(p)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def child(a):
    import torch  # noqa: F401  (the wheel's HIP runtime first: see the docstring)
    import numpy as np
    sys.path.insert(0, ROOT)
    import dipper_amd
    from dipper_amd import capi
    W = (a.sites + 15) // 16
    packed = np.fromfile(a.packed4, dtype=np.uint64).reshape(a.tips, W)
    d = dipper_amd.Dipper(0)
    d.set_msa(packed, a.sites)
    d.dist_matrix(capi.SRC_MSA, 2)
    main = d.nj_run()
    counts = np.zeros(a.tips - 2, dtype=np.int32)
    for r in range(a.child):
        t0 = time.perf_counter()
        d.msa_resample(1, r)
        t1 = time.perf_counter()
        d.dist_matrix(capi.SRC_MSA, 2)
        rep = d.nj_run()
        t2 = time.perf_counter()
        capi.split_support(a.tips, main["merge_x"], main["merge_y"], rep["merge_x"], rep["merge_y"], counts)
        t3 = time.perf_counter()
        print(f"replicate {r}: resample {1e3 * (t1 - t0):.2f} ms, distances + NJ {1e3 * (t2 - t1):.1f} ms, split count "
              f"{1e3 * (t3 - t2):.2f} ms", flush=True)
    d.close()


if __name__ == "__main__":
    main()
