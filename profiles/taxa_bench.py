"""Per-taxon transfer index timing: python profiles/taxa_bench.py [--tips 30000] [--sites 10000] [--replicates 20] [--pairs 2]
[--rocprof 30000,100000] [--parent-bin PATH] [--out DIR (default profiles/taxa)]

The input is bench.py's aligned input, as in profiles/tbe_bench.py.  Records, one JSON line each, into DIR/taxa.jsonl:
  - the whole command, `--bootstrap R`, alternated (--pairs rounds, one rank) over the arms: the parent commit's binary with
    `--bootstrap-metric tbe` (only with --parent-bin: a build of the parent commit), this build with tbe, this build with tbe
    and --bootstrap-taxa, this build with fbp and --bootstrap-taxa; wall time and the command's own Bootstrap line.  The first
    round runs this build's tbe arms under DPR_LOG=cli: their per-replicate lines (the last field is the whole
    dpr_transfer_support / dpr_transfer_taxa call; the library's own lap of the host ordering) go to DIR/breakdown.txt;
  - for every size of --rocprof: `rocprofv3 --kernel-trace --stats` of a process of its own (this script with --child) that calls
    dpr_transfer_taxa and dpr_transfer_support through the C ABI; the lines of tbe_kernel and tbe_moved_kernel from its kernel
    statistics.  Trees as in profiles/tbe_bench.py: NJ trees of the input and its replicates at the bench's size, random merge
    logs elsewhere;
  - `rocprofv3 --hip-trace --stats` (a run of its own) of the child with 1 and with 4 replicates on random logs: the calls of
    hipMalloc and hipStreamSynchronize -- the difference is what three more replicates add.
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


def stats_rows(pdir, suffix, keep):
    lines = []
    for p in glob.glob(os.path.join(pdir, "**", "*" + suffix), recursive=True):
        rows = open(p).read().splitlines()
        lines += rows[:1] + [l for l in rows[1:] if any(k in l for k in keep)]
    for p in glob.glob(os.path.join(pdir, "**", "*"), recursive=True):
        if os.path.isfile(p) and not p.endswith("_stats.csv"):
            os.remove(p)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--replicates", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--rocprof", default="30000,100000")
    ap.add_argument("--parent-bin", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taxa"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--packed4", default="", help=argparse.SUPPRESS)
    ap.add_argument("--taxa-only", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="taxa_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rec = open(os.path.join(a.out, "taxa.jsonl"), "a")

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
        taxa = os.path.join(tmp, "taxa.tsv")
        arms = [("parent tbe", a.parent_bin, ["--bootstrap-metric", "tbe"]),
                ("tbe", BIN, ["--bootstrap-metric", "tbe"]),
                ("tbe + taxa", BIN, ["--bootstrap-metric", "tbe", "--bootstrap-taxa", taxa]),
                ("fbp + taxa", BIN, ["--bootstrap-metric", "fbp", "--bootstrap-taxa", taxa])]
        texts, reports, breakdown = {}, {}, []
        for i in range(a.pairs):
            for arm, exe, extra in arms:
                if not exe:
                    continue
                out = os.path.join(tmp, "out.nwk")
                log = i == 0 and exe == BIN and "tbe" in extra
                r, wall = run([exe, *base, "-O", out, *extra], env={"DPR_LOG": "cli"} if log else None, limit=900)
                m = LINE.search(r.stderr)
                text = open(out).read()
                metric = extra[1]
                texts.setdefault(metric, text)
                d = dict(run=arm, pair=i, replicates=a.replicates, wall_s=round(wall, 3), bootstrap_ms=int(m.group(3)),
                         ms_per_replicate=float(m.group(4)), cli_log=log, same_newick_as_first_of_metric=text == texts[metric])
                if "--bootstrap-taxa" in extra:
                    rep = open(taxa).read()
                    reports.setdefault("taxa", rep)
                    d.update(same_report_as_first=rep == reports["taxa"], report_head=rep.split("\n", 1)[0],
                             stderr_line=[l for l in r.stderr.splitlines() if l.startswith("Transfer index:")][0])
                put(d)
                if log:
                    breakdown += [f"== {arm}"] + [l for l in r.stderr.splitlines() if l.startswith("  replicate") or l.startswith("  main tree")
                                                  or l.startswith("    transfer taxa") or l.startswith("Bootstrap:")
                                                  or l.startswith("Transfer index:") or l.startswith("Tree Created")]
        if breakdown:
            with open(os.path.join(a.out, "breakdown.txt"), "w") as f:
                f.write("\n".join(breakdown) + "\n")
        me = [sys.executable, os.path.abspath(__file__), "--sites", str(a.sites)]
        for n in [int(x) for x in a.rocprof.split(",") if x]:
            pdir = os.path.join(a.out, f"rocprof_{n}")
            shutil.rmtree(pdir, ignore_errors=True)
            cmd = [*me, "--child", "3", "--tips", str(n)] + (["--packed4", p4] if n == a.tips else [])
            r, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "taxa", "--", *cmd], limit=900)
            put(dict(run="rocprof", kernel_tips=n, trees="nj" if n == a.tips else "random merge logs",
                     kernel_stats=stats_rows(pdir, "kernel_stats.csv", ("tbe_kernel", "tbe_moved_kernel")),
                     child=[l for l in r.stdout.splitlines() if l.startswith("replicate")]))
        for reps in (1, 4):
            pdir = os.path.join(a.out, f"hiptrace_{reps}")
            shutil.rmtree(pdir, ignore_errors=True)
            cmd = [*me, "--child", str(reps), "--tips", str(a.tips), "--taxa-only", "1"]
            run(["rocprofv3", "--hip-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "taxa", "--", *cmd], limit=900)
            put(dict(run="hip api calls", kernel_tips=a.tips, child_replicates=reps,
                     api_stats=stats_rows(pdir, "hip_api_stats.csv", ("hipMalloc", "hipStreamSynchronize", "hipFree", "hipMemcpy", "hipMemset"))))
            shutil.rmtree(pdir, ignore_errors=True)
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
    phi, moved, pairs = np.zeros(n - 2, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(1, dtype=np.int64)
    plain = np.zeros(n - 2, dtype=np.int64)
    for r in range(a.child):
        if a.packed4:
            d.msa_resample(1, r)
            d.dist_matrix(capi.SRC_MSA, 2)
            rep = d.nj_run()
            rx, ry = rep["merge_x"], rep["merge_y"]
        else:
            rx, ry = _tbe.shared_prefix(rng, n, mx, my)
        t0 = time.perf_counter()
        d.transfer_taxa(n, mx, my, rx, ry, 300, phi, moved, pairs)
        t1 = time.perf_counter()
        if not a.taxa_only:
            d.transfer_support(n, mx, my, rx, ry, plain)
        t2 = time.perf_counter()
        print(f"replicate {r}: transfer taxa {1e3 * (t1 - t0):.2f} ms, transfer support {1e3 * (t2 - t1):.2f} ms (host + device); "
              f"pairs so far {int(pairs[0])}, sum moved {int(moved.sum())}", flush=True)
    d.close()


if __name__ == "__main__":
    main()
