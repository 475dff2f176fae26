"""Time of the pairs within a distance threshold (dpr_pairs_*, `dipper -o p`) on one GPU.  One JSON line per measurement on stdout
(and appended to --out).

    python tools/pairs_bench.py --out profiles/pairs/pairs_bench.jsonl

Inputs from tools/bin/gen_synth (seeded, tips in shuffled order; nothing is read from outside the repository):
  library   30 000 x 1 000 and 30 000 x 10 000 nucleotides (JC) and 30 000 reads of ~2 000 bases (Mash, k 15, S 1 000).  Per input the
            thresholds that keep about 0.1 % and about 10 % of the pairs, taken as quantiles of the first 2 048 tips' pairs; per
            threshold one warm-up stream and --reps timed ones.  Reported from HIP events, summed over the blocks of a stream: the row
            provider (the distance kernel), count + scan + write + union, the copies of the pairs to the host; beside them the wall
            time of the whole stream.  The pairs are counted and dropped (the host does no formatting here).
  command   --cli-tips x --cli-sites: one whole `dipper -i m -d 2 -o p --within T --clusters FILE` at a size whose matrix no device
            holds, T the 0.01 % quantile of the 30 000 x 1 000 input, peak device bytes from the command's DPR_LOG=cli line; and at
            30 000 x 1 000 the wall time of `-o p` (T at 0.1 %) beside `-o d` written to /dev/null.
No torch.  Every GPU step runs under a time limit of its own; a step that overruns ends the process, nothing is started after it."""
import argparse
import json
import os
import re
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _util  # noqa: E402

BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
DBL_MAX = float(np.finfo(np.float64).max)


class step:
    """a GPU step under its own time limit: overrun = one line on stderr and the end of the process (status 124)"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def late(signum, frame):
            sys.stderr.write(f"[pairs_bench] step '{self.what}' passed its limit of {self.seconds} s: stopping\n")
            sys.stderr.flush()
            os._exit(124)
        signal.signal(signal.SIGALRM, late)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)
        sys.stderr.write(f"[pairs_bench] {self.what}: {time.perf_counter() - self.t0:.2f} s\n")
        return False


def quantiles(d, src, dt, k, qs):
    """thresholds at the quantiles qs of the distances among the first 2 048 tips (one block of a stream that keeps everything)"""
    d.pairs_begin(src, dt, k, threshold=DBL_MAX, block_rows=2048)
    try:
        _, _, dist, _ = d.pairs_next()
    finally:
        d.pairs_end()
    return [float(np.quantile(dist, q)) for q in qs]


def measure(d, src, dt, k, T, reps):
    with step("stream, warm-up (allocation, first launches)", 240):
        d.pairs_within(src, dt, k, threshold=T, keep=False)
    runs = []
    for _ in range(reps):
        with step("stream, timed", 240):
            t0 = time.perf_counter()
            got = d.pairs_within(src, dt, k, threshold=T, keep=False)
            wall = 1e3 * (time.perf_counter() - t0)
        runs.append(dict(wall_ms=wall, **{key: got["info"][key] for key in ("dist_ms", "filter_ms", "copy_ms")}))
    n = got["info"]["n"]
    best = min(runs, key=lambda r: r["wall_ms"])
    return dict(threshold=T, pairs=got["stats"]["pairs"], share=got["stats"]["pairs"] / (n * (n - 1) / 2), blocks=got["stats"]["blocks"],
                block_rows=got["info"]["block_rows"], clusters=got["stats"]["components"], largest=got["stats"]["largest"],
                peak_device_bytes=got["stats"]["peak_device_bytes"], runs=runs, filter_over_dist=best["filter_ms"] / best["dist_ms"],
                gpairs_per_s_wall=n * (n - 1) / 2 / best["wall_ms"] / 1e6)


def command(args, seconds, what):
    env = dict(os.environ, DPR_LOG="cli")
    with step(what, seconds):
        t0 = time.perf_counter()
        r = subprocess.run([BIN, *args], capture_output=True, text=True, env=env, timeout=seconds)
        wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(f"[pairs_bench] {what}: exit status {r.returncode}")
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", default="1000,10000")
    ap.add_argument("--read-bases", type=int, default=2000, help="0: no Mash input")
    ap.add_argument("--cli-tips", type=int, default=300000, help="0: no whole command")
    ap.add_argument("--cli-sites", type=int, default=1000)
    ap.add_argument("--matrix-command", action="store_true", help="also time -o d beside -o p at --tips x the first of --sites")
    a = ap.parse_args()
    recs = []
    mean = 2e-4
    small_T = None

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        d = dipper_amd.Dipper(0)
        try:
            for sites in [int(s) for s in a.sites.split(",") if s]:
                inp = _util.gen_synth(tmp, f"a{sites}", a.tips, sites, 1, mean, mean / 10, mean * 10, shuffle=1)
                with step("upload", 120):
                    d.set_msa(inp["packed4"], sites)
                with step("thresholds", 120):
                    T = quantiles(d, capi.SRC_MSA, capi.DIST_JC, 15, (1e-4, 1e-3, 0.1))
                if small_T is None:
                    small_T = T
                for q, t in ((1e-3, T[1]), (0.1, T[2])):
                    rec = dict(input="alignment, JC", tips=a.tips, sites=sites, device=d.device_name(), quantile=q)
                    rec.update(measure(d, capi.SRC_MSA, capi.DIST_JC, 15, t, a.reps))
                    emit(rec)
            if a.read_bases:
                inp = _util.gen_synth(tmp, "r", a.tips, a.read_bases, 2, mean * 20, mean * 2, mean * 200, reads=True, shuffle=1)
                with step("upload and sketches", 240):
                    d.set_reads_packed(*inp["reads"])
                    d.sketch(k=15, S=1000, fetch=False)
                with step("thresholds", 120):
                    T = quantiles(d, capi.SRC_MASH, 0, 15, (1e-3, 0.1))
                for q, t in ((1e-3, T[0]), (0.1, T[1])):
                    rec = dict(input="reads, Mash k 15 S 1000", tips=a.tips, bases=a.read_bases, device=d.device_name(), quantile=q, index=d.mash_index_info()["built"])
                    rec.update(measure(d, capi.SRC_MASH, 0, 15, t, a.reps))
                    emit(rec)
        finally:
            d.close()
        if a.matrix_command and small_T is not None:
            sites = int(a.sites.split(",")[0])
            inp = _util.gen_synth(tmp, "c", a.tips, sites, 1, mean, mean / 10, mean * 10, shuffle=1, fasta=True)
            wp, err = command(["-i", "m", "-I", inp["fasta"], "-d", "2", "-o", "p", "--within", repr(small_T[1]), "-O", os.path.join(tmp, "c.tsv")], 300, "-o p")
            wd, _ = command(["-i", "m", "-I", inp["fasta"], "-d", "2", "-o", "d", "-O", "/dev/null"], 420, "-o d to /dev/null")
            emit(dict(input="whole commands", tips=a.tips, sites=sites, pairs_wall_s=wp, matrix_wall_s=wd, pairs_file_bytes=os.path.getsize(os.path.join(tmp, "c.tsv")),
                      pairs_line=[ln for ln in err.split("\n") if ln.startswith("Pairs:")]))
            os.unlink(os.path.join(tmp, "c.tsv"))
        if a.cli_tips and small_T is not None:
            with step("gen_synth for the whole command", 420):
                inp = _util.gen_synth(tmp, "big", a.cli_tips, a.cli_sites, 3, mean, mean / 10, mean * 10, shuffle=1, fasta=True)
            out, cl = os.path.join(tmp, "big.tsv"), os.path.join(tmp, "big.clusters")
            wall, err = command(["-i", "m", "-I", inp["fasta"], "-d", "2", "-o", "p", "--within", repr(small_T[0]), "-O", out, "--clusters", cl], 540, "-o p, whole command")
            dev = re.search(r"device: (\d+) blocks of (\d+) rows; distances (\S+) ms, filter and components (\S+) ms, copies (\S+) ms; peak device bytes (\d+)", err)
            emit(dict(input="whole command", tips=a.cli_tips, sites=a.cli_sites, threshold=small_T[0], wall_s=wall, pairs_file_bytes=os.path.getsize(out),
                      matrix_bytes_never_allocated=8 * a.cli_tips * a.cli_tips, pairs_line=[ln for ln in err.split("\n") if ln.startswith("Pairs:")],
                      blocks=int(dev.group(1)) if dev else None, block_rows=int(dev.group(2)) if dev else None, dist_ms=float(dev.group(3)) if dev else None,
                      filter_ms=float(dev.group(4)) if dev else None, copy_ms=float(dev.group(5)) if dev else None,
                      peak_device_bytes=int(dev.group(6)) if dev else None))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
