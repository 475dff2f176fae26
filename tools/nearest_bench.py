"""Time of each sequence's K nearest neighbours (dpr_nearest_*, `dipper -o n`) on one GPU.  One JSON line per measurement on stdout
(and appended to --out).

    python tools/nearest_bench.py --out profiles/nearest/nearest_bench.jsonl

Inputs from tools/bin/gen_synth (seeded, tips in shuffled order; nothing is read from outside the repository):
  library   --tips x --sites nucleotides (JC), K = 10 and 100: per K one warm-up stream and --reps timed ones.  Reported from HIP events,
            summed over the blocks of a stream and per block: the row provider (full rows), the select, the copies of the results; beside
            them the wall time of the whole stream.  From the same process and the same blocks of rows, the yardstick: a stream of pairs
            (dpr_pairs_*, threshold at the 0.1 % quantile) stepped block by block, its count + scan + write + union per block -- one pass
            of that filter over a block against one pass of the select; the last block of the stream of pairs is the one whose rows are
            (nearly) as wide as the select's.
            --read-bases: the same for --tips reads (Mash, k 15, S 1 000), K = 10.
  command   `dipper -i m -d 2 -o n --nearest 10` at --tips x --sites and at --cli-tips x --cli-sites (a size whose matrix no device
            holds): wall time, the `Nearest:` line, the device line of DPR_LOG=cli with the peak device bytes.
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
            sys.stderr.write(f"[nearest_bench] step '{self.what}' passed its limit of {self.seconds} s: stopping\n")
            sys.stderr.flush()
            os._exit(124)
        signal.signal(signal.SIGALRM, late)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)
        sys.stderr.write(f"[nearest_bench] {self.what}: {time.perf_counter() - self.t0:.2f} s\n")
        return False


def per_block(begin, step_once, info, end, keys):
    """a stream stepped block by block: the event times of every block as the differences of the stream's running sums"""
    begin()
    try:
        n = info()["n"]
        out, done, last = [], 0, {k: 0.0 for k in keys}
        while done < n:
            done = step_once()
            now = info()
            out.append({k: now[k] - last[k] for k in keys})
            last = now
    finally:
        end()
    return out


def nearest_blocks(d, src, dt, k, K):
    def once():
        _, _, cnt, row0 = d.nearest_next(K, copy=False)
        return row0 + len(cnt)
    return per_block(lambda: d.nearest_begin(src, dt, k, K), once, d.nearest_info, d.nearest_end, ("dist_ms", "select_ms", "copy_ms"))


def pairs_blocks(d, src, dt, k, T):
    return per_block(lambda: d.pairs_begin(src, dt, k, threshold=T), lambda: d.pairs_next(copy=False)[3], d.pairs_info, d.pairs_end,
                     ("dist_ms", "filter_ms", "copy_ms"))


def quantile_threshold(d, src, dt, k, q):
    d.pairs_begin(src, dt, k, threshold=DBL_MAX, block_rows=2048)
    try:
        _, _, dist, _ = d.pairs_next()
    finally:
        d.pairs_end()
    return float(np.quantile(dist, q))


def measure(d, src, dt, k, K, reps):
    with step(f"K {K}: stream, warm-up (allocation, first launches)", 240):
        d.nearest(src, dt, k, K=K, keep=False)
    runs = []
    for _ in range(reps):
        with step(f"K {K}: stream, timed", 240):
            t0 = time.perf_counter()
            got = d.nearest(src, dt, k, K=K, keep=False)
            wall = 1e3 * (time.perf_counter() - t0)
        runs.append(dict(wall_ms=wall, **{key: got["info"][key] for key in ("dist_ms", "select_ms", "copy_ms")}))
    with step(f"K {K}: stream, block by block", 240):
        blocks = nearest_blocks(d, src, dt, k, K)
    best = min(runs, key=lambda r: r["wall_ms"])
    n, nb = got["info"]["n"], got["stats"]["blocks"]
    return dict(K=K, neighbours=got["stats"]["neighbours"], blocks=nb, block_rows=got["info"]["block_rows"], early_selections=got["stats"]["flushes"],
                peak_device_bytes=got["stats"]["peak_device_bytes"], runs=runs, select_ms_per_block=best["select_ms"] / nb,
                dist_ms_per_block=best["dist_ms"] / nb, select_over_dist=best["select_ms"] / best["dist_ms"],
                select_gbytes_per_s=8.0 * n * n / best["select_ms"] / 1e6, per_block=blocks)


def yardstick(d, src, dt, k):
    """one pass of the -o p filter over the same blocks of rows (its rows end at the diagonal block: the last block is the widest)"""
    with step("pairs: threshold", 120):
        T = quantile_threshold(d, src, dt, k, 1e-3)
    with step("pairs: stream, warm-up", 240):
        d.pairs_within(src, dt, k, threshold=T, keep=False)
    with step("pairs: stream, block by block", 240):
        blocks = pairs_blocks(d, src, dt, k, T)
    return dict(threshold=T, per_block=blocks, filter_ms_last_block=blocks[-1]["filter_ms"], filter_ms_sum=sum(b["filter_ms"] for b in blocks),
                dist_ms_sum=sum(b["dist_ms"] for b in blocks))


def command(args, seconds, what):
    env = dict(os.environ, DPR_LOG="cli")
    with step(what, seconds):
        t0 = time.perf_counter()
        r = subprocess.run([BIN, *args], capture_output=True, text=True, env=env, timeout=seconds)
        wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(f"[nearest_bench] {what}: exit status {r.returncode}")
    return wall, r.stderr


def whole_command(tmp, tag, tips, sites, seed, mean, K):
    with step("gen_synth for the whole command", 420):
        inp = _util.gen_synth(tmp, tag, tips, sites, seed, mean, mean / 10, mean * 10, shuffle=1, fasta=True)
    out = os.path.join(tmp, tag + ".tsv")
    wall, err = command(["-i", "m", "-I", inp["fasta"], "-d", "2", "-o", "n", "--nearest", str(K), "-O", out], 540, f"-o n, whole command, {tips} x {sites}")
    dev = re.search(r"device: (\d+) blocks of (\d+) rows; distances (\S+) ms, select (\S+) ms \((\d+) early selections\), copies (\S+) ms; peak device bytes (\d+)", err)
    rec = dict(input="whole command", tips=tips, sites=sites, K=K, wall_s=wall, file_bytes=os.path.getsize(out), matrix_bytes_never_allocated=8 * tips * tips,
               nearest_line=[ln for ln in err.split("\n") if ln.startswith("Nearest:")],
               blocks=int(dev.group(1)) if dev else None, block_rows=int(dev.group(2)) if dev else None, dist_ms=float(dev.group(3)) if dev else None,
               select_ms=float(dev.group(4)) if dev else None, early_selections=int(dev.group(5)) if dev else None,
               copy_ms=float(dev.group(6)) if dev else None, peak_device_bytes=int(dev.group(7)) if dev else None)
    os.unlink(out)
    os.unlink(inp["fasta"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--read-bases", type=int, default=2000, help="0: no Mash input")
    ap.add_argument("--cli-tips", type=int, default=300000, help="0: no whole command at the large size")
    ap.add_argument("--cli-sites", type=int, default=1000)
    ap.add_argument("--no-library", action="store_true", help="only the whole command at --cli-tips x --cli-sites")
    a = ap.parse_args()
    recs = []
    mean = 2e-4

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        if a.no_library:
            emit(whole_command(tmp, "big", a.cli_tips, a.cli_sites, 3, mean, 10))
            return
        d = dipper_amd.Dipper(0)
        try:
            inp = _util.gen_synth(tmp, "a", a.tips, a.sites, 1, mean, mean / 10, mean * 10, shuffle=1)
            with step("upload", 120):
                d.set_msa(inp["packed4"], a.sites)
            for K in [int(s) for s in a.ks.split(",") if s]:
                rec = dict(input="alignment, JC", tips=a.tips, sites=a.sites, device=d.device_name())
                rec.update(measure(d, capi.SRC_MSA, capi.DIST_JC, 15, K, a.reps))
                emit(rec)
            rec = dict(input="alignment, JC: the -o p filter over the same blocks", tips=a.tips, sites=a.sites)
            rec.update(yardstick(d, capi.SRC_MSA, capi.DIST_JC, 15))
            emit(rec)
            if a.read_bases:
                inp = _util.gen_synth(tmp, "r", a.tips, a.read_bases, 2, mean * 20, mean * 2, mean * 200, reads=True, shuffle=1)
                with step("upload and sketches", 240):
                    d.set_reads_packed(*inp["reads"])
                    d.sketch(k=15, S=1000, fetch=False)
                rec = dict(input="reads, Mash k 15 S 1000", tips=a.tips, bases=a.read_bases, index=d.mash_index_info()["built"])
                rec.update(measure(d, capi.SRC_MASH, 0, 15, 10, 1))
                emit(rec)
        finally:
            d.close()
        emit(whole_command(tmp, "c", a.tips, a.sites, 1, mean, 10))
        if a.cli_tips:
            emit(whole_command(tmp, "big", a.cli_tips, a.cli_sites, 3, mean, 10))


if __name__ == "__main__":
    main()
