"""Time of the minimum spanning forest of the distances (dpr_mst_run, `dipper -o s`) on one GPU.  One JSON line per measurement on stdout
(and appended to --out).

    python tools/mst_bench.py --out profiles/mst/mst_bench.jsonl

Inputs from tools/bin/gen_synth (seeded, tips in shuffled order; nothing is read from outside the repository):
  library   --tips x --sites nucleotides (JC): one warm-up call and --reps timed ones.  Reported from HIP events, summed over the rounds
            of a call and per block: the row provider (full rows), the row minimum, the per-round component work and the copy of the
            count; beside them the rounds and the wall time of the whole call.  From the same process and the same block shape, the
            yardstick: --reps streams of neighbours at K = 1 (dpr_nearest_*), their select per block and its run-to-run spread -- one pass
            of mst_row_min_kernel over a block against one pass of nearest_select_kernel.  The row minimum's bytes per second count the
            distances of a block (8 x rows x ld) and the labels every row reads (4 x rows x n).
            --read-bases: the same call for --tips reads (Mash, k 15, S 1 000).
  command   `dipper -i m -d 2 -o s` at --tips x --sites and at --cli-tips x --cli-sites (a size whose matrix no device holds): wall
            time, the `MST:` line, the device line of DPR_LOG=cli with the peak device bytes.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _util  # noqa: E402

BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
MS = ("dist_ms", "rowmin_ms", "round_ms")


class step:
    """a GPU step under its own time limit: overrun = one line on stderr and the end of the process (status 124)"""

    def __init__(self, what, seconds):
        self.what, self.seconds = what, seconds

    def __enter__(self):
        def late(signum, frame):
            sys.stderr.write(f"[mst_bench] step '{self.what}' passed its limit of {self.seconds} s: stopping\n")
            sys.stderr.flush()
            os._exit(124)
        signal.signal(signal.SIGALRM, late)
        signal.setitimer(signal.ITIMER_REAL, self.seconds)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        signal.setitimer(signal.ITIMER_REAL, 0)
        sys.stderr.write(f"[mst_bench] {self.what}: {time.perf_counter() - self.t0:.2f} s\n")
        return False


def measure(d, src, dt, k, reps):
    with step("mst: warm-up (allocation, first launches)", 240):
        d.mst(src, dt, k)
    runs = []
    for _ in range(reps):
        with step("mst: timed", 240):
            t0 = time.perf_counter()
            got = d.mst(src, dt, k)
            wall = 1e3 * (time.perf_counter() - t0)
        runs.append(dict(wall_ms=wall, **{key: got["info"][key] for key in MS}))
    best = min(runs, key=lambda r: r["wall_ms"])
    st, n, rows = got["stats"], got["info"]["n"], got["info"]["block_rows"]
    ld = (n + 15) // 16 * 16
    walked = st["rows_walked"]      # rows of all rounds: every one reads ld distances and n labels
    per_block = [r["rowmin_ms"] / st["blocks"] for r in runs]
    return dict(rounds=st["rounds"], blocks=st["blocks"], block_rows=rows, edges=st["edges"], components=st["components"],
                peak_device_bytes=st["peak_device_bytes"], runs=runs, rowmin_ms_per_block=best["rowmin_ms"] / st["blocks"],
                rowmin_ms_per_block_runs=per_block, dist_ms_per_block=best["dist_ms"] / st["blocks"],
                round_ms_per_round=best["round_ms"] / st["rounds"],
                rowmin_gbytes_per_s=(8.0 * ld + 4.0 * n) * walked / best["rowmin_ms"] / 1e6, tree_length=float(got["d"].sum()))


def yardstick(d, src, dt, k, reps):
    """the select of a stream of neighbours at K = 1 over the same blocks of rows, per block, and its spread over the runs"""
    with step("nearest K 1: warm-up", 240):
        d.nearest(src, dt, k, K=1, keep=False)
    per_block, runs = [], []
    for _ in range(reps):
        with step("nearest K 1: timed", 240):
            got = d.nearest(src, dt, k, K=1, keep=False)
        runs.append({key: got["info"][key] for key in ("dist_ms", "select_ms", "copy_ms")})
        per_block.append(got["info"]["select_ms"] / got["stats"]["blocks"])
    return dict(K=1, blocks=got["stats"]["blocks"], block_rows=got["info"]["block_rows"], runs=runs, select_ms_per_block_runs=per_block,
                select_ms_per_block=min(per_block), select_ms_per_block_spread=max(per_block) - min(per_block))


def command(args, seconds, what):
    env = dict(os.environ, DPR_LOG="cli")
    with step(what, seconds):
        t0 = time.perf_counter()
        r = subprocess.run([BIN, *args], capture_output=True, text=True, env=env, timeout=seconds)
        wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(f"[mst_bench] {what}: exit status {r.returncode}")
    return wall, r.stderr


def whole_command(tmp, tag, tips, sites, seed, mean):
    with step("gen_synth for the whole command", 420):
        inp = _util.gen_synth(tmp, tag, tips, sites, seed, mean, mean / 10, mean * 10, shuffle=1, fasta=True)
    out = os.path.join(tmp, tag + ".tsv")
    wall, err = command(["-i", "m", "-I", inp["fasta"], "-d", "2", "-o", "s", "-O", out], 540, f"-o s, whole command, {tips} x {sites}")
    dev = re.search(r"device: (\d+) rounds, (\d+) blocks of (\d+) rows; distances (\S+) ms, row minimum (\S+) ms, components and copies (\S+) ms; "
                    r"peak device bytes (\d+)", err)
    rec = dict(input="whole command", tips=tips, sites=sites, wall_s=wall, file_bytes=os.path.getsize(out), matrix_bytes_never_allocated=8 * tips * tips,
               mst_line=[ln for ln in err.split("\n") if ln.startswith("MST:")],
               rounds=int(dev.group(1)) if dev else None, blocks=int(dev.group(2)) if dev else None, block_rows=int(dev.group(3)) if dev else None,
               dist_ms=float(dev.group(4)) if dev else None, rowmin_ms=float(dev.group(5)) if dev else None,
               round_ms=float(dev.group(6)) if dev else None, peak_device_bytes=int(dev.group(7)) if dev else None)
    os.unlink(out)
    os.unlink(inp["fasta"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--read-bases", type=int, default=2000, help="0: no Mash input")
    ap.add_argument("--cli-tips", type=int, default=300000, help="0: no whole command at the large size")
    ap.add_argument("--cli-sites", type=int, default=1000)
    ap.add_argument("--no-library", action="store_true", help="only the whole command at --cli-tips x --cli-sites")
    a = ap.parse_args()
    mean = 2e-4

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        if a.no_library:
            emit(whole_command(tmp, "big", a.cli_tips, a.cli_sites, 3, mean))
            return
        d = dipper_amd.Dipper(0)
        try:
            inp = _util.gen_synth(tmp, "a", a.tips, a.sites, 1, mean, mean / 10, mean * 10, shuffle=1)
            with step("upload", 120):
                d.set_msa(inp["packed4"], a.sites)
            rec = dict(input="alignment, JC", tips=a.tips, sites=a.sites, device=d.device_name())
            rec.update(measure(d, capi.SRC_MSA, capi.DIST_JC, 15, a.reps))
            emit(rec)
            rec = dict(input="alignment, JC: the select of -o n at K = 1 over the same blocks", tips=a.tips, sites=a.sites)
            rec.update(yardstick(d, capi.SRC_MSA, capi.DIST_JC, 15, a.reps))
            emit(rec)
            if a.read_bases:
                inp = _util.gen_synth(tmp, "r", a.tips, a.read_bases, 2, mean * 20, mean * 2, mean * 200, reads=True, shuffle=1)
                with step("upload and sketches", 240):
                    d.set_reads_packed(*inp["reads"])
                    d.sketch(k=15, S=1000, fetch=False)
                rec = dict(input="reads, Mash k 15 S 1000", tips=a.tips, bases=a.read_bases, index=d.mash_index_info()["built"])
                rec.update(measure(d, capi.SRC_MASH, 0, 15, 1))
                emit(rec)
        finally:
            d.close()
        emit(whole_command(tmp, "c", a.tips, a.sites, 1, mean))
        if a.cli_tips:
            emit(whole_command(tmp, "big", a.cli_tips, a.cli_sites, 3, mean))


if __name__ == "__main__":
    main()
